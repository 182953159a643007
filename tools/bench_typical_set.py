"""Times the typical-set coder (csrc/scl_typical.hip): the table build on the device, ONE block coded by the whole grid with the
Huffman block path on the same symbols as the yardstick, and the classes end to end.  Recorded, not gated:
profiles/typical_set_bench.txt.

    python tools/bench_typical_set.py [--log2-symbols 26] [--steps 20] [--warmup 5] [--reference-ms MS] [--out FILE]

  (a) the table build: TypicalSetModel(...) -- upload, three kernels, the read-back of the count, two allocations -- between HIP
      events, median of 10, at (K, n) = (3, 10), (4, 12), (2, 24); beside it the same enumeration in Python on the CPU at
      (3, 10) (generate_typical_set_coder_lookup_tables of this package: the reference's loop) and, with --reference-ms, the
      reference's own function as timed where it is checked out;
  (b) one block of 2^26 symbols of {0.6, 0.3, 0.1} in chunks of 10 at eps = 0.1: encode_block_into / decode_block_device
      between HIP events, buffers allocated once, medians of --steps after --warmup, round trip verified;
  (c) the yardstick in the same process: the same symbols through PrefixModel.encode_block_into / decode_block_device under
      their Huffman code;
  (d) the classes' encode_block / decode_block end to end (wall clock, best of 3), 2^10 to 2^20 symbols in steps of 4x.  There
      is no host path to hold against: every block goes to the device.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import HuffmanTree  # noqa: E402
from stanford_compression_library_amd.compressors import typical_set_coder as tsc  # noqa: E402
from stanford_compression_library_amd.core.data_block import DataBlock  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402

from bench_prefix import timed  # noqa: E402
from bench_prefix_block import best_of  # noqa: E402

DISTS = {3: {"A": 0.6, "B": 0.3, "C": 0.1}, 4: {"A": 0.4, "B": 0.3, "C": 0.2, "D": 0.1}, 2: {"A": 0.7, "B": 0.3}}


def line(name, what, ms, n, extra=""):
    med = statistics.median(ms)
    return (f"{name:22s} {what}: median {med:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  "
            f"{n / med / 1e6:7.2f} G symbols/s{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-symbols", type=int, default=26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reference-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    lines = [f"typical-set bench: {torch.cuda.get_device_name(0)}", "(a) the table build, HIP events around TypicalSetModel(...), median of 10"]
    for K, n in ((3, 10), (4, 12), (2, 24)):
        params = tsc.TypicalSetCoderParams(n, 0.1, ProbabilityDist(DISTS[K]))
        nlp, entropy = tsc.model_inputs(params)
        made = []  # (kept until the timing is over: freeing a table waits for the device)
        ms = timed(lambda: made.append(models.TypicalSetModel(nlp, n, entropy, 0.1)), 10, 2)
        model = made[-1]
        lines.append(f"K = {K}, n = {n:2d}: {K ** n:9d} tuples, {model.count:9d} typical, bt {model.bt} bo {model.bo}: median "
                     f"{statistics.median(ms):8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}")
        for m in made:
            m.close()
    params = tsc.TypicalSetCoderParams(10, 0.1, ProbabilityDist(DISTS[3]))
    t0 = time.perf_counter()
    typical, _ = tsc.generate_typical_set_coder_lookup_tables(params)
    lines.append(f"K = 3, n = 10 in Python on the CPU (this package's generate_typical_set_coder_lookup_tables, one run): "
                 f"{(time.perf_counter() - t0) * 1e3:.0f} ms, {len(typical)} typical")
    if args.reference_ms is not None:
        lines.append(f"K = 3, n = 10, the reference's generate_typical_set_coder_lookup_tables, as timed on the CPU where it is "
                     f"checked out (one run): {args.reference_ms:.0f} ms; its classes run it twice")

    n_sym = (1 << args.log2_symbols) // 10 * 10
    nlp, entropy = tsc.model_inputs(params)
    model = models.TypicalSetModel(nlp, 10, entropy, 0.1)
    host = np.random.default_rng(0).choice(3, size=n_sym, p=[0.6, 0.3, 0.1]).astype(np.uint8)
    sym = torch.from_numpy(host).to(dev)
    lines.append(f"(b) one block of {n_sym} symbols ({n_sym // 10} chunks of 10), the whole grid; {args.warmup} warm-up + {args.steps} "
                 "timed steps, HIP events")
    out = torch.empty(model.slot_bytes(n_sym), dtype=torch.uint8, device=dev)
    dec = torch.empty(n_sym, dtype=torch.uint8, device=dev)
    es = model.block_scratch(n_sym, 0, dev)
    nbits, status = (int(v) for v in model.encode_block_into(sym, out, scratch=es).cpu())
    ds = model.block_scratch(0, nbits, dev)
    e_ms = timed(lambda: model.encode_block_into(sym, out, scratch=es), args.steps, args.warmup)
    d_ms = timed(lambda: model.decode_block_device(out, nbits, out_cap=n_sym, out=dec, scratch=ds), args.steps, args.warmup)
    _, n_out, used, dstatus, passes = model.decode_block_device(out, nbits, out_cap=n_sym, out=dec, scratch=ds)
    ok = status == 0 and dstatus == 0 and n_out == n_sym and used == nbits and torch.equal(dec, sym)
    lines.append(line("typical set", "encode", e_ms, n_sym))
    lines.append(line("typical set", "decode", d_ms, n_sym, f"  sync_passes {passes}"))
    lines.append(f"{'typical set':22s} {nbits / n_sym:.4f} bits/symbol (entropy {entropy:.4f}), {model.count} typical of {model.N}, "
                 f"codewords of {1 + model.bt} and {1 + model.bo} bits, round trip {'ok' if ok else 'FAILED'}")
    del out, dec, es, ds

    lines.append("(c) the yardstick: the same symbols, Huffman block path (scl_prefix_*_block), same process")
    table = HuffmanTree(ProbabilityDist({0: 0.6, 1: 0.3, 2: 0.1})).get_encoding_table()
    lengths = np.array([len(table[i]) for i in range(3)], np.uint8)
    huff = models.PrefixModel(np.array([int(table[i].to01(), 2) for i in range(3)], np.uint32), lengths)
    out = torch.empty(huff.slot_bytes(n_sym), dtype=torch.uint8, device=dev)
    dec = torch.empty(n_sym, dtype=torch.uint8, device=dev)
    nbits, status = (int(v) for v in huff.encode_block_into(sym, out).cpu())
    e_ms = timed(lambda: huff.encode_block_into(sym, out), args.steps, args.warmup)
    d_ms = timed(lambda: huff.decode_block_device(out, nbits, out_cap=n_sym, out=dec), args.steps, args.warmup)
    _, n_out, used, dstatus, passes = huff.decode_block_device(out, nbits, out_cap=n_sym, out=dec)
    ok = status == 0 and dstatus == 0 and n_out == n_sym and used == nbits and torch.equal(dec, sym)
    lines.append(line("huffman", "encode", e_ms, n_sym))
    lines.append(line("huffman", "decode", d_ms, n_sym, f"  sync_passes {passes}"))
    lines.append(f"{'huffman':22s} {nbits / n_sym:.4f} bits/symbol, round trip {'ok' if ok else 'FAILED'}")
    del out, dec

    lines.append("(d) the classes' encode_block / decode_block end to end, wall clock, best of 3 (ms); every block goes to the device")
    enc, dec_ = tsc.TypicalSetEncoder(params), tsc.TypicalSetDecoder(params)
    names = "ABC"
    for k in range(10, 21, 2):
        part = [names[i] for i in host[:(1 << k) // 10 * 10].tolist()]
        bits = enc.encode_block(DataBlock(part))
        e = best_of(lambda: enc.encode_block(DataBlock(part)))
        d = best_of(lambda: dec_.decode_block(bits))
        same = dec_.decode_block(bits)[0].data_list == part
        lines.append(f"{len(part):8d} symbols  encode {e:9.3f}   decode {d:9.3f}   {len(bits):9d} bits, round trip "
                     f"{'ok' if same else 'FAILED'}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
