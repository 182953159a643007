"""Times the integer codes -- Golomb, universal, Elias-delta -- on ONE block coded by the whole grid (csrc/scl_uint_block.hip),
with the Huffman block path on the same values as the yardstick and the host's numpy path beside it.  Recorded, not gated:
profiles/uint_codes_bench.txt.

    python tools/bench_uint_codes.py [--log2-values 24] [--steps 20] [--warmup 5] [--out FILE]

Data: one block of 2^24 values from a geometric source with mean about 8 (seeded).  Golomb runs at the M that codes this
block in the fewest bits (found on the host from the block itself, M = 1..32).  HIP events on the current stream, buffers
allocated once, medians of --steps after --warmup, round trip verified.
  (a) encode_block_into / decode_block_device of the block, per code, with the decoder's sync_passes;
  (b) the yardstick in the same process: the values clipped to bytes through PrefixModel.encode_block_into /
      decode_block_device under the Huffman code of their histogram (scl_prefix_*_block, the same kernels' bodies with a
      table in LDS);
  (c) the host numpy path of the classes on a 2^20 slice: wall clock, best of 3;
  (d) the sweep behind UINT_BLOCK_MIN: the classes' encode_block / decode_block end to end (wall clock, best of 3), host
      path against device path, 2^10 to 2^20 values in steps of 4x.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import (GolombUintDecoder, GolombUintEncoder, HuffmanTree,  # noqa: E402
                                                          UniversalUintDecoder, UniversalUintEncoder, _uint_block)
from stanford_compression_library_amd.compressors.elias_delta_uint_coder import (EliasDeltaUintDecoder,  # noqa: E402
                                                                                 EliasDeltaUintEncoder)
from stanford_compression_library_amd.core.data_block import DataBlock  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402

from bench_prefix import timed  # noqa: E402
from bench_prefix_block import best_of  # noqa: E402


def line(name, what, ms, n, extra=""):
    med = statistics.median(ms)
    return (f"{name:22s} {what}: median {med:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  "
            f"{n / med / 1e6:7.2f} G values/s{extra}")


def golomb_bits(values, M):
    b = M.bit_length() - 1
    cutoff = (2 << b) - M
    q, r = values // M, values % M
    return int((q + 1 + b + ((r >= cutoff) & (cutoff != M))).sum())


def class_coders(kind, M):
    if kind == "golomb":
        return GolombUintEncoder(M), GolombUintDecoder(M)
    if kind == "universal":
        return UniversalUintEncoder(), UniversalUintDecoder()
    return EliasDeltaUintEncoder(), EliasDeltaUintDecoder()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-values", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    n = 1 << args.log2_values
    host = (np.random.default_rng(8).geometric(1.0 / 9.0, n) - 1).astype(np.int64)
    best_m = min(range(1, 33), key=lambda M: golomb_bits(host[:1 << 20], M))
    codes = [("golomb", best_m), ("universal", None), ("elias_delta", None)]
    values = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev)
    lines = [f"integer-code block bench: {n} values, geometric source, mean {host.mean():.3f}, max {int(host.max())}; "
             f"{args.warmup} warm-up + {args.steps} timed steps, HIP events, {torch.cuda.get_device_name(0)}",
             f"Golomb at M = {best_m}, the M of the fewest bits for this source among 1..32",
             "(a) one block, the whole grid"]
    for kind, M in codes:
        code = models.UintCode(kind, M)
        out = torch.empty(4 * n + 16, dtype=torch.uint8, device=dev)
        dec = torch.empty(n, dtype=torch.int32, device=dev)
        es, _ = code._block_scratch(n, 0, dev)
        nbits, status = (int(v) for v in code.encode_block_into(values, out, scratch=es).cpu())
        ds, _ = code._block_scratch(0, nbits, dev)
        e_ms = timed(lambda: code.encode_block_into(values, out, scratch=es), args.steps, args.warmup)
        d_ms = timed(lambda: code.decode_block_device(out, nbits, out_cap=n, out=dec, scratch=ds), args.steps, args.warmup)
        _, n_out, used, dstatus, passes = code.decode_block_device(out, nbits, out_cap=n, out=dec, scratch=ds)
        ok = status == 0 and dstatus == 0 and n_out == n and used == nbits and torch.equal(dec, values)
        name = f"{kind}{'' if M is None else ' M=' + str(M)}"
        lines.append(line(name, "encode", e_ms, n))
        lines.append(line(name, "decode", d_ms, n, f"  sync_passes {passes}"))
        lines.append(f"{name:22s} {nbits / n:.4f} bits/value, round trip {'ok' if ok else 'FAILED'}")
        del out, dec, es, ds
    lines.append("(b) the yardstick: the values clipped to bytes, Huffman block path (scl_prefix_*_block), same process")
    clipped = np.minimum(host, 255).astype(np.uint8)
    probs = np.maximum(np.bincount(clipped, minlength=256).astype(np.float64), 2e-6 * n)  # (ProbabilityDist asks for >= 1e-6)
    probs /= probs.sum()
    table = HuffmanTree(ProbabilityDist({i: float(p) for i, p in enumerate(probs)})).get_encoding_table()
    lengths = np.array([len(table[i]) for i in range(256)], np.uint8)
    model = models.PrefixModel(np.array([int(table[i].to01(), 2) for i in range(256)], np.uint32), lengths)
    sym = torch.from_numpy(clipped).to(dev)
    out = torch.empty(model.slot_bytes(n), dtype=torch.uint8, device=dev)
    dec = torch.empty(n, dtype=torch.uint8, device=dev)
    nbits, status = (int(v) for v in model.encode_block_into(sym, out).cpu())
    e_ms = timed(lambda: model.encode_block_into(sym, out), args.steps, args.warmup)
    d_ms = timed(lambda: model.decode_block_device(out, nbits, out_cap=n, out=dec), args.steps, args.warmup)
    _, n_out, used, dstatus, passes = model.decode_block_device(out, nbits, out_cap=n, out=dec)
    ok = status == 0 and dstatus == 0 and n_out == n and used == nbits and torch.equal(dec, sym)
    lines.append(line("huffman (bytes)", "encode", e_ms, n))
    lines.append(line("huffman (bytes)", "decode", d_ms, n, f"  sync_passes {passes}"))
    lines.append(f"{'huffman (bytes)':22s} {nbits / n:.4f} bits/value, code lengths {int(lengths.min())}..{int(lengths.max())}, "
                 f"round trip {'ok' if ok else 'FAILED'}")
    del out, dec, sym

    small = host[:1 << 20].tolist()
    lines.append("(c) the classes' host numpy path, 2^20 values, wall clock, best of 3")
    saved = _uint_block.UINT_BLOCK_MIN
    _uint_block.UINT_BLOCK_MIN = 1 << 62
    for kind, M in codes:
        enc, dec_ = class_coders(kind, M)
        bits = enc.encode_block(DataBlock(small))
        e = best_of(lambda: enc.encode_block(DataBlock(small)))
        d = best_of(lambda: dec_.decode_block(bits))
        lines.append(f"{kind:12s} encode {e:10.3f} ms  decode {d:10.3f} ms  ({len(small) / e / 1e3:.2f} / "
                     f"{len(small) / d / 1e3:.2f} M values/s)")
    lines.append("(d) encode_block / decode_block end to end, wall clock, best of 3: device path | host path (ms)")
    for k in range(10, 21, 2):
        part = small[:1 << k]
        for kind, M in codes:
            enc, dec_ = class_coders(kind, M)
            _uint_block.UINT_BLOCK_MIN = 0
            bits = enc.encode_block(DataBlock(part))
            e_dev = best_of(lambda: enc.encode_block(DataBlock(part)))
            d_dev = best_of(lambda: dec_.decode_block(bits))
            back = dec_.decode_block(bits)[0].data_list
            _uint_block.UINT_BLOCK_MIN = 1 << 62
            same = enc.encode_block(DataBlock(part)) == bits and back == part
            e_host = best_of(lambda: enc.encode_block(DataBlock(part)))
            d_host = best_of(lambda: dec_.decode_block(bits))
            lines.append(f"{1 << k:8d} values {kind:12s} encode {e_dev:9.3f} | {e_host:9.3f}   decode {d_dev:9.3f} | "
                         f"{d_host:9.3f}   {len(bits):9d} bits, streams {'equal' if same else 'DIFFER'}")
    _uint_block.UINT_BLOCK_MIN = saved
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
