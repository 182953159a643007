"""Times the tuned prefix-code (Huffman) encode and decode kernels at the headline shape, with the rANS headline kernels
timed in the same process as the yardstick.  Recorded, not gated: profiles/prefix_bench.txt.

    python tools/bench_prefix.py [--chunks 262144] [--chunk-len 4096] [--steps 20] [--warmup 5] [--out FILE]

Data: the i.i.d. byte source of bench_data.py (t256 table); the Huffman code is built from the data's histogram.
Kernel time only: HIP events around each batch call on the current stream, buffers allocated once.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd import bench_data  # noqa: E402
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import HuffmanTree  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=262144)
    ap.add_argument("--chunk-len", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    freq = bench_data.t256_table()
    sym = bench_data.iid_chunks_device(freq, args.chunks, args.chunk_len, 1, dev)
    hist = torch.bincount(sym.reshape(-1).to(torch.int64), minlength=256).cpu().numpy().astype(np.float64)
    probs = np.maximum(hist, 1.0)
    probs /= probs.sum()
    table = HuffmanTree(ProbabilityDist({i: float(p) for i, p in enumerate(probs)})).get_encoding_table()
    lengths = np.array([len(table[i]) for i in range(256)], np.uint8)
    codes = np.array([int(table[i].to01(), 2) for i in range(256)], np.uint32)
    coders = {"huffman": models.PrefixModel(codes, lengths),
              "rans (yardstick)": models.RansModel(freq.tolist(), 1 << 16, 1, 32)}
    raw = args.chunks * args.chunk_len
    lines = [f"prefix-code bench: {args.chunks} chunks x {args.chunk_len} bytes = {raw / 2**30:.3f} GiB, i.i.d. t256 source, "
             f"{args.warmup} warm-up + {args.steps} timed steps, HIP events, {torch.cuda.get_device_name(0)}",
             f"huffman table: lengths {int(lengths.min())}..{int(lengths.max())} bits, "
             f"lut_bits {coders['huffman'].info().lut_bits}, fast_path {coders['huffman'].info().fast_path}"]
    for name, model in coders.items():
        enc = model.alloc_encoded(args.chunks, args.chunk_len, dev)
        model.encode_batch(sym, out=enc)
        out = model.alloc_decoded(args.chunks, args.chunk_len, dev)
        e_ms = timed(lambda: model.encode_batch(sym, out=enc), args.steps, args.warmup)
        d_ms = timed(lambda: model.decode_encoded(enc, args.chunk_len, out=out), args.steps, args.warmup)
        dsym, dlens, _, status = model.decode_encoded(enc, args.chunk_len, out=out)
        ok = bool((status == 0).all() and (enc.status == 0).all() and (dlens == args.chunk_len).all()
                  and torch.equal(dsym, sym))
        bits = float(enc.nbits.to(torch.float64).sum().item()) / raw
        kernels = model.kernel_names(args.chunks)
        for what, ms, k in (("encode", e_ms, kernels[0]), ("decode", d_ms, kernels[1])):
            med = statistics.median(ms)
            lines.append(f"{name:17s} {what}: median {med:7.3f} ms  min {min(ms):7.3f}  max {max(ms):7.3f}  "
                         f"{raw / med / 1e6:8.1f} GB/s of symbols  [{k.split('<')[0]}]")
        lines.append(f"{name:17s} {bits:.4f} bits/symbol, round trip {'ok' if ok else 'FAILED'}")
        del enc, out
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
