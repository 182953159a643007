"""Times ONE large Huffman block coded by the whole grid (csrc/scl_prefix_block.hip) against the two other ways to code the
same bytes.  Recorded, not gated: profiles/prefix_block_bench.txt.

    python tools/bench_prefix_block.py [--sizes-mib 16,256,1024] [--steps 20] [--warmup 5] [--out FILE]

Data: the i.i.d. byte source of bench_data.py (t256 table); the Huffman code is built from the data's histogram, as in
tools/bench_prefix.py.  HIP events on the current stream, buffers allocated once.
  (a) encode_block_into / decode_block_device of one block per size, with the decoder's sync_passes;
  (b) the same 16 MiB block as ONE chunk of the batched kernels (one lane codes it): a single timed step;
  (c) the same bytes as 4 KiB chunks through the batched kernels: the yardstick of profiles/prefix_bench.txt;
  (d) the sweep behind PrefixModel.BLOCK_PARALLEL_MIN: encode_host / decode_host end to end (wall clock, best of 3)
      through the block path and through the one-lane path, 4 Ki to 1 Mi symbols.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd import bench_data  # noqa: E402
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import HuffmanTree  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402

from bench_prefix import timed  # noqa: E402


def line(name, what, ms, raw, extra=""):
    med = statistics.median(ms)
    return (f"{name:28s} {what}: median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  "
            f"{raw / med / 1e6:8.2f} GB/s of symbols{extra}")


def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="16,256,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) << 20 for s in args.sizes_mib.split(",")]
    lib.require_device()
    dev = torch.device("cuda:0")
    freq = bench_data.t256_table()
    sym = bench_data.iid_chunks_device(freq, max(sizes) // 4096, 4096, 1, dev).reshape(-1)
    hist = torch.bincount(sym[:16 << 20].to(torch.int64), minlength=256).cpu().numpy().astype(np.float64)
    probs = np.maximum(hist, 1.0)
    probs /= probs.sum()
    table = HuffmanTree(ProbabilityDist({i: float(p) for i, p in enumerate(probs)})).get_encoding_table()
    lengths = np.array([len(table[i]) for i in range(256)], np.uint8)
    codes = np.array([int(table[i].to01(), 2) for i in range(256)], np.uint32)
    model = models.PrefixModel(codes, lengths)
    info = model.block_info()
    lines = [f"prefix-code block bench: i.i.d. t256 source, {args.warmup} warm-up + {args.steps} timed steps, HIP events, "
             f"{torch.cuda.get_device_name(0)}",
             f"huffman table: lengths {int(lengths.min())}..{int(lengths.max())} bits; block geometry: sub_bits "
             f"{info.sub_bits}, tile_symbols {info.tile_symbols}, code_len_gcd {info.code_len_gcd}",
             "(a) one block, the whole grid"]
    for n in sizes:
        block = sym[:n]
        out = torch.empty(model.slot_bytes(n), dtype=torch.uint8, device=dev)
        nbits, status = (int(v) for v in model.encode_block_into(block, out).cpu())
        dec = torch.empty(n, dtype=torch.uint8, device=dev)
        e_ms = timed(lambda: model.encode_block_into(block, out), args.steps, args.warmup)
        d_ms = timed(lambda: model.decode_block_device(out, nbits, out_cap=n, out=dec), args.steps, args.warmup)
        _, n_out, used, dstatus, passes = model.decode_block_device(out, nbits, out_cap=n, out=dec)
        ok = status == 0 and dstatus == 0 and n_out == n and used == nbits and torch.equal(dec, block)
        name = f"block {n >> 20:5d} MiB"
        lines.append(line(name, "encode", e_ms, n))
        lines.append(line(name, "decode", d_ms, n, f"  sync_passes {passes}"))
        lines.append(f"{name:28s} {nbits / n:.4f} bits/symbol, round trip {'ok' if ok else 'FAILED'}")
        del out, dec
    n = sizes[0]
    lines.append(f"(b) the {n >> 20} MiB block as one chunk of the batched kernels (one lane), a single step")
    row = sym[:n].reshape(1, n)
    enc = model.alloc_encoded(1, n, dev)
    out = model.alloc_decoded(1, n, dev)
    e_ms = timed(lambda: model.encode_batch(row, out=enc), 1, 0)
    d_ms = timed(lambda: model.decode_encoded(enc, n, out=out), 1, 0)
    ok = bool(int(enc.status[0]) == 0 and int(out[3][0]) == 0 and torch.equal(out[0][0, :n], row[0]))
    lines.append(line("one lane", "encode", e_ms, n))
    lines.append(line("one lane", "decode", d_ms, n, f"  round trip {'ok' if ok else 'FAILED'}"))
    del enc, out
    lines.append(f"(c) the same {n >> 20} MiB as {n // 4096} chunks of 4 KiB through the batched kernels")
    rows = sym[:n].reshape(n // 4096, 4096)
    enc = model.alloc_encoded(n // 4096, 4096, dev)
    out = model.alloc_decoded(n // 4096, 4096, dev)
    model.encode_batch(rows, out=enc)
    e_ms = timed(lambda: model.encode_batch(rows, out=enc), args.steps, args.warmup)
    d_ms = timed(lambda: model.decode_encoded(enc, 4096, out=out), args.steps, args.warmup)
    lines.append(line("batched 4 KiB chunks", "encode", e_ms, n))
    lines.append(line("batched 4 KiB chunks", "decode", d_ms, n))
    del enc, out
    lines.append("(d) encode_host / decode_host end to end, wall clock, best of 3: block path | one-lane path (ms)")
    one_lane = models.PrefixModel(codes, lengths)
    one_lane.BLOCK_PARALLEL_MIN = 1 << 62
    grid = models.PrefixModel(codes, lengths)
    grid.BLOCK_PARALLEL_MIN = 0
    host = sym[:1 << 20].cpu().numpy()
    for k in range(12, 21, 2):
        part = host[:1 << k]
        packed, nbits = grid.encode_host(part)
        packed1, nbits1 = one_lane.encode_host(part)
        same = nbits == nbits1 and np.array_equal(packed, packed1)
        e = best_of(lambda: grid.encode_host(part)), best_of(lambda: one_lane.encode_host(part))
        d = best_of(lambda: grid.decode_host(packed, nbits)), best_of(lambda: one_lane.decode_host(packed, nbits))
        lines.append(f"{1 << k:8d} symbols  encode {e[0]:9.3f} | {e[1]:9.3f}   decode {d[0]:9.3f} | {d[1]:9.3f}   "
                     f"streams {'equal' if same else 'DIFFER'}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
