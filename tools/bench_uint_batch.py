"""Times the batched integer coders -- Golomb, universal, Elias-delta, one wavefront lane per chunk (csrc/scl_uint.hip) -- with
the block kernels and the Huffman batch path on the same values as yardsticks.  Recorded, not gated -- but for one rule: the
tuned kernel pair stays in the library only while it beats the any-parameter pair by more than 3 % on both encode and decode
at this shape.  profiles/uint_batch_bench.txt.

    python tools/bench_uint_batch.py [--chunks 65536] [--chunk-len 1024] [--steps 20] [--warmup 5] [--out FILE]

Data: 65 536 chunks of 1024 values from the geometric source of tools/bench_uint_codes.py (mean about 8, seeded); codes Golomb
M = 6, universal, Elias-delta.  HIP events on the current stream, buffers allocated once, medians of --steps after --warmup,
round trip verified, one process.
  (a) encode_batch / decode_batch, tuned and any-parameter kernels, measured twice in alternation (the spread of this box);
  (b) the same with one value in 1024 replaced by a uniform 32-bit one (Golomb: by a run up to 1024 ones -- a uniform 32-bit
      value is 2^32 / 6 ones): universal and Elias-delta codewords of 33 to 64 bits;
  (c) the yardsticks: the block kernels (scl_uint_*_block) on the concatenation of (a), and scl_prefix_*_batch on the values
      clipped to bytes under the Huffman code of their histogram;
  (d) the classes end to end, wall clock, best of 3: encode_blocks / decode_blocks against a loop of encode_block /
      decode_block over 4096 blocks of 1024 values.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import HuffmanTree, _uint_block  # noqa: E402
from stanford_compression_library_amd.core.data_block import DataBlock  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402

from bench_prefix import timed  # noqa: E402
from bench_prefix_block import best_of  # noqa: E402
from bench_uint_codes import class_coders  # noqa: E402

CODES = [("golomb", 6), ("universal", None), ("elias_delta", None)]


def row(name, what, ms, n, extra=""):
    med = statistics.median(ms)
    return (f"{name:26s} {what}: median {med:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  "
            f"{n / med / 1e6:7.2f} G values/s{extra}")


def batch_rows(name, code, values, stride, steps, warmup):
    """(a) / (b): both kernel pairs on one batch in slots of ``stride`` bytes, in alternation
    -> (lines, {(side, form): best median})"""
    n_chunks, chunk_len = values.shape
    n = n_chunks * chunk_len
    dev = values.device
    enc = code.alloc_encoded(n_chunks, chunk_len, dev, stride)
    dec = code.alloc_decoded(n_chunks, chunk_len, dev)
    lines, best = [], {}
    for any_kernels in (False, True):  # the two pairs write the same bytes
        code.encode_batch(values, out=enc, any_parameter_kernels=any_kernels)
        val, lens, used, status = code.decode_encoded(enc, chunk_len, out=dec, any_parameter_kernels=any_kernels)
        ok = (not enc.status.any().item() and not status.any().item() and torch.equal(val, values)
              and torch.equal(used, enc.nbits) and bool((lens == chunk_len).all().item()))
        bits = int(enc.nbits.to(torch.int64).sum().item())
        form = "any-parameter" if any_kernels else "tuned"
        lines.append(f"{name:26s} {form}: {bits / n:.4f} bits/value, slot {enc.stride} bytes, round trip {'ok' if ok else 'FAILED'}")
    for rnd in (1, 2):
        for any_kernels in (False, True):
            form = "any-parameter" if any_kernels else "tuned"
            e_ms = timed(lambda: code.encode_batch(values, out=enc, any_parameter_kernels=any_kernels), steps, warmup)
            d_ms = timed(lambda: code.decode_encoded(enc, chunk_len, out=dec, any_parameter_kernels=any_kernels), steps, warmup)
            lines.append(row(name, f"{form:13s} encode #{rnd}", e_ms, n))
            lines.append(row(name, f"{form:13s} decode #{rnd}", d_ms, n))
            for side, ms in (("encode", e_ms), ("decode", d_ms)):
                best[side, form] = min(best.get((side, form), 1e30), statistics.median(ms))
    for side in ("encode", "decode"):
        gain = best[side, "any-parameter"] / best[side, "tuned"] - 1.0
        lines.append(f"{name:26s} {side}: tuned over any-parameter {100 * gain:+.1f} % (the better median of each)")
    return lines, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=65536)
    ap.add_argument("--chunk-len", type=int, default=1024)
    ap.add_argument("--class-blocks", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    n_chunks, chunk_len = args.chunks, args.chunk_len
    n = n_chunks * chunk_len
    rng = np.random.default_rng(8)
    host = (rng.geometric(1.0 / 9.0, n) - 1).astype(np.int64)
    values = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev).view(n_chunks, chunk_len)
    spots = rng.random(n) < 1.0 / 1024
    lines = [f"integer-code batch bench: {n_chunks} chunks of {chunk_len} values, geometric source, mean {host.mean():.3f}, max "
             f"{int(host.max())}; {args.warmup} warm-up + {args.steps} timed steps, HIP events, {torch.cuda.get_device_name(0)}",
             "(a) one lane per chunk, both kernel pairs, twice in alternation"]
    verdict = []
    for kind, M in CODES:
        name = f"{kind}{'' if M is None else ' M=' + str(M)}"
        code = models.UintCode(kind, M)
        got, best = batch_rows(name, code, values, code.slot_bytes(chunk_len, int(host.max())), args.steps, args.warmup)
        lines += got
        verdict.append((name, best))
    lines.append("(b) one value in 1024 replaced: a uniform 32-bit value (Golomb: a run of up to 1024 ones)")
    for kind, M in CODES:
        name = f"{kind}{'' if M is None else ' M=' + str(M)} +wide"
        wide = host.copy()
        wide[spots] = rng.integers(0, 1024 * M if kind == "golomb" else 1 << 32, int(spots.sum()))
        wide_values = torch.from_numpy(wide.astype(np.uint32).view(np.int32)).to(dev).view(n_chunks, chunk_len)
        # (the slot of chunk_len values of the largest one is 8 KiB a chunk: sized from the batch's own lengths instead)
        code = models.UintCode(kind, M)
        longest = int(_uint_block.code_lengths(code, wide).reshape(n_chunks, chunk_len).sum(axis=1).max())
        got, _ = batch_rows(name, code, wide_values, (longest + 127) // 128 * 16, args.steps, args.warmup)
        lines += got
        del wide_values
    lines.append("(c) yardsticks, same process: the block kernels on the concatenation; Huffman batch on the values clipped to bytes")
    flat = values.reshape(-1)
    for kind, M in CODES:
        code = models.UintCode(kind, M)
        name = f"{kind}{'' if M is None else ' M=' + str(M)} block"
        out = torch.empty(4 * n + 16, dtype=torch.uint8, device=dev)
        dec = torch.empty(n, dtype=torch.int32, device=dev)
        es, _ = code._block_scratch(n, 0, dev)
        nbits, status = (int(v) for v in code.encode_block_into(flat, out, scratch=es).cpu())
        ds, _ = code._block_scratch(0, nbits, dev)
        e_ms = timed(lambda: code.encode_block_into(flat, out, scratch=es), args.steps, args.warmup)
        d_ms = timed(lambda: code.decode_block_device(out, nbits, out_cap=n, out=dec, scratch=ds), args.steps, args.warmup)
        _, n_out, used, dstatus, _ = code.decode_block_device(out, nbits, out_cap=n, out=dec, scratch=ds)
        ok = status == 0 and dstatus == 0 and n_out == n and used == nbits and torch.equal(dec, flat)
        lines.append(row(name, "encode", e_ms, n))
        lines.append(row(name, "decode", d_ms, n, f"  round trip {'ok' if ok else 'FAILED'}"))
        del out, dec, es, ds
    clipped = np.minimum(host, 255).astype(np.uint8)
    probs = np.maximum(np.bincount(clipped, minlength=256).astype(np.float64), 2e-6 * n)  # (ProbabilityDist asks for >= 1e-6)
    probs /= probs.sum()
    table = HuffmanTree(ProbabilityDist({i: float(p) for i, p in enumerate(probs)})).get_encoding_table()
    model = models.PrefixModel(np.array([int(table[i].to01(), 2) for i in range(256)], np.uint32),
                               np.array([len(table[i]) for i in range(256)], np.uint8))
    sym = torch.from_numpy(clipped).to(dev).view(n_chunks, chunk_len)
    enc = model.alloc_encoded(n_chunks, chunk_len, dev)
    dec = model.alloc_decoded(n_chunks, chunk_len, dev)
    model.encode_batch(sym, out=enc)
    back, _, used, status = model.decode_encoded(enc, chunk_len, out=dec)
    ok = not enc.status.any().item() and not status.any().item() and torch.equal(back, sym) and torch.equal(used, enc.nbits)
    e_ms = timed(lambda: model.encode_batch(sym, out=enc), args.steps, args.warmup)
    d_ms = timed(lambda: model.decode_encoded(enc, chunk_len, out=dec), args.steps, args.warmup)
    lines.append(row("huffman batch (bytes)", "encode", e_ms, n))
    lines.append(row("huffman batch (bytes)", "decode", d_ms, n, f"  round trip {'ok' if ok else 'FAILED'}"))
    del enc, dec, sym

    nb = args.class_blocks
    lines.append(f"(d) the classes end to end, {nb} blocks of {chunk_len} values, wall clock, best of 3: "
                 "encode_blocks / decode_blocks | a loop of encode_block / decode_block (ms)")
    blocks = [DataBlock(host[k * chunk_len: (k + 1) * chunk_len].tolist()) for k in range(nb)]
    for kind, M in CODES:
        enc_, dec_ = class_coders(kind, M)
        bits = enc_.encode_blocks(blocks)
        same = bits == [enc_.encode_block(b) for b in blocks]
        back = dec_.decode_blocks(bits)
        same = same and [b.data_list for b, _ in back] == [b.data_list for b in blocks]
        e_batch = best_of(lambda: enc_.encode_blocks(blocks))
        d_batch = best_of(lambda: dec_.decode_blocks(bits))
        e_loop = best_of(lambda: [enc_.encode_block(b) for b in blocks])
        d_loop = best_of(lambda: [dec_.decode_block(b) for b in bits])
        lines.append(f"{kind:12s} encode {e_batch:10.1f} | {e_loop:10.1f}   decode {d_batch:10.1f} | {d_loop:10.1f}   "
                     f"({nb * chunk_len / e_batch / 1e3:.2f} | {nb * chunk_len / e_loop / 1e3:.2f} M values/s encode, "
                     f"{nb * chunk_len / d_batch / 1e3:.2f} | {nb * chunk_len / d_loop / 1e3:.2f} decode), "
                     f"results {'equal' if same else 'DIFFER'}")
    lines.append("the 3 % rule at shape (a): the tuned pair stays if it wins by more than 3 % on encode AND decode")
    for name, best in verdict:
        e = best["encode", "any-parameter"] / best["encode", "tuned"] - 1.0
        d = best["decode", "any-parameter"] / best["decode", "tuned"] - 1.0
        lines.append(f"{name:26s} encode {100 * e:+.1f} %  decode {100 * d:+.1f} %  -> {'keep' if min(e, d) > 0.03 else 'drop'}")
    lines.append("not measured: other chunk lengths and chunk counts, ragged batches, rows the tuned kernels do not take, "
                 "kernel time by rocprofv3, the host path of the classes at this shape beyond the loop above")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
