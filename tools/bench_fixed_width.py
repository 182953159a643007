"""Times the fixed-width kernels (csrc/scl_fixed.hip) against a device-to-device copy, and sweeps the classes' host path against
their device path for the threshold ``FIXED_BLOCK_MIN``.  Recorded, not gated.  profiles/fixed_width_bench.txt.

    python tools/bench_fixed_width.py [--mib 1024] [--steps 10] [--warmup 3] [--out FILE]

(a) 1 GiB of byte symbols at w in {1, 3, 8}, uniform indices below 2^w, as one stream and as 262 144 streams of 4 KiB.  (A
    stream's length in bits is a uint32: 1 GiB of symbols at w = 8 is 2^33 bits, so "one stream" is four of 256 MiB there.)
    HIP events around the call on the current stream, buffers allocated once, medians of --steps after --warmup, round trip
    verified.  The call includes what the entry point does besides the kernel: the upload of the widths and alphabet sizes
    (2 MiB for 262 144 streams) and the zeroing of the status words.
    GB/s = algorithmic bytes (symbols + stream) per second.  The yardstick of the SAME run: ``copy_`` of a buffer of half
    that many bytes -- a copy reads and writes every byte, so it moves as many bytes as the kernel does.  ratio = kernel
    median / copy median.
(b) ``encode_block`` / ``decode_block`` of FixedBitwidthEncoder / Decoder end to end, wall clock, best of 3, 1 Ki to 1 Mi
    symbols over 256 in steps of 4x: the host path (numpy) against the device path (scl_fixed_*_host), chosen by setting the
    threshold.  The threshold to write next to ``FIXED_BLOCK_MIN`` is the smallest swept size from which the device never
    loses, on encode and on decode.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd.backend import lib, models  # noqa: E402
from stanford_compression_library_amd.compressors import fixed_bitwidth_compressor as fbc  # noqa: E402
from stanford_compression_library_amd.core.data_block import DataBlock  # noqa: E402

from bench_prefix import timed  # noqa: E402
from bench_prefix_block import best_of  # noqa: E402


def kernel_rows(code, total, n_streams, width, steps, warmup, dev):
    chunk_len = total // n_streams
    sym = torch.randint(0, 1 << width, (n_streams, chunk_len), dtype=torch.uint8, device=dev)
    enc = code.alloc_encoded(n_streams, chunk_len, dev, width=width)
    dec = code.alloc_decoded(n_streams, chunk_len, dev, torch.uint8)
    K = 1 << width
    code.encode_batch(sym, None, width, K, out=enc)
    val, lens, used, status = code.decode_encoded(enc, None, width, K, chunk_len, out=dec)
    ok = (not enc.status.any().item() and not status.any().item() and torch.equal(val, sym)
          and bool((lens == chunk_len).all().item()))
    stream_bytes = total * width // 8
    moved = total + stream_bytes
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    e_ms = statistics.median(timed(lambda: code.encode_batch(sym, None, width, K, out=enc), steps, warmup))
    d_ms = statistics.median(timed(lambda: code.decode_encoded(enc, None, width, K, chunk_len, out=dec), steps, warmup))
    c_ms = statistics.median(timed(lambda: b.copy_(a), steps, warmup))
    shape = f"{n_streams} x {chunk_len}"
    return (f"w={width}  {shape:>18s}  encode {e_ms:7.3f} ms {moved / e_ms / 1e6:7.1f} GB/s  decode {d_ms:7.3f} ms "
            f"{moved / d_ms / 1e6:7.1f} GB/s  copy of {moved // 2} B {c_ms:7.3f} ms {moved / c_ms / 1e6:7.1f} GB/s  "
            f"ratio encode {e_ms / c_ms:5.2f} decode {d_ms / c_ms:5.2f}  round trip {'ok' if ok else 'FAILED'}")


def sweep_rows():
    rng = np.random.default_rng(4)
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    keep = fbc.FIXED_BLOCK_MIN
    lines, never_loses = [], None
    try:
        for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20):
            data = rng.integers(0, 256, n)
            data[:256] = np.arange(256)
            block = DataBlock(data.tolist())
            t = {}
            for path, threshold in (("host", 1 << 62), ("device", 1)):
                fbc.FIXED_BLOCK_MIN = threshold
                bits = enc.encode_block(block)
                assert dec.decode_block(bits)[0].data_list == block.data_list
                t[path, "enc"] = best_of(lambda: enc.encode_block(block))
                t[path, "dec"] = best_of(lambda: dec.decode_block(bits))
            wins = t["device", "enc"] <= t["host", "enc"] and t["device", "dec"] <= t["host", "dec"]
            never_loses = (never_loses or n) if wins else None
            lines.append(f"{n:8d} symbols  encode host {t['host', 'enc']:9.3f} ms device {t['device', 'enc']:9.3f} ms   "
                         f"decode host {t['host', 'dec']:9.3f} ms device {t['device', 'dec']:9.3f} ms   "
                         f"device {'wins' if wins else 'loses'}")
    finally:
        fbc.FIXED_BLOCK_MIN = keep
    lines.append(f"smallest swept size from which the device never loses: {never_loses}  (FIXED_BLOCK_MIN is {keep})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    code = models.FixedWidthCode()
    total = args.mib << 20
    lines = [f"fixed-width bench: {args.mib} MiB of byte symbols, uniform below 2^w; {args.warmup} warm-up + {args.steps} timed "
             f"steps, medians, HIP events, {torch.cuda.get_device_name(0)}; kernels {code.kernel_names(1, 1)}",
             "(a) streams x symbols; GB/s of symbols + stream; the copy moves as many bytes (half as large, read and written)"]
    for width in (1, 3, 8):
        one = 1
        while (total // one) * width >= (1 << 32):  # a stream's bits are counted in 32
            one *= 2
        for n_streams in (one, total // 4096):
            lines.append(kernel_rows(code, total, n_streams, width, args.steps, args.warmup, dev))
            torch.cuda.empty_cache()
    lines.append("(b) FixedBitwidthEncoder.encode_block / Decoder.decode_block end to end, 256 symbols, wall clock, best of 3")
    lines += sweep_rows()
    lines.append("not measured: uint16 / uint32 rows, ragged batches, decode at odd bit offsets, kernel time by rocprofv3")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
