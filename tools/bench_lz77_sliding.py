"""Times the sliding-window LZ77 device layer -- index, parse, replay (csrc/scl_lz77_sliding.hip) -- on a batch of streams,
next to the greedy batch path (csrc/scl_lz77.hip, L = 6, M = 64) on the same bytes in the same run.  Recorded, not gated:
profiles/lz77_sliding_bench.txt.

    python tools/bench_lz77_sliding.py [--streams 4096] [--stream-kib 64] [--steps 10] [--warmup 2] [--out FILE]

Data: the first-order Markov source of bench_data.py over 16 symbols, one chain per stream (generated on the device), as
tools/bench_lz77.py.  The sliding coder runs with the reference's defaults: hash_length 4, hash_table_size 1 000 000,
max_chain_length 64, lazy, minimum_match_length 4, window_size 1 000 000.  Kernel time only: HIP events around each call on
the current stream, buffers and scratch allocated once; medians.  Both round trips are verified: the replay of the parse's
output must restore the input.  That the sequences are the reference's is the business of tests/test_gpu_lz77_sliding.py.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stanford_compression_library_amd import bench_data  # noqa: E402
from stanford_compression_library_amd.backend import lib  # noqa: E402
from stanford_compression_library_amd.backend import lz77  # noqa: E402

L, M = 6, 64


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


def run(name, win, n_streams, stream_len, steps, warmup, dev, sliding):
    total = n_streams * stream_len
    win_off = torch.arange(n_streams + 1, dtype=torch.int64, device=dev) * stream_len
    start = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    have = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    out = torch.empty_like(win)
    if sliding:
        params = lz77.SlidingParams()
        seq_cap = lz77.sliding_seq_cap(stream_len, params.min_match_length)
        scratch = torch.empty(lz77.sliding_scratch_bytes(total, n_streams), dtype=torch.uint8, device=dev)
        res = lz77.sliding_parse_batch(win, win_off, start, params, seq_cap, scratch=scratch)

        def parse(phases):
            return lz77.sliding_parse_batch(win, win_off, start, params, scratch=scratch, out=res, phases=phases)

        def replay():
            return lz77.sliding_replay_batch(out, win_off, have, res.literal_count, res.match_length, res.match_offset,
                                             res.n_seq, res.literals, res.lit_off, res.n_lit, params.window_size)
        kernels = lz77.sliding_kernel_names()
    else:
        seq_cap = lz77.default_seq_cap(stream_len, L)
        scratch = torch.empty(lz77.scratch_bytes(total, n_streams), dtype=torch.uint8, device=dev)
        res = lz77.parse_batch(win, win_off, start, L, M, seq_cap, scratch=scratch)

        def parse(phases):
            return lz77.parse_batch(win, win_off, start, L, M, seq_cap, scratch=scratch, out=res, phases=phases)

        def replay():
            return lz77.replay_batch(out, win_off, have, res.literal_count, res.match_length, res.match_offset, res.n_seq,
                                     res.literals, res.lit_off, res.n_lit)
        kernels = lz77.kernel_names()
    lines, medians = [], {}
    for what, fn in (("index", lambda: parse(lib.LZ77_INDEX)), ("parse", lambda: parse(lib.LZ77_PARSE)), ("replay", replay)):
        ms = timed(fn, steps, warmup)
        medians[what] = statistics.median(ms)
        lines.append(f"{name:28s} {what:6s}: median {medians[what]:10.3f} ms  min {min(ms):10.3f}  max {max(ms):10.3f}  "
                     f"{total / medians[what] / 1e6:8.3f} GB/s of input")
    out.fill_(0)
    out_len, status = replay()
    torch.cuda.synchronize()
    ok = bool((res.status == 0).all() and (status == 0).all() and (out_len == stream_len).all() and torch.equal(out, win))
    n_seq, n_lit = int(res.n_seq.to(torch.int64).sum()), int(res.n_lit.to(torch.int64).sum())
    matches = int((res.match_length != 0).sum())
    lines.append(f"{name:28s} {n_seq} sequences ({matches} with a match), {n_lit} literals "
                 f"({total / max(matches, 1):.1f} input bytes per match), kernels {', '.join(kernels)}, {steps} timed steps "
                 f"after {warmup}, round trip {'ok' if ok else 'FAILED'}")
    return lines, medians, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-kib", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    stream_len = args.stream_kib << 10
    win = bench_data.markov1_chunks_device(16, args.streams, stream_len, 77, dev).reshape(-1)
    shape = f"{args.streams} x {args.stream_kib} KiB"
    lines = [f"{torch.cuda.get_device_name(0)}; markov1 over 16 symbols, {shape}"]
    all_ok = True
    results = {}
    for label, sliding in ((f"sliding {shape}", True), (f"greedy L=6 M=64 {shape}", False)):
        rows, results[sliding], ok = run(label, win, args.streams, stream_len, args.steps, args.warmup, dev, sliding)
        lines += rows
        all_ok = all_ok and ok
    lines.append("sliding / greedy, same run: " + ", ".join(
        f"{what} {results[True][what] / results[False][what]:.2f}x" for what in ("index", "parse", "replay")))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
