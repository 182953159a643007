"""Times the sliding-window LZ77 device layer -- index, parse, replay (csrc/scl_lz77_sliding.hip) -- on a batch of streams,
next to the greedy batch path (csrc/scl_lz77.hip, L = 6, M = 64) on the same bytes in the same run.  Recorded, not gated:
profiles/lz77_sliding_bench.txt.

    python tools/bench_lz77_sliding.py [--streams 4096] [--stream-kib 64] [--steps 10] [--warmup 2] [--out FILE]
    python tools/bench_lz77_sliding.py --wide [--wide-kib 64,256,1024,4096,16384] [--wide-sources markov,all-equal,random]
                                       [--lib FILE] [--out FILE]

--wide times ONE stream on both paths in the same run -- the one-wave kernels (sliding_parse_batch / sliding_replay_batch of
a batch of one) and the wide ones (sliding_parse_wide phase by phase, sliding_replay_wide; csrc/scl_lz77_sliding_wide.hip) --
on the Markov source, on all-equal bytes and on random bytes, checks at every size that both paths give the same sequences
and literals and that both replays restore the input, and prints the lines scl_lz77_sliding_wide_threshold() and the 10x
gate at the largest size are read from: profiles/lz77_sliding_wide_bench.txt.  The walk follows what an earlier walk stored,
so it is timed as (speculate + walk) - speculate.  The step count follows the time of a call: the first call is the
warm-up; a call of more than 5 s is timed once, by that first call.  --lib loads another build of the library (the segment
is compile-time: -DLZ_SW_SEGMENT=...).

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


def timed_to_fit(fn):
    """median ms of fn and the timed steps: the first call is the warm-up and sets the number of steps; a call of more than
    5 s is its own measurement"""
    first = timed(fn, 1, 0)[0]
    if first > 5000:
        return first, 1
    steps = 3 if first > 500 else 7
    return statistics.median(timed(fn, steps, 0)), steps


def wide_rows(source, win, dev):
    """one stream of win.numel() bytes on both paths -> (lines, dict of medians in ms, everything equal)"""
    n = int(win.numel())
    name = f"{source} 1 x {n >> 10} KiB"
    params = lz77.SlidingParams()
    seq_cap = lz77.sliding_seq_cap(n, params.min_match_length)
    win_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(lz77.sliding_scratch_bytes(n, 1), dtype=torch.uint8, device=dev)
    wscratch = torch.empty(lz77.sliding_wide_scratch_bytes(n), dtype=torch.uint8, device=dev)
    one = lz77.sliding_parse_batch(win, win_off, zero, params, seq_cap, scratch=scratch, phases=lib.LZ77_INDEX)
    wide = lz77.sliding_parse_wide(win, 0, params, seq_cap=seq_cap, scratch=wscratch)
    med, steps = {}, {}

    def wide_phase(mask):
        return lambda: lz77.sliding_parse_wide(win, 0, params, scratch=wscratch, out=wide, phases=mask)

    med["one-wave parse"], steps["one-wave parse"] = timed_to_fit(
        lambda: lz77.sliding_parse_batch(win, win_off, zero, params, scratch=scratch, out=one, phases=lib.LZ77_PARSE))
    for what, mask in (("wide index", lib.LZ77_SLIDING_WIDE_INDEX), ("wide speculate", lib.LZ77_SLIDING_WIDE_SPECULATE),
                       ("wide speculate+walk", lib.LZ77_SLIDING_WIDE_SPECULATE | lib.LZ77_SLIDING_WIDE_WALK),
                       ("wide emit", lib.LZ77_SLIDING_WIDE_EMIT)):
        med[what], steps[what] = timed_to_fit(wide_phase(mask))
    n_seq, n_lit = int(one.n_seq[0]), int(one.n_lit[0])
    same = bool(int(wide.n_seq[0]) == n_seq and int(wide.n_lit[0]) == n_lit and int(one.status[0]) == 0 and
                int(wide.status[0]) == 0 and torch.equal(wide.literal_count[0, :n_seq], one.literal_count[0, :n_seq]) and
                torch.equal(wide.match_length[0, :n_seq], one.match_length[0, :n_seq]) and
                torch.equal(wide.match_offset[0, :n_seq], one.match_offset[0, :n_seq]) and
                torch.equal(wide.literals[:n_lit], one.literals[:n_lit]))
    out_one, out_wide = torch.zeros_like(win), torch.zeros_like(win)
    rscratch = torch.empty(lz77.wide_replay_scratch_bytes(n_seq, n), dtype=torch.uint8, device=dev)
    replays = (("one-wave replay", lambda: lz77.sliding_replay_batch(out_one, win_off, zero, one.literal_count, one.match_length,
                                                                     one.match_offset, one.n_seq, one.literals, one.lit_off,
                                                                     one.n_lit, params.window_size)),
               ("wide replay", lambda: lz77.sliding_replay_wide(out_wide, 0, wide.literal_count, wide.match_length,
                                                                wide.match_offset, n_seq, wide.literals, n_lit,
                                                                params.window_size, scratch=rscratch)))
    for what, fn in replays:
        med[what], steps[what] = timed_to_fit(fn)
    torch.cuda.synchronize()
    back = bool(torch.equal(out_one, win) and torch.equal(out_wide, win))
    med["wide walk"] = max(med["wide speculate+walk"] - med["wide speculate"], 0.0)
    med["wide parse"] = med["wide speculate+walk"] + med["wide emit"]
    lines = [f"{name:26s} {what:20s}: median {med[what]:12.3f} ms over {steps[what]} steps  "
             f"{n / med[what] / 1e6:9.4f} GB/s of input" for what in steps]
    lines.append(f"{name:26s} {n_seq} sequences, {n_lit} literals; wide parse = speculate + walk + emit = "
                 f"{med['wide parse']:.3f} ms, the walk {100 * med['wide walk'] / med['wide parse']:.1f} % of it "
                 f"({med['wide walk']:.3f} ms); one-wave / wide: parse {med['one-wave parse'] / med['wide parse']:.2f}x, replay "
                 f"{med['one-wave replay'] / med['wide replay']:.2f}x; same sequences and literals on both paths: "
                 f"{'yes' if same else 'NO'}; both round trips: {'ok' if back else 'FAILED'}")
    print("\n".join(lines), flush=True)
    return lines, med, same and back


def run_wide(sizes_kib, wanted, dev):
    top = max(sizes_kib) << 10
    segment, cap = lz77.sliding_wide_shape()
    lines = [f"lz77 sliding wide bench: ONE stream, one-wave kernels vs wide kernels in the same run; the reference's default "
             f"parameters, segment {segment}, cap {cap}, threshold {lz77.sliding_wide_threshold()} bytes, HIP events, "
             f"{torch.cuda.get_device_name(0)}", f"kernels: {', '.join(lz77.sliding_wide_kernel_names())}"]
    print("\n".join(lines), flush=True)
    make = {"markov": lambda: bench_data.markov1_chunks_device(16, max(top >> 16, 1), min(top, 1 << 16), 77, dev).reshape(-1),
            "all-equal": lambda: torch.full((top,), 7, dtype=torch.uint8, device=dev),
            "random": lambda: torch.randint(0, 256, (top,), dtype=torch.uint8, device=dev,
                                            generator=torch.Generator(device=dev).manual_seed(78))}
    ratios, all_ok = {}, True
    for source in wanted:
        data = make[source]()
        for kib in sizes_kib:
            rows, med, ok = wide_rows(source, data[: kib << 10].contiguous(), dev)
            lines += rows
            all_ok = all_ok and ok
            ratios[(source, kib)] = (med["one-wave parse"] / med["wide parse"], med["one-wave replay"] / med["wide replay"])
    kib = max(sizes_kib)
    if "markov" in wanted:
        p, r = ratios[("markov", kib)]
        lines.append(f"gate at {kib} KiB on the Markov source: wide parse {p:.1f}x, wide replay {r:.1f}x the one-wave path "
                     f"(10x each is asked): {'met' if p >= 10 and r >= 10 else 'MISSED'}")
    for what, i in (("parse", 0), ("replay", 1)):
        ok = [k for k in sizes_kib if all(ratios[(s, j)][i] > 1 for s in wanted for j in sizes_kib if j >= k)]
        lines.append(f"wide {what} is faster on {', '.join(wanted)} from {min(ok)} KiB on" if ok else
                     f"wide {what} is not faster at the largest measured size on every source")
    print("\n".join(lines[-3:]), flush=True)
    return lines, all_ok


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
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--wide-kib", default="64,256,1024,4096,16384")
    ap.add_argument("--wide-sources", default="markov,all-equal,random")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        lib._lib = lib.load(args.lib)
    lib.require_device()
    dev = torch.device("cuda:0")
    if args.wide:
        lines, ok = run_wide([int(k) for k in args.wide_kib.split(",")], args.wide_sources.split(","), dev)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0 if ok else 1
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
