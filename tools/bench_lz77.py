"""Times the LZ77 device layer -- index, parse, replay -- on a batch of streams and on one large stream as a batch of one,
and on the batch the entropy stage (encode_batch / decode_batch) beside its yardstick: the host stage of the classes,
LZ77StreamsEncoder.encode_block / LZ77StreamsDecoder.decode_block, timed on --host-streams of the same parsed streams and
scaled to the batch.  Recorded, not gated: profiles/lz77_bench.txt.

    python tools/bench_lz77.py [--streams 4096] [--stream-kib 64] [--single-mib 16] [--steps 20] [--warmup 5]
                               [--single-steps N] [--single-warmup N] [--host-streams 64] [--out FILE]
    python tools/bench_lz77.py --wide [--wide-kib 64,256,1024,4096,16384] [--wide-stages lz,entropy] [--out FILE]

--wide times ONE stream on both paths in the same run -- the one-wave kernels (parse_batch / replay_batch of a batch of
one) and the wide ones (parse_wide phase by phase, replay_wide) -- on the Markov source and on all-equal bytes, checks
that both paths store the same sequences and literals and that the replay restores the input, and prints the ratios
scl_lz77_wide_threshold() and the 10x gate at the largest size are read from.  The step count follows the time of a call:
3 timed steps for a call of more than a second, up to 15 for short ones.  The entropy stage of the same stream follows
(--wide-stages picks either half): encode_batch / decode_batch of the one-stream batch beside encode_wide / decode_wide on
the same ParsedBatch -- HIP events for the encoders, the wall clock around the call for the decoders (decode_wide
synchronises) -- with the bits and the decoded rows compared at every size, a 10x gate of its own at the largest size, and
the stream size -- in coded values, 3 n_seq + n_lit: what the stage's work depends on -- from which both wide calls win on
both sources: scl_lz77_entropy_wide_threshold() is read from that line.

Data: the first-order Markov source of bench_data.py over 16 symbols, one chain per stream (generated on the device).  The
single stream is the first --single-mib MiB of the very same bytes, read as ONE window: its parse is one wavefront.
Kernel time only: HIP events around each call on the current stream, buffers and scratch allocated once.  Every shape is
verified: the replay of the parse's output must restore the input.  That round trip checks parse and replay, NOT the index:
the parse re-checks every entry it reads from order[], so a misplaced entry still gives a valid parse, only with other
matches.  The index is compared with its definition, and the parse with the restated rule, in tests/test_gpu_lz77_limits.py.
The entropy rows are verified the same way: the decoder's output, replayed, must restore the input; that the bits are the
reference's is the business of tests/test_gpu_lz77_entropy.py.
"""
import argparse
import os
import statistics
import sys
import time

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


def entropy_rows(name, win, win_off, res, n_streams, stream_len, steps, warmup, host_streams, dev):
    """the entropy stage on the parsed batch `res`, and the host classes on its first `host_streams` streams"""
    from stanford_compression_library_amd.compressors.lz77 import LZ77Sequence, LZ77StreamsDecoder, LZ77StreamsEncoder

    total = n_streams * stream_len
    enc = lz77.encode_batch(res)
    lit_cap = torch.full((n_streams,), stream_len, dtype=torch.int32, device=dev)
    dec = lz77.decode_batch(enc.bits, enc.bit_offset, enc.nbits, res.seq_cap, res.lit_off, lit_cap)
    rows = (("encode", lambda: lz77.encode_batch(res, out=enc)),
            ("decode", lambda: lz77.decode_batch(enc.bits, enc.bit_offset, enc.nbits, res.seq_cap, res.lit_off, lit_cap, out=dec)))
    lines = []
    for what, fn in rows:
        ms = timed(fn, steps, warmup)
        med = statistics.median(ms)
        lines.append(f"{name:22s} entropy {what}: median {med:10.3f} ms  min {min(ms):10.3f}  max {max(ms):10.3f}  "
                     f"{total / med / 1e6:8.3f} GB/s of input")
    out = torch.zeros_like(win)
    have = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    out_len, status = lz77.replay_batch(out, win_off, have, dec.literal_count, dec.match_length, dec.match_offset, dec.n_seq,
                                        dec.literals, dec.lit_off, dec.n_lit)
    torch.cuda.synchronize()
    ok = bool((enc.status == 0).all() and (dec.status == 0).all() and torch.equal(dec.consumed, enc.nbits) and
              (status == 0).all() and torch.equal(out, win))
    coded = int(enc.nbits.to(torch.int64).sum()) // 8
    lines.append(f"{name:22s} entropy stage: {coded} coded bytes ({total / max(coded, 1):.2f} : 1), slots of {enc.out_stride} "
                 f"bytes, kernels {', '.join(lz77.entropy_kernel_names())}, {steps} timed steps after {warmup}, "
                 f"encode -> decode -> replay {'ok' if ok else 'FAILED'}")
    # the yardstick: the host stage of the classes, stream by stream
    k = min(host_streams, n_streams)
    n_seq, n_lit = res.n_seq[:k].cpu().tolist(), res.n_lit[:k].cpu().tolist()
    fields = [t[:k].cpu().numpy().view("uint32") for t in (res.literal_count, res.match_length, res.match_offset)]
    lits, lit_off = res.literals.cpu().numpy(), res.lit_off[:k].cpu().tolist()
    t_enc = t_dec = 0.0
    same = True
    nbits = enc.nbits[:k].cpu().tolist()
    for s in range(k):
        seqs = [LZ77Sequence(*t) for t in zip(*(f[s, : n_seq[s]].tolist() for f in fields))]
        literals = lits[lit_off[s]: lit_off[s] + n_lit[s]].tolist()
        t0 = time.perf_counter()
        bits = LZ77StreamsEncoder().encode_block(seqs, literals)
        t1 = time.perf_counter()
        (got_seqs, got_lits), used = LZ77StreamsDecoder().decode_block(bits)
        t2 = time.perf_counter()
        t_enc += t1 - t0
        t_dec += t2 - t1
        same = same and len(bits) == nbits[s] and used == nbits[s] and got_seqs == seqs and got_lits == literals
    scale = n_streams / max(k, 1)
    lines.append(f"{name:22s} host stage of the classes on {k} streams: encode {t_enc:.3f} s, decode {t_dec:.3f} s; scaled to "
                 f"{n_streams} streams: encode {t_enc * scale * 1e3:.0f} ms, decode {t_dec * scale * 1e3:.0f} ms; "
                 f"same bit counts and values as the device stage: {'yes' if same else 'NO'}")
    return lines


def run_shape(name, win, n_streams, stream_len, steps, warmup, dev, host_streams=0):
    total = n_streams * stream_len
    win_off = torch.arange(n_streams + 1, dtype=torch.int64, device=dev) * stream_len
    start = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    seq_cap = lz77.default_seq_cap(stream_len, L)
    scratch = torch.empty(lz77.scratch_bytes(total, n_streams), dtype=torch.uint8, device=dev)
    res = lz77.parse_batch(win, win_off, start, L, M, seq_cap, scratch=scratch)
    out = torch.empty_like(win)
    have = torch.zeros(n_streams, dtype=torch.int32, device=dev)

    def replay():
        return lz77.replay_batch(out, win_off, have, res.literal_count, res.match_length, res.match_offset, res.n_seq,
                                 res.literals, res.lit_off, res.n_lit)

    phases = (("index", lambda: lz77.parse_batch(win, win_off, start, L, M, seq_cap, scratch=scratch, out=res,
                                                  phases=lib.LZ77_INDEX)),
              ("parse", lambda: lz77.parse_batch(win, win_off, start, L, M, seq_cap, scratch=scratch, out=res,
                                                  phases=lib.LZ77_PARSE)),
              ("replay", replay))
    lines = []
    for what, fn in phases:
        ms = timed(fn, steps, warmup)
        med = statistics.median(ms)
        lines.append(f"{name:22s} {what:6s}: median {med:10.3f} ms  min {min(ms):10.3f}  max {max(ms):10.3f}  "
                     f"{total / med / 1e6:8.3f} GB/s of input")
    out.fill_(0)
    out_len, status = replay()
    torch.cuda.synchronize()
    ok = bool((res.status == 0).all() and (status == 0).all() and (out_len == stream_len).all() and torch.equal(out, win))
    n_seq, n_lit = int(res.n_seq.to(torch.int64).sum()), int(res.n_lit.to(torch.int64).sum())
    lines.append(f"{name:22s} {n_seq} sequences, {n_lit} literals ({total / max(n_seq, 1):.1f} input bytes per sequence), "
                 f"{steps} timed steps after {warmup}, round trip {'ok' if ok else 'FAILED'}")
    if host_streams:
        lines += entropy_rows(name, win, win_off, res, n_streams, stream_len, steps, warmup, host_streams, dev)
    return lines


def timed_to_fit(fn):
    """median ms of fn: the first call is the warm-up and sets the number of timed steps"""
    first = timed(fn, 1, 0)[0]
    steps = 3 if first > 1000 else 7 if first > 50 else 15
    ms = timed(fn, steps, 1 if first <= 1000 else 0)
    return statistics.median(ms), steps


def timed_wall_to_fit(fn):
    """timed_to_fit by the wall clock around fn, the device idle before and after: for calls that synchronise"""
    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first = once()
    steps = 3 if first > 1000 else 7 if first > 50 else 15
    if first <= 1000:
        once()
    return statistics.median([once() for _ in range(steps)]), steps


def wide_entropy_rows(source, win, dev):
    """the entropy stage of one stream of win.numel() bytes on both paths -> (lines, dict of medians in ms)"""
    n = int(win.numel())
    name = f"{source} 1 x {n >> 10} KiB"
    parsed = lz77.parse_wide(win, 0, L, M)
    torch.cuda.synchronize()
    n_seq, n_lit = int(parsed.n_seq[0]), int(parsed.n_lit[0])
    stride = lz77.entropy_slot_bytes(n_seq, n_lit)
    one = lz77.encode_batch(parsed, out_stride=stride)
    scratch = torch.empty(lz77.entropy_wide_scratch_bytes(parsed.seq_cap, n, 8 * stride), dtype=torch.uint8, device=dev)
    wide = lz77.encode_wide(parsed, out_stride=stride, n_seq=n_seq, n_lit=n_lit, lit_off=0, scratch=scratch)
    torch.cuda.synchronize()
    nbits = int(one.nbits[0]) & 0xFFFFFFFF
    same_bits = bool(int(one.status[0]) == 0 and int(wide.status[0]) == 0 and int(wide.nbits64[0]) == nbits and
                     torch.equal(one.bits[: (nbits + 7) // 8], wide.bits[: (nbits + 7) // 8]))
    lit_cap = torch.full((1,), n, dtype=torch.int32, device=dev)
    dec_one = lz77.decode_batch(one.bits, one.bit_offset, one.nbits, parsed.seq_cap, parsed.lit_off, lit_cap)
    dec_wide = lz77.decode_wide(wide.bits, 0, nbits, parsed.seq_cap, n, scratch=scratch)
    calls = (("one-wave encode", timed_to_fit, lambda: lz77.encode_batch(parsed, out=one)),
             ("wide encode", timed_to_fit, lambda: lz77.encode_wide(parsed, n_seq=n_seq, n_lit=n_lit, lit_off=0, scratch=scratch,
                                                                    out=wide)),
             ("one-wave decode", timed_wall_to_fit, lambda: lz77.decode_batch(one.bits, one.bit_offset, one.nbits, parsed.seq_cap,
                                                                              parsed.lit_off, lit_cap, out=dec_one)),
             ("wide decode", timed_wall_to_fit, lambda: lz77.decode_wide(wide.bits, 0, nbits, parsed.seq_cap, n, scratch=scratch,
                                                                         out=dec_wide)))
    med, lines = {}, []
    for what, timer, fn in calls:
        med[what], steps = timer(fn)
        lines.append(f"{name:26s} {what:16s}: median {med[what]:10.3f} ms over {steps:2d} steps  "
                     f"{n / med[what] / 1e6:9.4f} GB/s of input")
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    same_rows = bool(int(dec_one.status[0]) == 0 and int(dec_wide.status[0]) == 0 and int(dec_wide.n_seq[0]) == n_seq and
                     int(dec_wide.n_lit[0]) == n_lit and int(dec_wide.consumed[0]) == nbits and
                     int(dec_one.consumed[0]) & 0xFFFFFFFF == nbits and
                     all(torch.equal(a[0, :n_seq], b[0, :n_seq]) and torch.equal(a[0, :n_seq], c[0, :n_seq])
                         for a, b, c in ((dec_wide.literal_count, dec_one.literal_count, parsed.literal_count),
                                         (dec_wide.match_length, dec_one.match_length, parsed.match_length),
                                         (dec_wide.match_offset, dec_one.match_offset, parsed.match_offset))) and
                     torch.equal(dec_wide.literals[:n_lit], dec_one.literals[:n_lit]) and
                     torch.equal(dec_wide.literals[:n_lit], parsed.literals[:n_lit]))
    lines.append(f"{name:26s} {n_seq} sequences, {n_lit} literals, {nbits} bits; one-wave / wide: encode "
                 f"{med['one-wave encode'] / med['wide encode']:.2f}x, decode {med['one-wave decode'] / med['wide decode']:.2f}x; "
                 f"sync_passes {int(dec_wide.sync_passes[0])}; identical bits: {'yes' if same_bits else 'NO'}, identical decoded "
                 f"rows and literals (both paths, and the parse's): {'yes' if same_rows else 'NO'}")
    print(lines[-1], flush=True)
    med["values"] = 3 * n_seq + n_lit
    return lines, med


def run_wide_entropy(sizes_kib, sources, dev):
    lines = [f"lz77 wide entropy bench: ONE stream, scl_lz77_entropy_*_batch on a batch of one vs scl_lz77_entropy_*_wide in the "
             f"same run; binned_offset {lz77.DEFAULT_BINNED_OFFSET}, threshold {lz77.entropy_wide_threshold()} coded values; encoders: "
             f"HIP events, decoders: wall clock around the call", f"kernels: {', '.join(lz77.entropy_kernel_names())} vs "
             f"{', '.join(lz77.entropy_wide_kernel_names())}"]
    print("\n".join(lines), flush=True)
    ratios, values = {}, {}
    for source, data in sources:
        for kib in sizes_kib:
            rows, med = wide_entropy_rows(source, data[: kib << 10].contiguous(), dev)
            lines += rows
            ratios[(source, kib)] = (med["one-wave encode"] / med["wide encode"], med["one-wave decode"] / med["wide decode"])
            values[(source, kib)] = med["values"]
    kib = max(sizes_kib)
    e, d = ratios[("markov", kib)]
    lines.append(f"entropy gate at {kib} KiB on the Markov source: wide encode {e:.1f}x, wide decode {d:.1f}x the one-wave kernels "
                 f"(10x each is asked): {'met' if e >= 10 and d >= 10 else 'MISSED'}")
    # by the size of the STREAM, 3 n_seq + n_lit coded values: the block's bytes do not say how much there is to code
    ok = [v for v in values.values() if all(min(ratios[k]) > 1 for k in ratios if values[k] >= v)]
    lost = [values[k] for k in ratios if min(ratios[k]) <= 1]
    lines.append((f"both wide entropy calls are faster on every measured stream of at least {min(ok)} coded values (3 n_seq + "
                  f"n_lit)" if ok else "the wide entropy calls are not both faster on the largest measured stream") +
                 (f"; the largest measured stream on which one of them loses has {max(lost)}" if lost else "; none loses"))
    print("\n".join(lines[-2:]), flush=True)
    return lines


def wide_shape_rows(source, win, dev):
    """one stream of win.numel() bytes on both paths -> (lines, dict of medians in ms)"""
    n = int(win.numel())
    name = f"{source} 1 x {n >> 10} KiB"
    win_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    seq_cap = lz77.default_seq_cap(n, L)
    scratch = torch.empty(lz77.scratch_bytes(n, 1), dtype=torch.uint8, device=dev)
    one = lz77.parse_batch(win, win_off, zero, L, M, seq_cap, scratch=scratch)
    wscratch = torch.empty(lz77.wide_scratch_bytes(n), dtype=torch.uint8, device=dev)
    wide = lz77.parse_wide(win, 0, L, M, seq_cap=seq_cap, scratch=wscratch)
    torch.cuda.synchronize()
    n_seq, n_lit = int(one.n_seq[0]), int(one.n_lit[0])
    same = bool(int(wide.n_seq[0]) == n_seq and int(wide.n_lit[0]) == n_lit and int(one.status[0]) == 0 and
                int(wide.status[0]) == 0 and torch.equal(wide.literal_count[0, :n_seq], one.literal_count[0, :n_seq]) and
                torch.equal(wide.match_length[0, :n_seq], one.match_length[0, :n_seq]) and
                torch.equal(wide.match_offset[0, :n_seq], one.match_offset[0, :n_seq]) and
                torch.equal(wide.literals[:n_lit], one.literals[:n_lit]))
    out_one, out_wide = torch.zeros_like(win), torch.zeros_like(win)
    rscratch = torch.empty(lz77.wide_replay_scratch_bytes(n_seq, n), dtype=torch.uint8, device=dev)

    def parse_phase(mask):
        return lambda: lz77.parse_wide(win, 0, L, M, scratch=wscratch, out=wide, phases=mask)

    calls = (("one-wave index", lambda: lz77.parse_batch(win, win_off, zero, L, M, seq_cap, scratch=scratch, out=one,
                                                         phases=lib.LZ77_INDEX)),
             ("one-wave parse", lambda: lz77.parse_batch(win, win_off, zero, L, M, seq_cap, scratch=scratch, out=one,
                                                         phases=lib.LZ77_PARSE)),
             ("one-wave replay", lambda: lz77.replay_batch(out_one, win_off, zero, one.literal_count, one.match_length,
                                                           one.match_offset, one.n_seq, one.literals, one.lit_off, one.n_lit)),
             ("wide index", parse_phase(lib.LZ77_WIDE_INDEX)), ("wide score", parse_phase(lib.LZ77_WIDE_SCORE)),
             ("wide walk", parse_phase(lib.LZ77_WIDE_WALK)), ("wide emit", parse_phase(lib.LZ77_WIDE_EMIT)),
             ("wide replay", lambda: lz77.replay_wide(out_wide, 0, wide.literal_count, wide.match_length, wide.match_offset,
                                                      n_seq, wide.literals, n_lit, scratch=rscratch)))
    med, lines = {}, []
    for what, fn in calls:
        med[what], steps = timed_to_fit(fn)
        lines.append(f"{name:26s} {what:16s}: median {med[what]:10.3f} ms over {steps:2d} steps  "
                     f"{n / med[what] / 1e6:9.4f} GB/s of input")
        print(lines[-1], flush=True)
    torch.cuda.synchronize()
    back = bool(torch.equal(out_one, win) and torch.equal(out_wide, win))
    med["wide parse"] = med["wide score"] + med["wide walk"] + med["wide emit"]
    lines.append(f"{name:26s} {n_seq} sequences, {n_lit} literals; wide parse = score + walk + emit = "
                 f"{med['wide parse']:.3f} ms, the walk {100 * med['wide walk'] / med['wide parse']:.1f} % of it; one-wave / wide: "
                 f"parse {med['one-wave parse'] / med['wide parse']:.2f}x, replay "
                 f"{med['one-wave replay'] / med['wide replay']:.2f}x; same sequences and literals on both paths: "
                 f"{'yes' if same else 'NO'}, round trip on both: {'ok' if back else 'FAILED'}")
    print(lines[-1], flush=True)
    return lines, med


def run_wide(sizes_kib, dev, stages=("lz", "entropy")):
    top = max(sizes_kib) << 10
    markov = bench_data.markov1_chunks_device(16, max(top >> 16, 1), min(top, 1 << 16), 77, dev).reshape(-1)
    sources = (("markov", markov), ("all-equal", torch.full((top,), 7, dtype=torch.uint8, device=dev)))
    lines = []
    if "lz" in stages:
        lines += run_wide_lz(sizes_kib, sources, dev)
    if "entropy" in stages:
        lines += run_wide_entropy(sizes_kib, sources, dev)
    return lines


def run_wide_lz(sizes_kib, sources, dev):
    tile, cap = lz77.wide_shape()
    lines = [f"lz77 wide bench: ONE stream, one-wave kernels vs wide kernels in the same run; min_match_length {L}, "
             f"max_num_matches_considered {M}, tile {tile}, cap {cap}, threshold {lz77.wide_threshold()} bytes, HIP events, "
             f"{torch.cuda.get_device_name(0)}", f"kernels: {', '.join(lz77.wide_kernel_names())}"]
    print("\n".join(lines), flush=True)
    ratios = {}
    for source, data in sources:
        for kib in sizes_kib:
            rows, med = wide_shape_rows(source, data[: kib << 10].contiguous(), dev)
            lines += rows
            ratios[(source, kib)] = (med["one-wave parse"] / med["wide parse"], med["one-wave replay"] / med["wide replay"])
    kib = max(sizes_kib)
    p, r = ratios[("markov", kib)]
    lines.append(f"gate at {kib} KiB on the Markov source: wide parse {p:.1f}x, wide replay {r:.1f}x the one-wave path "
                 f"(10x each is asked): {'met' if p >= 10 and r >= 10 else 'MISSED'}")
    for what, i in (("parse", 0), ("replay", 1)):
        ok = [k for k in sizes_kib if all(ratios[(s, j)][i] > 1 for s, _ in sources for j in sizes_kib if j >= k)]
        lines.append(f"wide {what} is faster on both sources from {min(ok)} KiB on" if ok else
                     f"wide {what} is not faster on both sources at the largest size")
    print("\n".join(lines[-3:]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-kib", type=int, default=64)
    ap.add_argument("--single-mib", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--single-steps", type=int, default=None)
    ap.add_argument("--single-warmup", type=int, default=None)
    ap.add_argument("--host-streams", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--wide-kib", default="64,256,1024,4096,16384")
    ap.add_argument("--wide-stages", default="lz,entropy")
    args = ap.parse_args()
    lib.require_device()
    dev = torch.device("cuda:0")
    if args.wide:
        text = "\n".join(run_wide([int(k) for k in args.wide_kib.split(",")], dev, tuple(args.wide_stages.split(","))))
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    stream_len = args.stream_kib << 10
    single_len = args.single_mib << 20
    assert single_len <= args.streams * stream_len
    win = bench_data.markov1_chunks_device(16, args.streams, stream_len, 77, dev).reshape(-1)
    lines = [f"lz77 bench: min_match_length {L}, max_num_matches_considered {M}, first-order Markov source over 16 symbols, "
             f"HIP events, {torch.cuda.get_device_name(0)}", f"kernels: {', '.join(lz77.kernel_names())}"]
    print("\n".join(lines), flush=True)
    lines += run_shape(f"{args.streams} x {args.stream_kib} KiB", win, args.streams, stream_len, args.steps, args.warmup, dev,
                       host_streams=args.host_streams)
    print("\n".join(lines[2:]), flush=True)
    n_batch = len(lines)
    lines += run_shape(f"1 x {args.single_mib} MiB", win[:single_len].contiguous(), 1, single_len,
                       args.steps if args.single_steps is None else args.single_steps,
                       args.warmup if args.single_warmup is None else args.single_warmup, dev)
    print("\n".join(lines[n_batch:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
