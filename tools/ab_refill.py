"""Same-box alternation of several builds of libscl_hip.so in ONE process (the form of tools/try_striped_rt.py):

    python tools/ab_refill.py parent.so parent_copy.so result.so [--rounds 7] [--reps 25]

Every library given is loaded side by side (give the parent twice, as two FILES, for the A/A margin) and gets its own model
objects; the batches, the slots and the output buffers are shared.  Per case and round every library runs `reps` round trips
(encode, decode -- HIP events around each) and `reps` decodes behind a decode; the rounds alternate between the libraries.
Every library's first round trip is verified against the input.  Printed per case and library: the median over the rounds of
the per-round means, the spread (max - min over the rounds), and per round the result-against-first-library differences.

Cases: the headline batch (rANS, t256, 262 144 x 4096, striped), the same on tANS, configs[1] (65 536 chunks, linear slots),
configs[2] (range coder, uniform bytes, striped), the headline on linear slots; and, on linear slots, what else runs on the
frame of scl_ans_frame.h: rANS NUM_BITS_OUT = 8 (b8) and = 2 (b2, scl_rans_fast_b.hip), the tANS table kernels (tanstab:
SCL_TANS_KERNELS=table for the case), rANS on a table of total 86 (t86) -- each also as a 65 536-chunk batch (*_64k), which
runs the 256-lane forms."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stanford_compression_library_amd import bench_data  # noqa: E402
from stanford_compression_library_amd.backend import lib as _lib  # noqa: E402
from stanford_compression_library_amd.backend import models  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--cases", default="headline,tans,configs1,configs2,linear")
args = ap.parse_args()
dev = torch.device("cuda:0")
handles = [_lib.load(os.path.abspath(p)) for p in args.libs]


def with_lib(i, make):
    """models bind the library that is current when they are created"""
    _lib._lib = handles[i]
    try:
        return make()
    finally:
        _lib._lib = handles[0]


t256 = bench_data.t256_table()
ones = np.ones(256, dtype=np.int64)
CASES = {
    "headline": ("rANS t256 262144 x 4096 striped", lambda: models.RansModel(t256.tolist(), 1 << 16, 1, 32), t256, 262144, "striped"),
    "tans": ("tANS t256 262144 x 4096 striped", lambda: models.TansModel(t256.tolist(), 1, 32), t256, 262144, "striped"),
    "configs1": ("configs[1]: rANS t256 65536 x 4096 linear", lambda: models.RansModel(t256.tolist(), 1 << 16, 1, 32), t256, 65536, "linear"),
    "configs2": ("configs[2]: range coder, uniform bytes, 262144 x 4096 striped", lambda: models.RangeModel(ones.tolist(), 32, 32), ones, 262144,
                 "striped"),
    "linear": ("rANS t256 262144 x 4096 linear", lambda: models.RansModel(t256.tolist(), 1 << 16, 1, 32), t256, 262144, "linear"),
}
t86 = np.array([3, 1, 7, 2, 19, 40, 5, 9], dtype=np.int64)
for tag, n in (("", 262144), ("_64k", 65536)):
    CASES["b8" + tag] = (f"rANS b=8 RF=2^8 t256 {n} x 4096 linear", lambda: models.RansModel(t256.tolist(), 1 << 8, 8, 32), t256, n, "linear")
    CASES["b2" + tag] = (f"rANS b=2 RF=2^8 t256 {n} x 4096 linear", lambda: models.RansModel(t256.tolist(), 1 << 8, 2, 32), t256, n, "linear")
    CASES["tanstab" + tag] = (f"tANS table kernels RF=1 t256 {n} x 4096 linear", lambda: models.TansModel(t256.tolist(), 1, 32), t256, n, "linear",
                              {"SCL_TANS_KERNELS": "table"})
    CASES["t86" + tag] = (f"rANS total 86 {n} x 4096 linear", lambda: models.RansModel(t86.tolist(), 1 << 16, 1, 32), t86, n, "linear")
chunk_len = 4096


def time_case(model, sym, enc, dec, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for i in range(reps):
        model.encode_batch(sym, out=enc)
        ev[2 * i + 1].record()
        model.decode_encoded(enc, chunk_len, out=dec)
        ev[2 * i + 2].record()
    dd = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    model.decode_encoded(enc, chunk_len, out=dec)
    dd[0].record()
    for i in range(reps):
        model.decode_encoded(enc, chunk_len, out=dec)
        dd[i + 1].record()
    torch.cuda.synchronize()
    te = np.mean([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps)])
    td = np.mean([ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(reps)])
    tdd = np.mean([dd[i].elapsed_time(dd[i + 1]) for i in range(reps)])
    return te, td, te + td, tdd


for key in args.cases.split(","):
    title, make, freq, n_chunks, layout = CASES[key][:5]
    env = CASES[key][5] if len(CASES[key]) > 5 else {}
    os.environ.update(env)  # read by the library at every call
    ms = [with_lib(i, make) for i in range(len(handles))]
    sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=1, device=dev)
    enc = ms[0].alloc_encoded(n_chunks, chunk_len, dev, layout=layout)
    dec = ms[0].alloc_decoded(n_chunks, chunk_len, dev)
    print(f"== {title}" + (f"   kernels: {ms[0].kernel_names(n_chunks, layout)}" if key != "configs2" else ""))
    for i, m in enumerate(ms):
        m.encode_batch(sym, out=enc)
        out = m.decode_encoded(enc, chunk_len, out=dec)
        torch.cuda.synchronize()
        assert int(out[3].abs().sum()) == 0 and torch.equal(out[0], sym) and torch.equal(out[2], enc.nbits), args.libs[i]
    for _ in range(3):
        for m in ms:
            time_case(m, sym, enc, dec, args.reps)
    res = [[] for _ in ms]
    for rnd in range(args.rounds):
        for j in range(len(ms)):  # the order rotates from round to round: no library always runs behind the same one
            i = (j + rnd) % len(ms)
            res[i].append(time_case(ms[i], sym, enc, dec, args.reps))
    res = np.array(res)  # [lib][round][enc, dec, rt, dec behind dec]
    names = ("encode", "decode", "round trip", "decode behind decode")
    for i, p in enumerate(args.libs):
        med, lo, hi = np.median(res[i], axis=0), res[i].min(axis=0), res[i].max(axis=0)
        print(f"  {os.path.basename(p):28s} " + "  ".join(f"{n} {m:.4f} ({a:.4f} .. {b:.4f}, spread {b - a:.4f})"
                                                            for n, m, a, b in zip(names, med, lo, hi)) + " ms")
    for i in range(1, len(ms)):
        d = res[i] - res[0]
        for k, n in enumerate(names):
            print(f"  {os.path.basename(args.libs[i])} - {os.path.basename(args.libs[0])}, {n}, per round: "
                  + " ".join(f"{x:+.4f}" for x in d[:, k]) + f"   median {np.median(d[:, k]):+.4f} ms ({100 * np.median(d[:, k]) / np.median(res[0][:, k]):+.2f} %)")
    for k in env:
        del os.environ[k]
    del sym, enc, dec, ms
    torch.cuda.empty_cache()
