"""Per-wave lifetimes of the two headline kernels (rANS, t256, 262 144 x 4096, striped slots): do the four waves of a SIMD
advance together?

    python tools/wave_lifetimes.py --build OUT.so [-DSCL_WAVE_PRIO_ENC=1 ...]   build a tracing copy of the library
    python tools/wave_lifetimes.py --lib OUT.so [--launches 3] [--layout striped]  run it (MI355X)

--build compiles csrc/scl_rans_fast.hip once more with -DSCL_WAVE_TRACE (and whatever -D options follow) and links it with
the other objects of the normal build (csrc/_build, so `make -C stanford_compression_library_amd/csrc` comes first).  Without
--trace-off the copy records; with it only the -D options apply (the candidates of profiles/wave_progress_timing.txt).
Under the macro lane 0 of every wave of rans_encode_fast_kernel / rans_decode_fast_kernel writes {HW_ID | XCC_ID << 32,
s_memtime behind the table staging, s_memtime at the end, wave number + 1} to the buffer that this tool hands over through
scl_wave_trace_set (a __device__ pointer of that file); the normal build has none of it and the same device code as before.

Printed per kernel: how many waves each SIMD held; whether the slot order is the start order; per start-order rank and per
slot the median lifetime, start and end as fractions of the SIMD's span (first start to last end); the distribution over
the SIMDs of shortest lifetime / longest lifetime, of the tail (last end - first end) / span and of the span in ticks.  Only
stamps of one SIMD are ever subtracted from each other: the counters of different CUs do not agree (they read tens of millions
of ticks apart inside one launch), so there is no "fraction of the launch" across the chip; the span of a SIMD stands for it."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford_compression_library_amd", "csrc")


def build(out, defines, trace):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.abspath(out) + ".scl_rans_fast.o"
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
    subprocess.check_call([hipcc] + flags + (["-DSCL_WAVE_TRACE"] if trace else []) + defines +
                          ["-c", os.path.join(CSRC, "scl_rans_fast.hip"), "-o", obj])
    others = sorted(os.path.join(CSRC, "_build", f) for f in os.listdir(os.path.join(CSRC, "_build"))
                    if f.endswith(".o") and f != "scl_rans_fast.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj] + others + ["-ldl"])
    os.remove(obj)


def fields(hw):
    """HW_ID of gfx9: wave_id [3:0], simd_id [5:4], cu_id [11:8], sh_id [12], se_id [15:13]; XCC_ID in bits 32.."""
    return {"slot": hw & 15, "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7,
            "xcc": (hw >> 32) & 15}


def report(name, rec, np):
    rec = rec[rec[:, 3] != 0]
    f = fields(rec[:, 0])
    t0, t1 = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    cu_key = ((f["xcc"] * 8 + f["se"]) * 2 + f["sh"]) * 16 + f["cu"]
    simd_key = cu_key * 4 + f["simd"]
    print(f"== {name}: {len(rec)} waves recorded on {len(np.unique(cu_key))} CUs, {len(np.unique(simd_key))} SIMDs, "
          f"{len(np.unique(f['xcc']))} XCDs; slots seen: {sorted(int(s) for s in np.unique(f['slot']))}")
    order = np.argsort(simd_key, kind="stable")
    groups = np.split(order, np.unique(simd_key[order], return_index=True)[1][1:])
    sizes = np.bincount([len(g) for g in groups])
    print("   waves per SIMD: " + ", ".join(f"{n} on {c}" for n, c in enumerate(sizes) if c))
    full = [g for g in groups if len(g) == 4]
    if not full:
        print("   no SIMD with four waves: nothing to arbitrate")
        return
    by_rank = np.zeros((len(full), 4, 3))   # start-order rank -> lifetime, start, end (fractions of the SIMD's span)
    by_slot = [[] for _ in range(16)]
    ratio, tail, spans, lives, slot_is_age = [], [], [], [], 0
    for k, g in enumerate(full):
        g = g[np.argsort(t0[g], kind="stable")]
        a, b = t0[g].min(), t1[g].max()
        span = float(b - a)
        life = (t1[g] - t0[g]) / span
        by_rank[k, :, 0], by_rank[k, :, 1], by_rank[k, :, 2] = life, (t0[g] - a) / span, (t1[g] - a) / span
        for j, w in enumerate(g):
            by_slot[int(f["slot"][w])].append((life[j], (t0[w] - a) / span, (t1[w] - a) / span))
        slot_is_age += int(np.all(np.diff(f["slot"][g]) > 0))
        ratio.append(life.min() / life.max())
        tail.append((t1[g].max() - t1[g].min()) / span)
        spans.append(span)
        lives.append(np.sort(t1[g] - t0[g]))
    print(f"   SIMDs with four waves: {len(full)}; slot order = start order on {slot_is_age} of them")
    med = np.median(by_rank, axis=0)
    print("   by start order (0 = oldest), medians over the SIMDs, fractions of the SIMD's span:")
    for j in range(4):
        print(f"     rank {j}: lifetime {med[j, 0]:.4f}  start {med[j, 1]:.4f}  end {med[j, 2]:.4f}")
    print("   by slot (HW_ID.wave_id):")
    for s, rows in enumerate(by_slot):
        if rows:
            m = np.median(np.array(rows), axis=0)
            print(f"     slot {s}: {len(rows):5d} waves  lifetime {m[0]:.4f}  start {m[1]:.4f}  end {m[2]:.4f}")
    pct = (5, 25, 50, 75, 95)
    print("   percentiles over the SIMDs                  " + "  ".join(f"p{p:<5d}" for p in pct))
    for label, v in (("shortest lifetime / longest lifetime", ratio), ("tail = (last end - first end) / span   ", tail)):
        print(f"     {label}  " + "  ".join(f"{x:.4f}" for x in np.percentile(v, pct)))
    print("     SIMD span, s_memtime ticks            " + "  ".join(f"{x:6.0f}" for x in np.percentile(spans, pct)))
    print("   the four lifetimes of a SIMD in ticks, shortest first (medians): "
          + "  ".join(f"{x:.0f}" for x in np.median(np.array(lives), axis=0))
          + f";  sum of the four / (4 x span) = {np.median(np.array(lives).sum(axis=1) / (4 * np.array(spans))):.4f}")


def run(args):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from stanford_compression_library_amd import bench_data
    from stanford_compression_library_amd.backend import lib as _lib
    from stanford_compression_library_amd.backend import models

    handle = _lib.load(os.path.abspath(args.lib))
    _lib._lib = handle  # models bind the library that is current when they are created
    setter = handle.scl_wave_trace_set  # AttributeError: the library was not built with -DSCL_WAVE_TRACE
    setter.restype, setter.argtypes = C.c_int, (C.c_void_p, C.c_uint)
    dev = torch.device("cuda:0")
    n_chunks, chunk_len = args.chunks, 4096
    t256 = bench_data.t256_table()
    model = models.RansModel(t256.tolist(), 1 << 16, 1, 32)
    sym = bench_data.iid_chunks_device(t256, n_chunks, chunk_len, seed=1, device=dev)
    enc = model.alloc_encoded(n_chunks, chunk_len, dev, layout=args.layout)
    dec = model.alloc_decoded(n_chunks, chunk_len, dev)
    print("kernels:", model.kernel_names(n_chunks, args.layout))
    n_waves = (n_chunks + 63) // 64
    buf = torch.zeros(4 * n_waves, dtype=torch.int64, device=dev)

    def trace(on):
        torch.cuda.synchronize()
        assert setter(buf.data_ptr() if on else None, n_waves if on else 0) == 0

    trace(False)
    for _ in range(10):
        model.encode_batch(sym, out=enc)
        out = model.decode_encoded(enc, chunk_len, out=dec)
    torch.cuda.synchronize()
    assert int(out[3].abs().sum()) == 0 and torch.equal(out[0], sym)
    for k in range(args.launches):
        for side in ("encode", "decode"):
            buf.zero_()
            trace(True)
            if side == "encode":
                model.encode_batch(sym, out=enc)
            else:
                model.decode_encoded(enc, chunk_len, out=dec)
            trace(False)
            report(f"{side}, traced launch {k + 1}", buf.cpu().numpy().reshape(-1, 4), np)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build")
    ap.add_argument("--trace-off", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=262144)
    ap.add_argument("--layout", default="striped")
    args, defines = ap.parse_known_args()
    if args.build:
        assert all(d.startswith("-D") for d in defines), defines
        build(args.build, defines, not args.trace_off)
    else:
        run(args)
