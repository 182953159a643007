"""Times the paths that run on the scans of csrc/scl_scan.h, on the tree given as argv[1] (its library, its tools), so that two
builds can be compared by alternating processes on one GPU: profiles/scan_refactor_timing.txt.

    python tools/time_scan_paths.py TREE

  1. compaction: TREE/tools/time_compact.py as it is (dense and framed on the headline batch, mean of 5);
  2. the LZ77 one-wave kernels: run_shape of TREE/tools/bench_lz77.py on 1024 streams of 64 KiB (index = 8 passes);
  3. the wide LZ77 path: emit and replay of one Markov stream of 1 MiB and of 16 MiB, 15 steps after 3 (HIP events);
  4. the prefix block: part (a) of TREE/tools/bench_prefix_block.py at 256 MiB, 20 steps after 5.
"""
import os
import runpy
import statistics
import sys

root = os.path.abspath(sys.argv[1])
sys.path[0:0] = [root, os.path.join(root, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stanford_compression_library_amd import bench_data  # noqa: E402
from stanford_compression_library_amd.backend import lib, lz77, models  # noqa: E402

print("library:", lib.LIB_PATH, flush=True)
assert os.path.abspath(lib.LIB_PATH).startswith(root + os.sep), lib.LIB_PATH
lib.require_device()
dev = torch.device("cuda:0")

# 1. compaction: the tool as it is
runpy.run_path(os.path.join(root, "tools", "time_compact.py"), run_name="__main__")
sys.stdout.flush()

# 2. LZ77 one-wave kernels: the tool's run_shape on 1024 x 64 KiB (index = 8 passes)
import bench_lz77  # noqa: E402

win = bench_data.markov1_chunks_device(16, 1024, 65536, 77, dev).reshape(-1)
for ln in bench_lz77.run_shape("1024 x 64 KiB", win, 1024, 65536, 10, 3, dev, host_streams=0):
    print(ln, flush=True)

# 3. wide path: emit and replay, the tool's timed_to_fit, Markov source at 1 MiB and 16 MiB
L, M = bench_lz77.L, bench_lz77.M
for kib in (1024, 16384):
    w = win[: kib << 10].contiguous()
    n = int(w.numel())
    seq_cap = lz77.default_seq_cap(n, L)
    wscratch = torch.empty(lz77.wide_scratch_bytes(n), dtype=torch.uint8, device=dev)
    wide = lz77.parse_wide(w, 0, L, M, seq_cap=seq_cap, scratch=wscratch)
    torch.cuda.synchronize()
    n_seq, n_lit = int(wide.n_seq[0]), int(wide.n_lit[0])
    out = torch.zeros_like(w)
    rscratch = torch.empty(lz77.wide_replay_scratch_bytes(n_seq, n), dtype=torch.uint8, device=dev)
    calls = (("wide emit", lambda: lz77.parse_wide(w, 0, L, M, scratch=wscratch, out=wide, phases=lib.LZ77_WIDE_EMIT)),
             ("wide replay", lambda: lz77.replay_wide(out, 0, wide.literal_count, wide.match_length, wide.match_offset, n_seq,
                                                      wide.literals, n_lit, scratch=rscratch)))
    for what, fn in calls:
        ms = bench_lz77.timed(fn, 15, 3)
        print(f"markov 1 x {kib} KiB {what:12s}: median {statistics.median(ms):9.4f} ms  min {min(ms):9.4f}  max {max(ms):9.4f}",
              flush=True)
    torch.cuda.synchronize()
    print(f"markov 1 x {kib} KiB {n_seq} sequences, round trip {'ok' if torch.equal(out, w) else 'FAILED'}", flush=True)
    del wscratch, rscratch, out, wide
del win

# 4. prefix block: part (a) of tools/bench_prefix_block.py at 256 MiB
from bench_prefix import timed  # noqa: E402
from stanford_compression_library_amd.compressors import HuffmanTree  # noqa: E402
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist  # noqa: E402

freq = bench_data.t256_table()
n = 256 << 20
sym = bench_data.iid_chunks_device(freq, n // 4096, 4096, 1, dev).reshape(-1)
hist = torch.bincount(sym[:16 << 20].to(torch.int64), minlength=256).cpu().numpy().astype(np.float64)
probs = np.maximum(hist, 1.0)
probs /= probs.sum()
table = HuffmanTree(ProbabilityDist({i: float(p) for i, p in enumerate(probs)})).get_encoding_table()
lengths = np.array([len(table[i]) for i in range(256)], np.uint8)
codes = np.array([int(table[i].to01(), 2) for i in range(256)], np.uint32)
model = models.PrefixModel(codes, lengths)
outb = torch.empty(model.slot_bytes(n), dtype=torch.uint8, device=dev)
nbits, status = (int(v) for v in model.encode_block_into(sym, outb).cpu())
dec = torch.empty(n, dtype=torch.uint8, device=dev)
e_ms = timed(lambda: model.encode_block_into(sym, outb), 20, 5)
d_ms = timed(lambda: model.decode_block_device(outb, nbits, out_cap=n, out=dec), 20, 5)
_, n_out, used, dstatus, passes = model.decode_block_device(outb, nbits, out_cap=n, out=dec)
ok = status == 0 and dstatus == 0 and n_out == n and used == nbits and torch.equal(dec, sym)
for what, ms in (("encode", e_ms), ("decode", d_ms)):
    print(f"prefix block 256 MiB {what}: median {statistics.median(ms):9.4f} ms  min {min(ms):9.4f}  max {max(ms):9.4f}",
          flush=True)
print(f"prefix block 256 MiB sync_passes {passes}, round trip {'ok' if ok else 'FAILED'}", flush=True)
