"""The LZ layer of LZ77 on the device (csrc/scl_lz77.hip): match index + greedy parse, and sequence replay.

Two call shapes, as in :mod:`.models`:

* ``parse_host`` / ``replay_host`` -- one stream in host memory (what ``LZ77Encoder`` / ``LZ77Decoder`` use);
* ``parse_batch`` / ``replay_batch`` -- many independent streams resident in HBM, given as torch tensors.

A batch is ``n_streams`` windows laid out one after another in one uint8 tensor; ``win_off`` (int64, ``n_streams + 1``
entries) says where each starts.  uint32 / uint64 arrays of the C ABI travel as int32 / int64 tensors (the bit patterns).
Everything raises ``SclHipError`` when the library or a device is missing: no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import lib as _lib

MAX_MIN_MATCH_LENGTH = 8  # an L-gram is one 64-bit key in the index


def default_seq_cap(block_len: int, min_match_length: int) -> int:
    """sequences a block can produce at most: every match covers at least ``min_match_length`` bytes"""
    return max(int(block_len) // max(int(min_match_length), 1), 1)


# ---- one stream, host memory ---------------------------------------------------------------------------------------------
def parse_host(window: np.ndarray, start: int, min_match_length: int, max_matches: int):
    """window: uint8 array = history + block, the block starts at ``start``.
    -> (literal_count, match_length, match_offset: uint32 arrays; literals: uint8 array)"""
    L = _lib.load()
    _lib.require_device()
    window = np.ascontiguousarray(window, np.uint8)
    n, start = int(window.size), int(start)
    cap = default_seq_cap(n - start, min_match_length)
    seq = np.zeros((3, cap), np.uint32)
    literals = np.zeros(max(n - start, 1), np.uint8)
    n_seq, n_lit = C.c_uint64(0), C.c_uint64(0)
    rc = L.scl_lz77_parse_host(_lib.u8_ptr(window), n, start, int(min_match_length), int(max_matches), _lib.u32_ptr(seq[0]),
                               _lib.u32_ptr(seq[1]), _lib.u32_ptr(seq[2]), cap, C.byref(n_seq), _lib.u8_ptr(literals),
                               n - start, C.byref(n_lit))
    _lib.check(rc, "scl_lz77_parse_host")
    k = n_seq.value
    return seq[0, :k].copy(), seq[1, :k].copy(), seq[2, :k].copy(), literals[: n_lit.value].copy()


def replay_host(history: np.ndarray, literal_count, match_length, match_offset, literals) -> np.ndarray:
    """-> the bytes the sequences and literals append to ``history`` (uint8 array).  A damaged sequence raises
    ``SclHipError`` (SCL_E_CHUNK) naming the status."""
    L = _lib.load()
    _lib.require_device()
    lc, ml, mo = (np.ascontiguousarray(a, np.uint32) for a in (literal_count, match_length, match_offset))
    literals = np.ascontiguousarray(literals, np.uint8)
    history = np.asarray(history, np.uint8)
    have = int(history.size)
    grow = int(literals.size) + int(ml.astype(np.int64).sum())
    if have + grow >= 1 << 32:
        raise ValueError(f"a window of {have + grow} bytes: positions inside a stream are 32-bit")
    buf = np.zeros(max(have + grow, 1), np.uint8)
    buf[:have] = history
    out_len = C.c_uint64(0)
    rc = L.scl_lz77_replay_host(_lib.u8_ptr(buf), have, have + grow, _lib.u32_ptr(lc), _lib.u32_ptr(ml), _lib.u32_ptr(mo),
                                int(lc.size), _lib.u8_ptr(literals), int(literals.size), C.byref(out_len))
    _lib.check(rc, "scl_lz77_replay_host")
    return buf[have: have + out_len.value]


# ---- batches, device memory (torch tensors) --------------------------------------------------------------------------------
@dataclass
class ParsedBatch:
    """Device-resident result of :func:`parse_batch`.  Row ``s`` of the three sequence arrays holds ``n_seq[s]`` entries;
    stream ``s``'s ``n_lit[s]`` literals start at ``literals[win_off[s] + start[s]]`` (the block's own place)."""

    literal_count: "torch.Tensor"  # uint32 as int32 [n_streams, seq_cap]
    match_length: "torch.Tensor"
    match_offset: "torch.Tensor"
    literals: "torch.Tensor"       # uint8, laid out like the windows
    n_seq: "torch.Tensor"          # int32 [n_streams]
    n_lit: "torch.Tensor"
    status: "torch.Tensor"
    lit_off: "torch.Tensor"        # int64 [n_streams] = win_off[:-1] + start
    seq_cap: int


def scratch_bytes(total_bytes: int, n_streams: int) -> int:
    return int(_lib.load().scl_lz77_scratch_bytes(int(total_bytes), int(n_streams)))


def _stream_handle(stream, device):
    import torch

    return stream if stream is not None else torch.cuda.current_stream(device).cuda_stream


def parse_batch(win, win_off, start, min_match_length: int, max_matches: int, seq_cap: int, scratch=None, stream=None,
                out: Optional[ParsedBatch] = None, phases: int = 0) -> ParsedBatch:
    """win: uint8 CUDA tensor (the windows back to back); win_off: int64 [n_streams + 1]; start: int32 [n_streams].
    ``seq_cap``: entries per row (``default_seq_cap`` of the longest block always suffices).  ``scratch``: a uint8 tensor of
    ``scratch_bytes(win.numel(), n_streams)`` bytes to reuse across calls; ``phases``: 0 = index and parse,
    ``lib.LZ77_INDEX`` / ``lib.LZ77_PARSE`` = one of them on the same scratch."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous()
    assert win_off.dtype == torch.int64 and start.dtype == torch.int32 and win_off.numel() == start.numel() + 1
    dev, n_streams, total = win.device, int(start.numel()), int(win.numel())
    need = scratch_bytes(total, n_streams)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    if out is None:
        rows = lambda: torch.zeros((n_streams, seq_cap), dtype=torch.int32, device=dev)  # noqa: E731
        words = lambda: torch.zeros(n_streams, dtype=torch.int32, device=dev)  # noqa: E731
        out = ParsedBatch(rows(), rows(), rows(), torch.zeros(max(total, 1), dtype=torch.uint8, device=dev), words(),
                          words(), words(), win_off[:-1] + start.to(torch.int64), int(seq_cap))
    a = _lib.Lz77ParseArgs(win.data_ptr(), win_off.data_ptr(), start.data_ptr(), n_streams, total, int(min_match_length),
                           int(max_matches), out.seq_cap, int(phases), out.literal_count.data_ptr(),
                           out.match_length.data_ptr(), out.match_offset.data_ptr(), out.literals.data_ptr(),
                           out.n_seq.data_ptr(), out.n_lit.data_ptr(), out.status.data_ptr(), scratch.data_ptr(),
                           int(scratch.numel()))
    with torch.cuda.device(dev):
        rc = L.scl_lz77_parse_batch(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_parse_batch")
    out._scratch = scratch  # the kernels read it asynchronously: it lives as long as the result
    return out


def replay_batch(win, win_off, have, literal_count, match_length, match_offset, n_seq, literals, lit_off, n_lit,
                 stream=None):
    """Appends to the windows in place.  win: uint8 CUDA tensor of slots, slot s = [win_off[s], win_off[s + 1]) holding
    ``have[s]`` bytes already; sequence rows as :class:`ParsedBatch`; stream s's ``n_lit[s]`` literals start at
    ``literals[lit_off[s]]``.  -> (out_len, status): int32 [n_streams] each."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous() and literals.dtype == torch.uint8
    assert win_off.dtype == torch.int64 and lit_off.dtype == torch.int64
    assert all(t.dtype == torch.int32 for t in (have, literal_count, match_length, match_offset, n_seq, n_lit))
    dev, n_streams = win.device, int(have.numel())
    assert win_off.numel() == n_streams + 1 and literal_count.dim() == 2 and literal_count.is_contiguous()
    assert match_length.is_contiguous() and match_offset.is_contiguous()
    assert match_length.shape == literal_count.shape == match_offset.shape and literal_count.shape[0] == n_streams
    out_len = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    status = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    a = _lib.Lz77ReplayArgs(win.data_ptr(), win_off.data_ptr(), have.data_ptr(), n_streams, int(win.numel()),
                            int(literal_count.shape[1]), 0, literal_count.data_ptr(), match_length.data_ptr(),
                            match_offset.data_ptr(), n_seq.data_ptr(), literals.data_ptr(), int(literals.numel()),
                            lit_off.data_ptr(), n_lit.data_ptr(), out_len.data_ptr(), status.data_ptr())
    with torch.cuda.device(dev):
        rc = L.scl_lz77_replay_batch(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_replay_batch")
    return out_len, status


def kernel_names():
    """-> (index, parse, replay) kernel names as a kernel trace prints them"""
    bufs = [C.create_string_buffer(128) for _ in range(3)]
    _lib.check(_lib.load().scl_lz77_kernel_names(*bufs, 128), "scl_lz77_kernel_names")
    return tuple(b.value.decode() for b in bufs)
