"""LZ77 on the device: the LZ layer (csrc/scl_lz77.hip: match index + greedy parse, and sequence replay) and the entropy
stage above it (csrc/scl_lz77_entropy.hip: sequences and literals <-> the reference's block bits).

Two call shapes, as in :mod:`.models`:

* ``parse_host`` / ``replay_host`` -- one stream in host memory (what ``LZ77Encoder`` / ``LZ77Decoder`` use); from
  ``wide_threshold()`` bytes on the library spreads the stream over the whole GPU (csrc/scl_lz77_wide.hip), with the same
  results;
* ``parse_wide`` / ``replay_wide`` -- that wide path on ONE stream resident in HBM: a :class:`ParsedBatch` of one stream;
* ``parse_batch`` / ``replay_batch`` -- many independent streams resident in HBM, given as torch tensors;
  ``encode_batch`` / ``decode_batch`` turn their sequences and literals into block bits and back, ``compress_batch`` /
  ``decompress_batch`` do both steps.  No call loops over streams on the host;
* ``encode_wide`` / ``decode_wide`` -- that entropy stage for ONE stream on the whole GPU (csrc/scl_lz77_entropy_wide.hip),
  the same bits; ``compress_wide`` / ``decompress_wide`` = ``parse_wide`` + ``encode_wide`` / ``decode_wide`` + ``replay_wide``;
* ``sliding_parse_host`` / ``sliding_replay_host`` / ``sliding_parse_batch`` / ``sliding_replay_batch`` /
  ``sliding_compress_batch`` / ``sliding_decompress_batch`` -- the same shapes for the sliding-window coder
  (csrc/scl_lz77_sliding.hip: hash-bucket index, lazy parse, windowed replay); its :class:`ParsedBatch` goes through the
  same ``encode_batch``.  From ``sliding_wide_threshold()`` bytes on the host calls spread the stream over the whole GPU;
* ``sliding_parse_wide`` / ``sliding_replay_wide`` / ``sliding_compress_wide`` / ``sliding_decompress_wide`` -- that wide
  path of the sliding-window coder on ONE stream resident in HBM (csrc/scl_lz77_sliding_wide.hip), the same results.

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
def _parse_host(entry: str, window, start: int, seq_cap, extra, device_first: bool):
    """One host parse through the C call ``entry``, whose own parameters ``extra`` stand between ``start`` and the rows;
    ``seq_cap(block_len)`` sizes the rows.  ``device_first``: ask for a device before anything else, else only once the
    call has not refused a parameter (that is reported as such, device or not)."""
    L = _lib.load()
    if device_first:
        _lib.require_device()
    window = np.ascontiguousarray(window, np.uint8)
    n, start = int(window.size), int(start)
    cap = seq_cap(n - start)
    seq = np.zeros((3, cap), np.uint32)
    literals = np.zeros(max(n - start, 1), np.uint8)
    n_seq, n_lit = C.c_uint64(0), C.c_uint64(0)
    rc = getattr(L, entry)(_lib.u8_ptr(window), n, start, *extra, _lib.u32_ptr(seq[0]), _lib.u32_ptr(seq[1]),
                           _lib.u32_ptr(seq[2]), cap, C.byref(n_seq), _lib.u8_ptr(literals), n - start, C.byref(n_lit))
    if not device_first and rc != _lib.E_PARAM:
        _lib.require_device()
    _lib.check(rc, entry)
    k = n_seq.value
    return seq[0, :k].copy(), seq[1, :k].copy(), seq[2, :k].copy(), literals[: n_lit.value].copy()


def parse_host(window: np.ndarray, start: int, min_match_length: int, max_matches: int):
    """window: uint8 array = history + block, the block starts at ``start``.
    -> (literal_count, match_length, match_offset: uint32 arrays; literals: uint8 array)"""
    return _parse_host("scl_lz77_parse_host", window, start, lambda block: default_seq_cap(block, min_match_length),
                       (int(min_match_length), int(max_matches)), device_first=True)


def _replay_host(entry: str, history, literal_count, match_length, match_offset, literals, extra):
    """One host replay through the C call ``entry``, whose own parameters ``extra`` stand between the capacity and the rows"""
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
    rc = getattr(L, entry)(_lib.u8_ptr(buf), have, have + grow, *extra, _lib.u32_ptr(lc), _lib.u32_ptr(ml),
                           _lib.u32_ptr(mo), int(lc.size), _lib.u8_ptr(literals), int(literals.size), C.byref(out_len))
    _lib.check(rc, entry)
    return buf[have: have + out_len.value]


def replay_host(history: np.ndarray, literal_count, match_length, match_offset, literals) -> np.ndarray:
    """-> the bytes the sequences and literals append to ``history`` (uint8 array).  A damaged sequence raises
    ``SclHipError`` (SCL_E_CHUNK) naming the status."""
    return _replay_host("scl_lz77_replay_host", history, literal_count, match_length, match_offset, literals, ())


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


def _kernel_names(entry: str, count: int = 3):
    """the ``count`` kernel names the C call ``entry`` writes, as a kernel trace prints them"""
    bufs = [C.create_string_buffer(128) for _ in range(count)]
    _lib.check(getattr(_lib.load(), entry)(*bufs, 128), entry)
    return tuple(b.value.decode() for b in bufs)


def _new_parsed(n_streams: int, seq_cap: int, lit_bytes: int, lit_off, dev) -> ParsedBatch:
    """a fresh, zeroed :class:`ParsedBatch` of ``n_streams`` rows with ``lit_bytes`` bytes for the literals"""
    import torch

    rows = lambda: torch.zeros((n_streams, seq_cap), dtype=torch.int32, device=dev)  # noqa: E731
    words = lambda: torch.zeros(n_streams, dtype=torch.int32, device=dev)  # noqa: E731
    return ParsedBatch(rows(), rows(), rows(), torch.zeros(max(lit_bytes, 1), dtype=torch.uint8, device=dev), words(),
                       words(), words(), lit_off, int(seq_cap))


def _longest_block(win_off, start) -> int:
    """the longest block of a batch: one read-back (uint32 values travel as int32 bit patterns)"""
    import torch

    lens = win_off[1:] - win_off[:-1] - start.to(torch.int64).bitwise_and(0xFFFFFFFF)
    return max(int(lens.max().item()), 0) if start.numel() else 0


def _parse_batch(entry: str, need_bytes, fill, win, win_off, start, seq_cap, scratch, stream, out):
    """The parse of a batch through the C call ``entry``: ``need_bytes(total, n_streams)`` sizes the scratch,
    ``fill(out, scratch, n_streams, total)`` makes the argument struct, and a ``seq_cap`` given as a function is called
    with the longest block when neither ``out`` nor the caller brings a number"""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous()
    assert win_off.dtype == torch.int64 and start.dtype == torch.int32 and win_off.numel() == start.numel() + 1
    dev, n_streams, total = win.device, int(start.numel()), int(win.numel())
    if out is not None:
        seq_cap = out.seq_cap
    if callable(seq_cap):
        seq_cap = seq_cap(_longest_block(win_off, start))
    need = need_bytes(total, n_streams)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    if out is None:
        out = _new_parsed(n_streams, seq_cap, total, win_off[:-1] + start.to(torch.int64), dev)
    a = fill(out, scratch, n_streams, total)
    with torch.cuda.device(dev):
        rc = getattr(L, entry)(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, entry)
    out._scratch = scratch  # the kernels read it asynchronously: it lives as long as the result
    return out


def parse_batch(win, win_off, start, min_match_length: int, max_matches: int, seq_cap: int, scratch=None, stream=None,
                out: Optional[ParsedBatch] = None, phases: int = 0) -> ParsedBatch:
    """win: uint8 CUDA tensor (the windows back to back); win_off: int64 [n_streams + 1]; start: int32 [n_streams].
    ``seq_cap``: entries per row (``default_seq_cap`` of the longest block always suffices).  ``scratch``: a uint8 tensor of
    ``scratch_bytes(win.numel(), n_streams)`` bytes to reuse across calls; ``phases``: 0 = index and parse,
    ``lib.LZ77_INDEX`` / ``lib.LZ77_PARSE`` = one of them on the same scratch."""
    def fill(out, scratch, n_streams, total):
        return _lib.Lz77ParseArgs(win.data_ptr(), win_off.data_ptr(), start.data_ptr(), n_streams, total,
                                  int(min_match_length), int(max_matches), out.seq_cap, int(phases),
                                  out.literal_count.data_ptr(), out.match_length.data_ptr(), out.match_offset.data_ptr(),
                                  out.literals.data_ptr(), out.n_seq.data_ptr(), out.n_lit.data_ptr(),
                                  out.status.data_ptr(), scratch.data_ptr(), int(scratch.numel()))

    return _parse_batch("scl_lz77_parse_batch", scratch_bytes, fill, win, win_off, start, seq_cap, scratch, stream, out)


def _replay_batch(entry: str, args, window: int, win, win_off, have, literal_count, match_length, match_offset, n_seq,
                  literals, lit_off, n_lit, stream):
    """The replay of a batch through the C call ``entry``; ``args`` is its argument struct, whose seventh field takes
    ``window``: the sliding-window coder's ``window_size``, 0 for the greedy one's ``reserved``"""
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
    a = args(win.data_ptr(), win_off.data_ptr(), have.data_ptr(), n_streams, int(win.numel()), int(literal_count.shape[1]),
             int(window), literal_count.data_ptr(), match_length.data_ptr(), match_offset.data_ptr(), n_seq.data_ptr(),
             literals.data_ptr(), int(literals.numel()), lit_off.data_ptr(), n_lit.data_ptr(), out_len.data_ptr(),
             status.data_ptr())
    with torch.cuda.device(dev):
        rc = getattr(L, entry)(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, entry)
    return out_len, status


def replay_batch(win, win_off, have, literal_count, match_length, match_offset, n_seq, literals, lit_off, n_lit,
                 stream=None):
    """Appends to the windows in place.  win: uint8 CUDA tensor of slots, slot s = [win_off[s], win_off[s + 1]) holding
    ``have[s]`` bytes already; sequence rows as :class:`ParsedBatch`; stream s's ``n_lit[s]`` literals start at
    ``literals[lit_off[s]]``.  -> (out_len, status): int32 [n_streams] each."""
    return _replay_batch("scl_lz77_replay_batch", _lib.Lz77ReplayArgs, 0, win, win_off, have, literal_count, match_length,
                         match_offset, n_seq, literals, lit_off, n_lit, stream)


# ---- one large stream across the whole GPU (csrc/scl_lz77_wide.hip) ------------------------------------------------------------
def wide_shape():
    """-> (tile, cap): positions per tile and the cap of a scored extension, the kernels' compile-time shape"""
    tile, cap = C.c_uint32(0), C.c_uint32(0)
    _lib.load().scl_lz77_wide_shape(C.byref(tile), C.byref(cap))
    return tile.value, cap.value


def wide_threshold() -> int:
    """block bytes from which ``parse_host`` / ``replay_host`` take the wide path"""
    return int(_lib.load().scl_lz77_wide_threshold())


def wide_scratch_bytes(n: int) -> int:
    return int(_lib.load().scl_lz77_wide_scratch_bytes(int(n)))


def wide_replay_scratch_bytes(n_seq: int, grow_bytes: int) -> int:
    return int(_lib.load().scl_lz77_wide_replay_scratch_bytes(int(n_seq), int(grow_bytes)))


def wide_kernel_names():
    """-> (score, walk, resolve) kernel names as a kernel trace prints them"""
    return _kernel_names("scl_lz77_wide_kernel_names")


def parse_wide(win, start: int, min_match_length: int, max_matches: int, seq_cap: Optional[int] = None, scratch=None,
               stream=None, out: Optional[ParsedBatch] = None, phases: int = 0) -> ParsedBatch:
    """win: uint8 CUDA tensor, ONE window whose block starts at ``start``; 1 <= ``max_matches`` <= 64.  -> what
    ``parse_batch`` returns for a batch of this one stream (``n_streams == 1``: ``encode_batch`` takes it as it is).
    ``seq_cap`` defaults to ``default_seq_cap`` of the block; ``scratch``: a uint8 tensor of at least
    ``wide_scratch_bytes(win.numel())`` bytes to reuse across calls; ``out``: a one-stream :class:`ParsedBatch` whose
    buffers are written instead of new ones (its ``seq_cap`` holds); ``phases``: 0 = everything, else a mask of
    ``lib.LZ77_WIDE_INDEX`` / ``_SCORE`` / ``_WALK`` / ``_EMIT`` run on the same scratch (for measurements)."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous() and win.dim() == 1
    dev, n, start = win.device, int(win.numel()), int(start)
    if out is not None:
        seq_cap = out.seq_cap
    if seq_cap is None:
        seq_cap = default_seq_cap(n - start, min_match_length)
    need = wide_scratch_bytes(n)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    if out is None:
        out = _new_parsed(1, seq_cap, n, torch.full((1,), start, dtype=torch.int64, device=dev), dev)
    assert out.literal_count.shape == (1, out.seq_cap) and out.literals.numel() >= n
    a = _lib.Lz77WideParseArgs(win.data_ptr(), n, start, int(min_match_length), int(max_matches), out.seq_cap, int(phases),
                               out.literal_count.data_ptr(), out.match_length.data_ptr(), out.match_offset.data_ptr(),
                               out.literals.data_ptr(), out.n_seq.data_ptr(), out.n_lit.data_ptr(), out.status.data_ptr(),
                               scratch.data_ptr(), int(scratch.numel()))
    with torch.cuda.device(dev):
        rc = L.scl_lz77_parse_wide(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_parse_wide")
    out._scratch = scratch  # the kernels read it asynchronously: it lives as long as the result
    return out


def replay_wide(win, have: int, literal_count, match_length, match_offset, n_seq: int, literals, n_lit: int, cap=None,
                scratch=None, stream=None):
    """Appends to ``win[:cap]`` (default: all of it) in place, which holds ``have`` bytes already: ONE stream's ``n_seq``
    sequences (int32 tensors, the first ``n_seq`` entries of each) and ``n_lit`` literals from ``literals[0]`` on; the
    counts are host integers, they size the launches.  -> (out_len, status): int32 [1] each, as ``replay_batch``."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous() and literals.dtype == torch.uint8
    rows = tuple(t.reshape(-1) for t in (literal_count, match_length, match_offset))
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= int(n_seq) for t in rows)
    assert literals.numel() >= int(n_lit)
    dev, have, cap = win.device, int(have), int(win.numel() if cap is None else cap)
    assert cap <= win.numel()
    need = wide_replay_scratch_bytes(n_seq, max(cap - have, 0))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    out_len = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _lib.Lz77WideReplayArgs(win.data_ptr(), have, cap, rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(),
                                int(n_seq), literals.data_ptr(), int(n_lit), out_len.data_ptr(), status.data_ptr(),
                                scratch.data_ptr(), int(scratch.numel()))
    with torch.cuda.device(dev):
        rc = L.scl_lz77_replay_wide(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_replay_wide")
    out_len._inputs = (rows, literals, scratch)  # read asynchronously: they live as long as the result
    return out_len, status


# ---- the entropy stage: sequences and literals <-> block bits (csrc/scl_lz77_entropy.hip) ------------------------------------
DEFAULT_BINNED_OFFSET = 16  # LZ77StreamsEncoder's log_scale_binned_coder_offset


@dataclass
class EncodedBatch:
    """Device-resident result of :func:`encode_batch`: stream ``s`` is the ``nbits[s]`` bits from absolute bit
    ``bit_offset[s]`` (= ``8 * s * out_stride``) of ``bits`` -- the bits ``LZ77StreamsEncoder.encode_block`` returns.
    ``models.compact`` / ``compact_into`` (``scl_streams_compact``) take it as they take any batch of slots.

    LOOK AT ``status`` BEFORE COMPACTING.  A stream with a non-zero status has stored nothing, but ``nbits[s]`` of a
    ``lib.ST_CAPACITY`` stream is the length it needs, which is more than its slot: the compaction knows no slot size and
    would read that many bits from the slot on.  Encode such a batch again with a larger ``out_stride``."""

    bits: "torch.Tensor"        # uint8 [n_streams * out_stride + 16]
    bit_offset: "torch.Tensor"  # uint64 as int64 [n_streams]
    nbits: "torch.Tensor"       # uint32 as int32 [n_streams]
    status: "torch.Tensor"      # int32 [n_streams]
    out_stride: int

    # the names models.EncodedBatch gives the same things
    layout = "linear"
    data = property(lambda self: self.bits)
    stride = property(lambda self: self.out_stride)
    n_chunks = property(lambda self: int(self.nbits.numel()))


@dataclass
class DecodedBatch(ParsedBatch):
    """:class:`ParsedBatch` as :func:`decode_batch` fills it, plus ``consumed[s]`` = the bits of stream s the block took
    (``LZ77StreamsDecoder.decode_block``'s ``num_bits_consumed``)"""

    consumed: "torch.Tensor" = None


def entropy_slot_bytes(max_n_seq: int, max_n_lit: int, binned_offset: int = DEFAULT_BINNED_OFFSET) -> int:
    return int(_lib.load().scl_lz77_entropy_slot_bytes(int(max_n_seq), int(max_n_lit), int(binned_offset)))


def encode_batch(parsed: ParsedBatch, binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None,
                 stream=None, out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """The reference's block bits of every stream of ``parsed``, each in a slot of ``out_stride`` bytes (a multiple of 16;
    default: ``entropy_slot_bytes`` of the largest counts, which reads ``n_seq`` / ``n_lit`` back once).  ``status[s]``:
    ``lib.ST_CAPACITY`` = the slot is too small (``nbits[s]`` says what it takes), see include/scl_hip.h for the rest.
    ``out``: an :class:`EncodedBatch` whose buffers are written instead of new ones (``bits`` 16-byte aligned, at least
    ``n_streams * out.out_stride`` bytes)."""
    import torch

    L = _lib.load()
    lc, ml, mo = parsed.literal_count, parsed.match_length, parsed.match_offset
    assert lc.is_cuda and lc.dim() == 2 and lc.shape == ml.shape == mo.shape
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (lc, ml, mo, parsed.n_seq, parsed.n_lit))
    assert parsed.literals.dtype == torch.uint8 and parsed.lit_off.dtype == torch.int64
    dev, n_streams = lc.device, int(parsed.n_seq.numel())
    assert lc.shape[0] == n_streams and parsed.n_lit.numel() == n_streams and parsed.lit_off.numel() == n_streams
    lit_off = parsed.lit_off.contiguous()
    if out is not None:
        out_stride = out.out_stride
    if out_stride is None:
        top_seq = int(parsed.n_seq.max().item()) if n_streams else 0
        top_lit = int(parsed.n_lit.to(torch.int64).bitwise_and(0xFFFFFFFF).max().item()) if n_streams else 0
        out_stride = entropy_slot_bytes(min(top_seq & 0xFFFFFFFF, int(lc.shape[1])), top_lit, binned_offset)
    out_stride = int(out_stride)
    if out is None:
        out = EncodedBatch(torch.zeros(n_streams * out_stride + 16, dtype=torch.uint8, device=dev),
                           torch.zeros(n_streams, dtype=torch.int64, device=dev),
                           torch.zeros(n_streams, dtype=torch.int32, device=dev),
                           torch.zeros(n_streams, dtype=torch.int32, device=dev), out_stride)
    bits, bit_offset, nbits, status = out.bits, out.bit_offset, out.nbits, out.status
    assert bits.dtype == torch.uint8 and bits.is_contiguous() and bits.numel() >= n_streams * out_stride
    assert bit_offset.numel() == n_streams and nbits.numel() == n_streams and status.numel() == n_streams
    a = _lib.Lz77EntropyEncodeArgs(n_streams, int(lc.shape[1]), int(binned_offset), lc.data_ptr(), ml.data_ptr(),
                                   mo.data_ptr(), parsed.n_seq.data_ptr(), parsed.literals.data_ptr(),
                                   int(parsed.literals.numel()), lit_off.data_ptr(), parsed.n_lit.data_ptr(),
                                   bits.data_ptr(), out_stride, bit_offset.data_ptr(), nbits.data_ptr(), status.data_ptr())
    with torch.cuda.device(dev):
        rc = L.scl_lz77_entropy_encode_batch(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_entropy_encode_batch")
    out._inputs = (parsed, lit_off)  # read asynchronously: they live as long as the result
    return out


def decode_batch(bits, bit_offset, nbits, seq_cap: int, lit_off, lit_cap, binned_offset: int = DEFAULT_BINNED_OFFSET,
                 stream=None, out: Optional[DecodedBatch] = None) -> DecodedBatch:
    """bits: uint8 CUDA tensor; stream s = the ``nbits[s]`` (int32) bits from absolute bit ``bit_offset[s]`` (int64) on, at
    any alignment.  Its sequences go to row s (``seq_cap`` entries) of the result, its literals to
    ``literals[lit_off[s] : lit_off[s] + lit_cap[s]]`` (int64 / int32 per stream); ``literals`` has ``max(lit_off +
    lit_cap)`` bytes unless ``out`` brings buffers of its own.  -> :class:`DecodedBatch` (``status``, ``consumed``: int32)."""
    import torch

    L = _lib.load()
    assert bits.is_cuda and bits.dtype == torch.uint8 and bits.is_contiguous()
    assert bit_offset.dtype == torch.int64 and lit_off.dtype == torch.int64
    assert nbits.dtype == torch.int32 and lit_cap.dtype == torch.int32
    dev, n_streams = bits.device, int(nbits.numel())
    assert bit_offset.numel() == n_streams and lit_off.numel() == n_streams and lit_cap.numel() == n_streams
    bit_offset, nbits, lit_off, lit_cap = (t.contiguous() for t in (bit_offset, nbits, lit_off, lit_cap))
    if out is None:
        lit_bytes = int((lit_off + lit_cap.to(torch.int64).bitwise_and(0xFFFFFFFF)).max().item()) if n_streams else 0
        rows = lambda: torch.zeros((n_streams, seq_cap), dtype=torch.int32, device=dev)  # noqa: E731
        words = lambda: torch.zeros(n_streams, dtype=torch.int32, device=dev)  # noqa: E731
        out = DecodedBatch(rows(), rows(), rows(), torch.zeros(max(lit_bytes, 1), dtype=torch.uint8, device=dev), words(),
                           words(), words(), lit_off, int(seq_cap), words())
    assert out.seq_cap == int(seq_cap) and out.literal_count.shape == (n_streams, int(seq_cap))
    a = _lib.Lz77EntropyDecodeArgs(bits.data_ptr(), int(bits.numel()), bit_offset.data_ptr(), nbits.data_ptr(), n_streams,
                                   int(seq_cap), int(binned_offset), out.literal_count.data_ptr(),
                                   out.match_length.data_ptr(), out.match_offset.data_ptr(), out.n_seq.data_ptr(),
                                   out.literals.data_ptr(), int(out.literals.numel()), lit_off.data_ptr(),
                                   lit_cap.data_ptr(), out.n_lit.data_ptr(), out.consumed.data_ptr(), out.status.data_ptr())
    with torch.cuda.device(dev):
        rc = L.scl_lz77_entropy_decode_batch(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_entropy_decode_batch")
    out._inputs = (bits, bit_offset, nbits, lit_off, lit_cap)
    return out


def compress_batch(win, win_off, start, min_match_length: int, max_matches: int, seq_cap: Optional[int] = None,
                   binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None, scratch=None, stream=None):
    """parse + encode: the blocks of a batch of windows (see :func:`parse_batch`) -> (:class:`EncodedBatch`,
    :class:`ParsedBatch`).  A stream's status is ``parsed.status[s] | encoded.status[s]``: nothing here reads it back, so
    check it before the bits are used (see :class:`EncodedBatch`).  ``seq_cap`` defaults to ``default_seq_cap`` of the
    longest block and ``out_stride`` to ``entropy_slot_bytes(seq_cap, longest block)`` -- a block has at most as many
    literals as bytes -- so the defaults cost ONE read-back, of the block lengths, before anything is launched; parse and
    encode then follow each other on ``stream`` without the host in between.  That stride is the worst case (about 3.5
    bytes per input byte at ``min_match_length`` 6); pass a smaller one where the data allows it."""
    seq_cap, out_stride = _default_caps(win_off, start, seq_cap, out_stride, binned_offset,
                                        lambda longest: default_seq_cap(longest, min_match_length))
    parsed = parse_batch(win, win_off, start, min_match_length, max_matches, seq_cap, scratch=scratch, stream=stream)
    return encode_batch(parsed, binned_offset, out_stride, stream=stream), parsed


def _default_caps(win_off, start, seq_cap, out_stride, binned_offset, seq_cap_of):
    """``seq_cap`` and ``out_stride`` of a compress call with the missing ones filled in from the longest block"""
    if seq_cap is None or out_stride is None:
        longest = _longest_block(win_off, start)
        if seq_cap is None:
            seq_cap = seq_cap_of(longest)
        if out_stride is None:
            out_stride = entropy_slot_bytes(seq_cap, longest, binned_offset)
    return seq_cap, out_stride


def _decompress_batch(replay, bits, bit_offset, nbits, win, win_off, have, seq_cap, binned_offset, stream):
    """decode + ``replay`` (``replay_batch`` or ``sliding_replay_batch`` with its window), the literals of stream s in the
    room its slot has left"""
    import torch

    # (uint32 values travel as int32 bit patterns: masked on the way in, wrapped on the way out)
    room = (win_off[1:] - win_off[:-1] - have.to(torch.int64).bitwise_and(0xFFFFFFFF)).clamp(min=0, max=0xFFFFFFFF)
    lit_off = torch.cumsum(room, 0) - room
    lit_cap = torch.where(room >= 1 << 31, room - (1 << 32), room).to(torch.int32)
    decoded = decode_batch(bits, bit_offset, nbits, seq_cap, lit_off, lit_cap, binned_offset, stream=stream)
    out_len, status = replay(win, win_off, have, decoded.literal_count, decoded.match_length, decoded.match_offset,
                             decoded.n_seq, decoded.literals, lit_off, decoded.n_lit, stream=stream)
    return out_len, status | decoded.status, decoded.consumed


def decompress_batch(bits, bit_offset, nbits, win, win_off, have, seq_cap: int,
                     binned_offset: int = DEFAULT_BINNED_OFFSET, stream=None):
    """decode + replay: appends the block of every stream to its window slot ``win[win_off[s] : win_off[s + 1]]``, which
    holds ``have[s]`` bytes already (see :func:`replay_batch`).  A block has at most as many literals as bytes, so the
    room left in the slot bounds them.  -> (out_len, status, consumed): int32 [n_streams] each; status = the decoder's
    | the replay's (a stream the decoder faulted on replays what was decoded before the fault)."""
    return _decompress_batch(replay_batch, bits, bit_offset, nbits, win, win_off, have, seq_cap, binned_offset, stream)


# ---- the entropy stage of one large stream across the whole GPU (csrc/scl_lz77_entropy_wide.hip) ----------------------------
def entropy_wide_threshold() -> int:
    """coded values of a stream, ``3 * n_seq + n_lit``, from which ``encode_wide`` / ``decode_wide`` beat ``encode_batch`` /
    ``decode_batch`` on a batch of one (measured: DESIGN.md 3.6.3); the bits are the same on both sides of it"""
    return int(_lib.load().scl_lz77_entropy_wide_threshold())


def entropy_wide_scratch_bytes(n_seq: int, n_lit: int, in_nbits: int = 0) -> int:
    """scratch for ``encode_wide`` of ``n_seq`` sequences and ``n_lit`` literals, and for ``decode_wide`` of ``in_nbits``
    bits with ``seq_cap = n_seq``, ``lit_cap = n_lit``"""
    return int(_lib.load().scl_lz77_entropy_wide_scratch_bytes(int(n_seq), int(n_lit), int(in_nbits)))


def entropy_wide_kernel_names():
    """-> (emit, sync, resid) kernel names of the wide entropy stage as a kernel trace prints them"""
    return _kernel_names("scl_lz77_entropy_wide_kernel_names")


def encode_wide(parsed: ParsedBatch, binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None,
                n_seq: Optional[int] = None, n_lit: Optional[int] = None, lit_off: Optional[int] = None, scratch=None,
                stream=None, out: Optional[EncodedBatch] = None) -> EncodedBatch:
    """``encode_batch`` for a ONE-stream :class:`ParsedBatch` (what ``parse_wide`` returns) on the whole GPU: the same bits,
    ``nbits`` and ``status`` in an :class:`EncodedBatch` of one slot, so ``models.compact`` takes it unchanged.  ``n_seq`` /
    ``n_lit`` / ``lit_off`` size the launches: they are read back once (one copy) unless all three are passed.
    ``out_stride``: the slot's bytes, ANY positive count here (default: ``entropy_slot_bytes`` of the counts); nothing at or
    past it is written.  ``result.nbits64`` is the length as int64 (``nbits`` is its low 32 bits); asynchronous otherwise.
    ``scratch``: a uint8 tensor of at least ``entropy_wide_scratch_bytes(n_seq, n_lit)`` bytes to reuse across calls."""
    import torch

    L = _lib.load()
    lc, ml, mo = parsed.literal_count, parsed.match_length, parsed.match_offset
    assert lc.is_cuda and lc.dim() == 2 and lc.shape == ml.shape == mo.shape and lc.shape[0] == 1
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (lc, ml, mo))
    assert parsed.literals.dtype == torch.uint8 and parsed.literals.is_contiguous()
    dev = lc.device
    if n_seq is None or n_lit is None or lit_off is None:
        words = torch.cat((parsed.n_seq.to(torch.int64).bitwise_and(0xFFFFFFFF),
                           parsed.n_lit.to(torch.int64).bitwise_and(0xFFFFFFFF), parsed.lit_off.reshape(-1))).cpu().tolist()
        n_seq = words[0] if n_seq is None else n_seq
        n_lit = words[1] if n_lit is None else n_lit
        lit_off = words[2] if lit_off is None else lit_off
    n_seq, n_lit, lit_off = int(n_seq), int(n_lit), int(lit_off)
    assert n_seq <= lc.shape[1] and lit_off + n_lit <= parsed.literals.numel()
    if out is not None:
        out_stride = out.out_stride
    if out_stride is None:
        out_stride = entropy_slot_bytes(n_seq, n_lit, binned_offset)
    out_stride = int(out_stride)
    if out is None:
        out = EncodedBatch(torch.zeros(out_stride + 16, dtype=torch.uint8, device=dev),
                           torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev), out_stride)
    assert out.bits.dtype == torch.uint8 and out.bits.is_contiguous() and out.bits.numel() >= out_stride
    assert out.nbits.numel() == 1 and out.status.numel() == 1 and out.bit_offset.numel() == 1
    need = entropy_wide_scratch_bytes(n_seq, n_lit)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    nbits64 = torch.zeros(1, dtype=torch.int64, device=dev)
    a = _lib.Lz77EntropyWideEncodeArgs(lc.data_ptr(), ml.data_ptr(), mo.data_ptr(), n_seq,
                                       parsed.literals.data_ptr() + lit_off, n_lit, int(binned_offset), 0,
                                       out.bits.data_ptr(), out_stride, nbits64.data_ptr(), out.status.data_ptr(),
                                       scratch.data_ptr(), int(scratch.numel()))
    handle = _stream_handle(stream, dev)
    with torch.cuda.device(dev):
        rc = L.scl_lz77_entropy_encode_wide(C.byref(a), handle)
    _lib.check(rc, "scl_lz77_entropy_encode_wide")
    with torch.cuda.device(dev), torch.cuda.stream(None if stream is None else torch.cuda.ExternalStream(handle, device=dev)):
        out.nbits.copy_(nbits64.to(torch.int32))  # the low 32 bits, as the batch call's words
        out.bit_offset.zero_()
    out.nbits64 = nbits64
    out._inputs = (parsed, scratch)  # read asynchronously: they live as long as the result
    return out


def decode_wide(bits, bit_offset: int, nbits: int, seq_cap: int, lit_cap: int, binned_offset: int = DEFAULT_BINNED_OFFSET,
                scratch=None, stream=None, out: Optional[DecodedBatch] = None) -> DecodedBatch:
    """``decode_batch`` for ONE stream on the whole GPU: the ``nbits`` bits from absolute bit ``bit_offset`` of ``bits`` (host
    integers, any bit alignment) -> a one-stream :class:`DecodedBatch` (literals from ``literals[0]`` on; ``consumed`` is
    int64 here, and ``sync_passes`` counts the decoder's extra passes).  SYNCHRONISING on ``stream``: the field positions
    are read back as the call goes.  ``scratch``: at least ``entropy_wide_scratch_bytes(seq_cap, lit_cap, nbits)`` bytes."""
    import torch

    L = _lib.load()
    assert bits.is_cuda and bits.dtype == torch.uint8 and bits.is_contiguous()
    dev, seq_cap, lit_cap = bits.device, int(seq_cap), int(lit_cap)
    if out is None:
        rows = lambda: torch.zeros((1, seq_cap), dtype=torch.int32, device=dev)  # noqa: E731
        out = DecodedBatch(rows(), rows(), rows(), torch.zeros(max(lit_cap, 1), dtype=torch.uint8, device=dev), None, None,
                           None, torch.zeros(1, dtype=torch.int64, device=dev), seq_cap, None)
    assert out.seq_cap == seq_cap and out.literal_count.shape == (1, seq_cap) and out.literals.numel() >= lit_cap
    need = entropy_wide_scratch_bytes(seq_cap, lit_cap, nbits)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    result = torch.zeros(6, dtype=torch.int32, device=dev)  # scl_lz77_entropy_wide_result
    a = _lib.Lz77EntropyWideDecodeArgs(bits.data_ptr(), int(bits.numel()), int(bit_offset), int(nbits), int(binned_offset), 0,
                                       seq_cap, lit_cap, out.literal_count.data_ptr(), out.match_length.data_ptr(),
                                       out.match_offset.data_ptr(), out.literals.data_ptr(), result.data_ptr(),
                                       scratch.data_ptr(), int(scratch.numel()))
    with torch.cuda.device(dev):
        rc = L.scl_lz77_entropy_decode_wide(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_entropy_decode_wide")
    out.consumed, out.n_seq, out.n_lit = result[0:2].view(torch.int64), result[2:3], result[3:4]
    out.status, out.sync_passes = result[4:5], result[5:6]
    out._inputs = (bits, scratch, result)
    return out


def compress_wide(win, start: int, min_match_length: int, max_matches: int, seq_cap: Optional[int] = None,
                  binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None, scratch=None, stream=None,
                  out: Optional[EncodedBatch] = None):
    """``parse_wide`` + ``encode_wide``: ONE window whose block starts at ``start`` -> (:class:`EncodedBatch` of one slot,
    :class:`ParsedBatch`), the bits of ``compress_batch`` for a batch of this one stream.  The counts are read back once
    between the two steps (they size the encoder's launches).  ``scratch`` serves both steps, one after the other: at least
    ``wide_scratch_bytes(win.numel())`` and ``entropy_wide_scratch_bytes`` of the counts."""
    parsed = parse_wide(win, start, min_match_length, max_matches, seq_cap=seq_cap, scratch=scratch, stream=stream)
    return encode_wide(parsed, binned_offset, out_stride, lit_off=int(start), scratch=scratch, stream=stream, out=out), parsed


def decompress_wide(bits, bit_offset: int, nbits: int, win, have: int, seq_cap: int,
                    binned_offset: int = DEFAULT_BINNED_OFFSET, scratch=None, stream=None):
    """``decode_wide`` + ``replay_wide``: appends the block to ``win``, which holds ``have`` bytes already.  The room left in
    the window bounds the literals.  -> (out_len, status, consumed): status = the decoder's | the replay's."""
    lit_cap = max(int(win.numel()) - int(have), 0)
    decoded = decode_wide(bits, bit_offset, nbits, seq_cap, lit_cap, binned_offset, scratch=scratch, stream=stream)
    n_seq, n_lit = (int(x) & 0xFFFFFFFF for x in decoded._inputs[2][2:4].cpu().tolist())
    out_len, status = replay_wide(win, have, decoded.literal_count, decoded.match_length, decoded.match_offset, n_seq,
                                  decoded.literals, n_lit, stream=stream)
    return out_len, status | decoded.status, decoded.consumed


def entropy_kernel_names():
    """-> (encode, decode) kernel names of the entropy stage as a kernel trace prints them"""
    return _kernel_names("scl_lz77_entropy_kernel_names", 2)


def huffman_from_counts(counts):
    """The tree builder of the entropy kernels, run on the host: counts [K <= 256] -> (codes uint32, lengths uint8), the
    codeword of symbol i = the ``lengths[i]`` low bits of ``codes[i]``; (0, 0) for a symbol without a count.  Raises
    ``SclHipError`` (SCL_E_PARAM) for a code above 32 bits.  Needs no device."""
    counts = np.ascontiguousarray(counts, np.uint64)
    code, length = np.zeros(counts.size, np.uint32), np.zeros(counts.size, np.uint8)
    rc = _lib.load().scl_lz77_huffman_from_counts_host(counts.ctypes.data_as(_lib._u64p), int(counts.size),
                                                      _lib.u32_ptr(code), _lib.u8_ptr(length))
    _lib.check(rc, "scl_lz77_huffman_from_counts_host")
    return code, length


def kernel_names():
    """-> (index, parse, replay) kernel names as a kernel trace prints them"""
    return _kernel_names("scl_lz77_kernel_names")


# ---- sliding window: hash-bucket index, lazy parse, windowed replay (csrc/scl_lz77_sliding.hip) -------------------------------
MAX_HASH_LENGTH = 8          # a gram is hashed from at most 8 bytes
MAX_HASH_TABLE_SIZE = (1 << 32) - 1  # a bucket number is 32-bit
MAX_CHAIN_LENGTH = 64        # one candidate per lane of a wavefront


@dataclass(frozen=True)
class SlidingParams:
    """``HashBasedMatchFinder``'s five parameters and the coder's window size (0: no bound), with the reference's defaults"""

    hash_length: int = 4
    hash_table_size: int = 1000000
    max_chain_length: int = 64
    lazy: bool = True
    min_match_length: int = 4
    window_size: int = 1000000

    def _c(self):
        return (int(self.hash_length), int(self.hash_table_size), int(self.max_chain_length), int(bool(self.lazy)),
                int(self.min_match_length), int(self.window_size))


def sliding_seq_cap(block_len: int, min_match_length: int) -> int:
    """sequences a block can produce at most: every match covers at least ``min_match_length`` bytes, and the end of a
    block adds up to two literal-only sequences"""
    return int(block_len) // max(int(min_match_length), 1) + 2


def sliding_scratch_bytes(total_bytes: int, n_streams: int) -> int:
    return int(_lib.load().scl_lz77_sliding_scratch_bytes(int(total_bytes), int(n_streams)))


def sliding_kernel_names():
    """-> (index, parse, replay) kernel names of the sliding-window coder as a kernel trace prints them"""
    return _kernel_names("scl_lz77_sliding_kernel_names")


def sliding_bucket(gram, hash_table_size: int) -> int:
    """the bucket of a gram of 1..8 bytes: ``hash(tuple(gram)) % hash_table_size`` of a 64-bit CPython, computed by the
    function the kernels use.  Needs no device."""
    gram = np.ascontiguousarray(gram, np.uint8)
    if not 1 <= gram.size <= MAX_HASH_LENGTH or not 1 <= int(hash_table_size) <= MAX_HASH_TABLE_SIZE:
        raise ValueError("a gram of 1..8 bytes and 1 <= hash_table_size < 2^32")
    return int(_lib.load().scl_lz77_sliding_bucket_host(_lib.u8_ptr(gram), int(gram.size), int(hash_table_size)))


def sliding_parse_host(window: np.ndarray, start: int, params: SlidingParams = SlidingParams()):
    """``parse_host`` for the sliding-window coder (from ``sliding_wide_threshold()`` block bytes on: the wide path).
    window: uint8 array = history + block, the block starts at ``start``.
    -> (literal_count, match_length, match_offset: uint32 arrays; literals: uint8 array)"""
    _lib.load()
    hl, m, chain, lazy, mml, W = params._c()
    if not (0 <= hl < 1 << 32 and 0 <= m < 1 << 64 and 0 <= chain < 1 << 32 and 0 <= mml < 1 << 32 and 0 <= W < 1 << 32):
        raise ValueError("the sliding-window parameters are unsigned 32-bit integers (hash_table_size: 64-bit)")
    return _parse_host("scl_lz77_sliding_parse_host", window, start, lambda block: sliding_seq_cap(block, mml),
                       (hl, m, chain, lazy, mml, W), device_first=False)


def sliding_replay_host(history: np.ndarray, literal_count, match_length, match_offset, literals,
                        window_size: int = 0) -> np.ndarray:
    """``replay_host`` with the window's rules: a sequence with match length 0 copies nothing, and an offset beyond
    ``min(window_size, bytes so far)`` raises ``SclHipError`` (``window_size`` 0: no bound)."""
    return _replay_host("scl_lz77_sliding_replay_host", history, literal_count, match_length, match_offset, literals,
                        (int(window_size),))


def sliding_parse_batch(win, win_off, start, params: SlidingParams = SlidingParams(), seq_cap: Optional[int] = None,
                        scratch=None, stream=None, out: Optional[ParsedBatch] = None, phases: int = 0) -> ParsedBatch:
    """``parse_batch`` for the sliding-window coder: the same layout and the same :class:`ParsedBatch` (``encode_batch``
    takes it as it is).  ``seq_cap`` defaults to ``sliding_seq_cap`` of the longest block (one read-back of the block
    lengths); ``scratch``: a uint8 tensor of at least ``sliding_scratch_bytes(win.numel(), n_streams)`` bytes."""
    def fill(out, scratch, n_streams, total):
        hl, m, chain, lazy, mml, W = params._c()
        return _lib.Lz77SlidingParseArgs(win.data_ptr(), win_off.data_ptr(), start.data_ptr(), n_streams, total, m, hl,
                                         chain, lazy, mml, W, out.seq_cap, int(phases), 0, out.literal_count.data_ptr(),
                                         out.match_length.data_ptr(), out.match_offset.data_ptr(),
                                         out.literals.data_ptr(), out.n_seq.data_ptr(), out.n_lit.data_ptr(),
                                         out.status.data_ptr(), scratch.data_ptr(), int(scratch.numel()))

    if seq_cap is None:
        seq_cap = lambda longest: sliding_seq_cap(longest, params.min_match_length)  # noqa: E731
    return _parse_batch("scl_lz77_sliding_parse_batch", sliding_scratch_bytes, fill, win, win_off, start, seq_cap, scratch,
                        stream, out)


def sliding_replay_batch(win, win_off, have, literal_count, match_length, match_offset, n_seq, literals, lit_off, n_lit,
                         window_size: int = 0, stream=None):
    """``replay_batch`` with the window's rules (see :func:`sliding_replay_host`).  -> (out_len, status)"""
    return _replay_batch("scl_lz77_sliding_replay_batch", _lib.Lz77SlidingReplayArgs, window_size, win, win_off, have,
                         literal_count, match_length, match_offset, n_seq, literals, lit_off, n_lit, stream)


def sliding_compress_batch(win, win_off, start, params: SlidingParams = SlidingParams(), seq_cap: Optional[int] = None,
                           binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None, scratch=None,
                           stream=None):
    """``compress_batch`` for the sliding-window coder: parse + encode -> (:class:`EncodedBatch`, :class:`ParsedBatch`)"""
    seq_cap, out_stride = _default_caps(win_off, start, seq_cap, out_stride, binned_offset,
                                        lambda longest: sliding_seq_cap(longest, params.min_match_length))
    parsed = sliding_parse_batch(win, win_off, start, params, seq_cap, scratch=scratch, stream=stream)
    return encode_batch(parsed, binned_offset, out_stride, stream=stream), parsed


def sliding_decompress_batch(bits, bit_offset, nbits, win, win_off, have, seq_cap: int, window_size: int = 0,
                             binned_offset: int = DEFAULT_BINNED_OFFSET, stream=None):
    """``decompress_batch`` for the sliding-window coder: decode + windowed replay -> (out_len, status, consumed)"""
    replay = lambda *rows, stream: sliding_replay_batch(*rows, window_size, stream=stream)  # noqa: E731
    return _decompress_batch(replay, bits, bit_offset, nbits, win, win_off, have, seq_cap, binned_offset, stream)


# ---- sliding window, one large stream across the whole GPU (csrc/scl_lz77_sliding_wide.hip) -----------------------------------
def sliding_wide_shape():
    """-> (segment, cap): positions per speculated segment and the cap of a speculated right extension, compile-time"""
    segment, cap = C.c_uint32(0), C.c_uint32(0)
    _lib.load().scl_lz77_sliding_wide_shape(C.byref(segment), C.byref(cap))
    return segment.value, cap.value


def sliding_wide_threshold() -> int:
    """block bytes from which ``sliding_parse_host`` / ``sliding_replay_host`` take the wide path"""
    return int(_lib.load().scl_lz77_sliding_wide_threshold())


def sliding_wide_scratch_bytes(n: int) -> int:
    return int(_lib.load().scl_lz77_sliding_wide_scratch_bytes(int(n)))


def sliding_wide_kernel_names():
    """-> (speculate, walk, emit) kernel names as a kernel trace prints them"""
    return _kernel_names("scl_lz77_sliding_wide_kernel_names")


def sliding_parse_wide(win, start: int, params: SlidingParams = SlidingParams(), seq_cap: Optional[int] = None,
                       scratch=None, stream=None, out: Optional[ParsedBatch] = None, phases: int = 0) -> ParsedBatch:
    """``parse_wide`` for the sliding-window coder: ONE window whose block starts at ``start`` -> what
    ``sliding_parse_batch`` returns for a batch of this one stream.  ``seq_cap`` defaults to ``sliding_seq_cap`` of the
    block; ``scratch``: a uint8 tensor of at least ``sliding_wide_scratch_bytes(win.numel())`` bytes to reuse across calls;
    ``phases``: 0 = everything, else a mask of ``lib.LZ77_SLIDING_WIDE_INDEX`` / ``_SPECULATE`` / ``_WALK`` / ``_EMIT`` run
    on the same scratch (for measurements)."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous() and win.dim() == 1
    dev, n, start = win.device, int(win.numel()), int(start)
    hl, m, chain, lazy, mml, W = params._c()
    if out is not None:
        seq_cap = out.seq_cap
    if seq_cap is None:
        seq_cap = sliding_seq_cap(n - start, mml)
    need = sliding_wide_scratch_bytes(n)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    if out is None:
        out = _new_parsed(1, seq_cap, n, torch.full((1,), start, dtype=torch.int64, device=dev), dev)
    assert out.literal_count.shape == (1, out.seq_cap) and out.literals.numel() >= n
    a = _lib.Lz77SlidingWideParseArgs(win.data_ptr(), n, start, m, hl, chain, lazy, mml, W, out.seq_cap, int(phases), 0,
                                      out.literal_count.data_ptr(), out.match_length.data_ptr(),
                                      out.match_offset.data_ptr(), out.literals.data_ptr(), out.n_seq.data_ptr(),
                                      out.n_lit.data_ptr(), out.status.data_ptr(), scratch.data_ptr(), int(scratch.numel()))
    with torch.cuda.device(dev):
        rc = L.scl_lz77_sliding_parse_wide(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_sliding_parse_wide")
    out._scratch = scratch  # the kernels read it asynchronously: it lives as long as the result
    return out


def sliding_replay_wide(win, have: int, literal_count, match_length, match_offset, n_seq: int, literals, n_lit: int,
                        window_size: int = 0, cap=None, scratch=None, stream=None):
    """``replay_wide`` with the window's rules (see :func:`sliding_replay_host`).  ``scratch``: at least
    ``wide_replay_scratch_bytes(n_seq, cap - have)`` bytes.  -> (out_len, status): int32 [1] each."""
    import torch

    L = _lib.load()
    assert win.is_cuda and win.dtype == torch.uint8 and win.is_contiguous() and literals.dtype == torch.uint8
    rows = tuple(t.reshape(-1) for t in (literal_count, match_length, match_offset))
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= int(n_seq) for t in rows)
    assert literals.numel() >= int(n_lit)
    dev, have, cap = win.device, int(have), int(win.numel() if cap is None else cap)
    assert cap <= win.numel()
    need = wide_replay_scratch_bytes(n_seq, max(cap - have, 0))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    out_len = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _lib.Lz77SlidingWideReplayArgs(win.data_ptr(), have, cap, rows[0].data_ptr(), rows[1].data_ptr(),
                                       rows[2].data_ptr(), int(n_seq), literals.data_ptr(), int(n_lit), out_len.data_ptr(),
                                       status.data_ptr(), scratch.data_ptr(), int(scratch.numel()), int(window_size), 0)
    with torch.cuda.device(dev):
        rc = L.scl_lz77_sliding_replay_wide(C.byref(a), _stream_handle(stream, dev))
    _lib.check(rc, "scl_lz77_sliding_replay_wide")
    out_len._inputs = (rows, literals, scratch)  # read asynchronously: they live as long as the result
    return out_len, status


def sliding_compress_wide(win, start: int, params: SlidingParams = SlidingParams(), seq_cap: Optional[int] = None,
                          binned_offset: int = DEFAULT_BINNED_OFFSET, out_stride: Optional[int] = None, scratch=None,
                          stream=None, out: Optional[EncodedBatch] = None):
    """``sliding_parse_wide`` + ``encode_wide``: the bits of ``sliding_compress_batch`` for a batch of this one stream ->
    (:class:`EncodedBatch` of one slot, :class:`ParsedBatch`).  ``scratch`` serves both steps, one after the other."""
    parsed = sliding_parse_wide(win, start, params, seq_cap=seq_cap, scratch=scratch, stream=stream)
    return encode_wide(parsed, binned_offset, out_stride, lit_off=int(start), scratch=scratch, stream=stream, out=out), parsed


def sliding_decompress_wide(bits, bit_offset: int, nbits: int, win, have: int, seq_cap: int, window_size: int = 0,
                            binned_offset: int = DEFAULT_BINNED_OFFSET, scratch=None, stream=None):
    """``decode_wide`` + ``sliding_replay_wide``: appends the block to ``win``, which holds ``have`` bytes already.
    -> (out_len, status, consumed): status = the decoder's | the replay's."""
    lit_cap = max(int(win.numel()) - int(have), 0)
    decoded = decode_wide(bits, bit_offset, nbits, seq_cap, lit_cap, binned_offset, scratch=scratch, stream=stream)
    n_seq, n_lit = (int(x) & 0xFFFFFFFF for x in decoded._inputs[2][2:4].cpu().tolist())
    out_len, status = sliding_replay_wide(win, have, decoded.literal_count, decoded.match_length, decoded.match_offset, n_seq,
                                          decoded.literals, n_lit, window_size, stream=stream)
    return out_len, status | decoded.status, decoded.consumed
