"""The integer codes (Golomb, universal, Elias-delta) batched on the device, one lane per chunk (csrc/scl_uint.hip), against
the reference's goldens and the plain-Python restatement of tests/uint_batch_helpers.py: the bits, ``nbits``, the values and,
for damaged streams, the (values, consumed, status) of the sequential decoder -- all compared exactly, on both kernel forms.
Every buffer the kernels write lies between guard bands.  Sizes sit on the kernels' edges: a workgroup is 256 chunks, a wave
64; the tuned kernels read values 32 at a time (a 128-byte line) and the stream through a ring of 32 words, filled 16 words
(a half line) at a time; decoded values leave four at a time."""
import functools

import numpy as np
import pytest

from conftest import frame_blocks
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import EncodedBatch, UintCode, compact
from stanford_compression_library_amd.compressors import (GolombUintDecoder, GolombUintEncoder, UniversalUintDecoder,
                                                          UniversalUintEncoder)
from stanford_compression_library_amd.compressors.elias_delta_uint_coder import EliasDeltaUintDecoder, EliasDeltaUintEncoder
from stanford_compression_library_amd.core.data_block import DataBlock
from uint_batch_helpers import (BATCH_GOLDENS, CODES, ST_CAPACITY, ST_SIZE, ST_TRUNCATED, TOP, codeword_length,
                                decode_stream_wide, golden_bits, golden_code, stream_bits)
from uint_code_helpers import CODE_IDS, geometric, pack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL, FILL32 = 4096, 0xA5, 0xA5A5A5A5
FORMS = [False, True]  # any_parameter_kernels
FORM_IDS = ["tuned", "any"]
SOME_CODES = [("golomb", 10), ("universal", None), ("elias_delta", None)]
SOME_IDS = ["golomb10", "universal", "elias_delta"]
TUNED_PAIR = ("uint_encode_fast_kernel", "uint_decode_fast_kernel")
ANY_PAIR = ("uint_encode_kernel", "uint_decode_kernel")


def device():
    return torch.device("cuda:0")


class Arena:
    """buffers between guard bands (the pattern of test_gpu_uint_block.py)"""

    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes + 32 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.pos = GUARD
        self.used = []

    def take(self, nbytes, dtype=torch.uint8, align=256):
        start = (self.pos + align - 1) // align * align
        self.used.append((start, start + nbytes))
        self.pos = start + nbytes + GUARD
        assert self.pos + GUARD <= self.buf.numel()
        return self.buf[start:start + nbytes].view(dtype)

    def check(self, what):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for a, b in self.used:
            mask[a:b] = False
        bad = ((self.buf != FILL) & mask).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} guard bytes overwritten, first at arena offset {int(bad[0])}"


def exact_stride(nbits):
    """the smallest slot that holds a stream of ``nbits`` in whole words"""
    return max((int(nbits) + 127) // 128 * 16, 16)


def run_encode(code, rows, any_kernels, stride, what, shift=0):
    """the rows through ``encode_batch``, everything it writes between guard bands; ``shift``: the value rows start that
    many elements behind a 16-byte boundary -> (slots uint8 [n, stride], nbits uint32 [n], status [n], the value tensor)"""
    dev = device()
    n = len(rows)
    width = max((max(len(r) for r in rows) + 3) // 4 * 4, 4)
    arena = Arena(n * stride + 4 * n * width + 32 * n + 64, dev)
    flat = arena.take(4 * (n * width + 4), torch.int32)
    val = flat[shift: shift + n * width].view(n, width)
    host = np.full((n, width), FILL32, np.uint32)  # what lies behind a row's length is not a value
    for k, r in enumerate(rows):
        host[k, :len(r)] = r
    val.copy_(torch.from_numpy(host.view(np.int32)))
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    enc = EncodedBatch(arena.take(n * stride), stride, arena.take(8 * n, torch.int64), arena.take(4 * n, torch.int32),
                       arena.take(4 * n, torch.int32), n)
    code.encode_batch(val, lens=lens, out=enc, any_parameter_kernels=any_kernels)
    torch.cuda.synchronize()
    arena.check(what)
    assert enc.bit_offset.cpu().tolist() == [8 * stride * k for k in range(n)], what
    return (enc.data.cpu().numpy().reshape(n, stride), enc.nbits.cpu().numpy().view(np.uint32), enc.status.cpu().numpy(), val)


def want_slot(bits, stride):
    """a slot after its stream was stored: the stream, zero bits up to its last word, nothing behind that"""
    slot = np.full(stride, FILL, np.uint8)
    slot[: (bits.size + 31) // 32 * 4] = 0
    slot[: (bits.size + 7) // 8] = pack(bits)
    return slot


def check_encode(code, kind, M, rows, any_kernels, what, streams=None, stride=None, shift=0):
    streams = streams if streams is not None else [stream_bits(kind, M, r) for r in rows]
    stride = stride or max(exact_stride(b.size) for b in streams)
    slots, nbits, status, _ = run_encode(code, rows, any_kernels, stride, what, shift)
    assert nbits.tolist() == [b.size for b in streams], what
    assert not status.any(), what
    for k, bits in enumerate(streams):
        assert np.array_equal(slots[k], want_slot(bits, stride)), (what, k)
    return streams


def lay_streams(streams, lead_bits=0):
    """the streams (0/1 arrays) in one buffer of ones, each ``lead_bits`` behind a 16-byte boundary
    -> (bytes, a multiple of 16 of them; bit offsets)"""
    offs, parts, at = [], [], 0
    for bits in streams:
        body = pack(np.concatenate([np.ones(lead_bits, np.uint8), bits, np.ones((-(lead_bits + bits.size)) % 128, np.uint8)]))
        offs.append(8 * at + lead_bits)
        parts.append(body)
        at += body.size
    parts.append(np.full(16, 0xFF, np.uint8))
    return np.concatenate(parts), np.array(offs, np.int64)


def run_decode(code, data, offs, nbits, cap, any_kernels, what, in_shift=0, row_shift=0):
    """-> (values uint32 [n, row width] with what was not stored still FILL32, lens, consumed, status, the tensors)"""
    dev = device()
    n = len(offs)
    width = max((cap + 3) // 4 * 4, 4)
    arena = Arena(data.size + 4 * n * width + 64 * n + 128, dev)
    d_in = arena.take(data.size + 16)[in_shift: in_shift + data.size]
    d_in.copy_(torch.from_numpy(data))
    flat = arena.take(4 * (n * width + 4), torch.int32)
    val = flat[row_shift: row_shift + n * width].view(n, width)
    out = (val, arena.take(4 * n, torch.int32), arena.take(4 * n, torch.int32), arena.take(4 * n, torch.int32))
    d_offs = torch.from_numpy(np.asarray(offs, np.int64)).to(dev)
    d_nbits = torch.from_numpy(np.asarray(nbits, np.uint32).view(np.int32)).to(dev)
    code.decode_batch(d_in, d_offs, d_nbits, cap, out=out, any_parameter_kernels=any_kernels)
    torch.cuda.synchronize()
    arena.check(what)
    return (val.cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy(), val, d_in)


def check_decode(code, streams, nbits, wants, cap, any_kernels, what, lead_bits=0, in_shift=0, row_shift=0):
    """``wants``: (values, consumed, status) of every stream, from the restatement or the goldens"""
    data, offs = lay_streams(streams, lead_bits)
    val, lens, used, status, _, _ = run_decode(code, data, offs, nbits, cap, any_kernels, what, in_shift, row_shift)
    for k, (want, want_used, want_status) in enumerate(wants):
        assert (int(lens[k]), int(used[k]), int(status[k])) == (len(want), want_used, want_status), (what, k)
        assert np.array_equal(val[k, :len(want)], want), (what, k)
        assert (val[k, len(want):] == FILL32).all(), (what, k)  # nothing is stored past the count


def restated(kind, M, streams, nbits=None, cap=None):
    nbits = nbits if nbits is not None else [b.size for b in streams]
    return [decode_stream_wide(kind, M, b, nb, cap) for b, nb in zip(streams, nbits)]


# ---- the reference's bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_goldens(kind, M, any_kernels):
    cases = [c for c in BATCH_GOLDENS if golden_code(c) == (kind, M)]
    assert any(c.group == "wide" for c in cases) and any(c.group == "past_limit" for c in cases)
    code = UintCode(kind, M)
    rows = [c.arr("values").astype(np.uint32) for c in cases]
    streams = [golden_bits(c) for c in cases]
    check_encode(code, kind, M, rows, any_kernels, "goldens", streams=streams)
    wants = [(r, c.nbits, 0) for r, c in zip(rows, cases)]
    check_decode(code, streams, [c.nbits for c in cases], wants, max(len(r) for r in rows), any_kernels, "goldens")


# ---- ragged batches ---------------------------------------------------------------------------------------------------------
LENS = (0, 1, 31, 32, 33, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def ragged(kind, M, n_chunks):
    """chunks of the lengths above, geometric values around the code's scale, one in eight -- in every fourth chunk all -- of up
    to 32 bits (Golomb: of a run up to 600 ones): the longest streams pass a line, the ring and 4096 bits"""
    rng = np.random.default_rng(n_chunks)
    lens = [LENS[(k * 5 + 7) % 8] for k in range(n_chunks)]
    rows = []
    for k, n in enumerate(lens):
        v = geometric(n, mean=8.0 * (M or 1), seed=1000 * n_chunks + k).astype(np.int64)
        wide = rng.random(n) < (1.0 if k % 4 == 0 else 0.125)
        v[wide] = rng.integers(0, 600 * M, int(wide.sum())) if kind == "golomb" else rng.integers(1 << 16, 1 << 32, int(wide.sum()))
        rows.append(v.astype(np.uint32))
    streams = [stream_bits(kind, M, r) for r in rows]
    return rows, streams, restated(kind, M, streams)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n_chunks", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_ragged_batches(kind, M, n_chunks, any_kernels):
    rows, streams, wants = ragged(kind, M, n_chunks)
    assert max(b.size for b in streams) > 4096
    code = UintCode(kind, M)
    what = f"ragged {n_chunks}"
    check_encode(code, kind, M, rows, any_kernels, what, streams=streams)
    for (got, used, status), r, b in zip(wants, rows, streams):
        assert (got.tolist(), used, status) == (r.tolist(), b.size, 0)
    check_decode(code, streams, [b.size for b in streams], wants, 129, any_kernels, what, lead_bits=(n_chunks % 3) * 13)


# ---- long runs: the flush and refill contracts, the line boundary -----------------------------------------------------------
def reach(M, p):
    """short values whose codewords take exactly p bits (M = 1: one bit each; M = 3: 0 takes two bits, 1 three)"""
    if M == 1:
        return [0] * p
    return [] if p == 0 else [0] * ((p - 3) // 2) + [1]


@functools.lru_cache(maxsize=None)
def long_runs(M):
    rows = []
    for run in (31, 32, 33, 511, 512, 513, 2100):
        for p in (0, 31, 1023):
            for behind in ([], [0, 1, 2, 0, 5, 0, 0, 1]):
                rows.append(np.array(reach(M, p) + [run * M] + behind, np.uint32))
    streams = [stream_bits("golomb", M, r) for r in rows]
    for r, b in zip(rows, streams):  # the run starts where it is meant to
        p = b.size - int(sum(codeword_length("golomb", M, int(x)) for x in r[np.flatnonzero(r >= 31 * M)[0]:]))
        assert p in (0, 31, 1023) and b[p: p + 31].all()
    return rows, streams, restated("golomb", M, streams)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("M", [1, 3])
def test_long_golomb_runs(M, any_kernels):
    rows, streams, wants = long_runs(M)
    code = UintCode("golomb", M)
    check_encode(code, "golomb", M, rows, any_kernels, "long runs", streams=streams)
    for (got, used, status), r, b in zip(wants, rows, streams):
        assert (got.tolist(), used, status) == (r.tolist(), b.size, 0)
    cap = max(len(r) for r in rows)
    for lead in (0, 7):
        check_decode(code, streams, [b.size for b in streams], wants, cap, any_kernels, f"long runs +{lead}", lead_bits=lead)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
def test_129_universal_codewords_of_64_bits(any_kernels):
    """two words a value, every value: 8256 bits, past two rings"""
    rng = np.random.default_rng(64)
    rows = [rng.integers(1 << 31, 1 << 32, n).astype(np.uint32) for n in (129, 5, 129, 0, 128)]
    rows[0][:3] = (1 << 31, TOP, TOP - 1)
    code = UintCode("universal")
    streams = check_encode(code, "universal", None, rows, any_kernels, "64-bit codewords")
    assert streams[0].size == 129 * 64
    wants = [(r, b.size, 0) for r, b in zip(rows, streams)]
    check_decode(code, streams, [b.size for b in streams], wants, 129, any_kernels, "64-bit codewords", lead_bits=3)


# ---- slots ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_slots_of_exactly_slot_bytes(kind, M, any_kernels):
    code = UintCode(kind, M)
    top = 300 * M if kind == "golomb" else TOP
    rows = [np.full(100, top, np.uint32) if k % 7 == 0 else np.random.default_rng(k).integers(0, top + 1, 100).astype(np.uint32)
            for k in range(65)]
    stride = code.slot_bytes(100, top)
    assert stride == ((100 * codeword_length(kind, M, top) + 7) // 8 + 4 + 127) // 128 * 128
    check_encode(code, kind, M, rows, any_kernels, "slot_bytes", stride=stride)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_slots_16_bytes_short(kind, M, any_kernels):
    """the chunks that need the last 16 bytes report SCL_ST_CAPACITY and the length they need; the others, and the guards,
    are as if nothing had happened"""
    code = UintCode(kind, M)
    rows, _, _ = ragged(kind, M, 65)
    streams = [stream_bits(kind, M, r) for r in rows]
    need = [exact_stride(b.size) for b in streams]
    stride = max(need) - 16
    assert stride >= 16 and 1 <= sum(n > stride for n in need) < len(rows)
    slots, nbits, status, _ = run_encode(code, rows, any_kernels, stride, "short slots")
    assert nbits.tolist() == [b.size for b in streams]
    assert status.tolist() == [ST_CAPACITY if n > stride else 0 for n in need]
    for k, bits in enumerate(streams):
        if need[k] <= stride:
            assert np.array_equal(slots[k], want_slot(bits, stride)), k


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
def test_a_run_no_slot_holds_ends_at_once(any_kernels):
    """x = 4 * 10^9 with M = 1 is four thousand million ones: the lane stops emitting when its 128 bytes are full and only
    adds lengths, which saturate at 2^32 - 1"""
    code = UintCode("golomb", 1)
    rows = [np.array([5], np.uint32), np.array([4_000_000_000], np.uint32), np.array([3, 4_000_000_000, 4_000_000_000, 1], np.uint32),
            np.array([6], np.uint32)]
    slots, nbits, status, _ = run_encode(code, rows, any_kernels, 128, "a run no slot holds")
    assert nbits.tolist() == [6, 4_000_000_001, TOP, 7]
    assert status.tolist() == [0, ST_CAPACITY, ST_CAPACITY, 0]
    for k in (0, 3):
        assert np.array_equal(slots[k], want_slot(stream_bits("golomb", 1, rows[k]), 128))


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_out_cap_below_the_count(kind, M, any_kernels):
    rows, streams, _ = ragged(kind, M, 64)
    for cap in (1, 30, 32, 127):
        wants = restated(kind, M, streams, cap=cap)
        assert any(w[2] == ST_CAPACITY for w in wants) and any(w[2] == 0 for w in wants)
        check_decode(UintCode(kind, M), streams, [b.size for b in streams], wants, cap, any_kernels, f"out_cap {cap}")


# ---- alignment --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_unaligned_rows_run_the_any_parameter_pair(kind, M, any_kernels):
    rows, streams, wants = ragged(kind, M, 65)
    code = UintCode(kind, M)
    stride = max(exact_stride(b.size) for b in streams)
    slots, nbits, status, val = run_encode(code, rows, any_kernels, stride, "unaligned value rows", shift=1)
    assert val.data_ptr() % 16 == 4 and nbits.tolist() == [b.size for b in streams] and not status.any()
    for k, bits in enumerate(streams):
        assert np.array_equal(slots[k], want_slot(bits, stride)), k
    assert code.kernel_names(65, values=val)[0] == ANY_PAIR[0]
    data, offs = lay_streams(streams, 5)
    for in_shift, row_shift in ((4, 0), (0, 1), (4, 3)):
        val, lens, used, st, out_rows, d_in = run_decode(code, data, offs, [b.size for b in streams], 129, any_kernels,
                                                         "unaligned decode", in_shift, row_shift)
        assert d_in.data_ptr() % 16 == in_shift and out_rows.data_ptr() % 16 == 4 * row_shift
        for k, (want, want_used, want_status) in enumerate(wants):
            assert (int(lens[k]), int(used[k]), int(st[k])) == (len(want), want_used, want_status), k
            assert np.array_equal(val[k, :len(want)], want) and (val[k, len(want):] == FILL32).all(), k
        assert code.kernel_names(65, values=out_rows, data=d_in)[1] == ANY_PAIR[1]
    # rows the tuned kernels take: the pair follows the thread's switch
    _, _, _, val = run_encode(code, rows, any_kernels, stride, "aligned value rows")
    assert code.kernel_names(65, values=val, any_parameter_kernels=any_kernels) == (ANY_PAIR if any_kernels else TUNED_PAIR)


# ---- damaged streams --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damaged(kind, M):
    """every cut of a 40-codeword stream, 200 single-bit flips of it, 64 runs of random bytes, 64 zeros, 64 ones
    -> (streams, the bits of each that belong to it, the restatement's verdicts)"""
    rng = np.random.default_rng(M or 77)
    v = geometric(40, mean=8.0 * (M or 1), seed=40).astype(np.int64)
    v[[7, 23]] = (35 * M, 70 * M + M - 1) if kind == "golomb" else (TOP, 1 << 31)
    whole = stream_bits(kind, M, v)
    streams, nbits = [whole] * (whole.size + 1), list(range(whole.size + 1))
    for at in rng.integers(0, whole.size, 200):
        flipped = whole.copy()
        flipped[at] ^= 1
        streams.append(flipped)
        nbits.append(whole.size)
    for k in range(64):
        streams.append(np.unpackbits(rng.integers(0, 256, 64).astype(np.uint8)))
        nbits.append(512 - (k % 9))
    for bit in (0, 1):  # nothing but a run: 32 ones, six zeros
        streams.append(np.full(64, bit, np.uint8))
        nbits.append(64)
    return streams, nbits, restated(kind, M, streams, nbits)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_damaged_streams(kind, M, any_kernels):
    streams, nbits, wants = damaged(kind, M)
    met = {w[2] for w in wants}
    assert {0, ST_TRUNCATED} <= met and (ST_SIZE in met or kind == "golomb")  # (a Golomb run of 2^32 / M ones fits no test)
    cap = max(len(w[0]) for w in wants) + 1
    check_decode(UintCode(kind, M), streams, nbits, wants, cap, any_kernels, "damaged", lead_bits=9)


@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
def test_golomb_streams_that_announce_2_32(any_kernels):
    """SCL_ST_SIZE of the Golomb code: ones up to a quotient q with M * q >= 2^32, and a remainder that carries M * q over"""
    M = 3 << 18  # 2^32 - 1 = 5461 * M + 2^18 - 1, the last short remainder
    top = stream_bits("golomb", M, [7, TOP])
    past = np.concatenate([stream_bits("golomb", M, [7]), np.ones(5461, np.uint8), stream_bits("golomb", M, [1 << 18])])
    streams = [top, past, np.ones(6000, np.uint8), np.concatenate([stream_bits("golomb", M, [9, 9]), np.ones(5461, np.uint8)])]
    wants = restated("golomb", M, streams)
    assert [w[2] for w in wants] == [0, ST_SIZE, ST_SIZE, ST_TRUNCATED] and wants[0][0].tolist() == [7, TOP]
    check_decode(UintCode("golomb", M), streams, [b.size for b in streams], wants, 4, any_kernels, "announcing", lead_bits=21)


# ---- compaction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_kernels", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind,M", SOME_CODES, ids=SOME_IDS)
def test_compaction_takes_the_batch(kind, M, any_kernels):
    rows, streams, _ = ragged(kind, M, 65)
    assert any(b.size == 0 for b in streams)
    dev = device()
    width = 132
    host = np.zeros((65, width), np.uint32)
    for k, r in enumerate(rows):
        host[k, :len(r)] = r
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    code = UintCode(kind, M)
    enc = code.encode_batch(torch.from_numpy(host.view(np.int32)).to(dev), lens=lens,
                            out_stride=max(exact_stride(b.size) for b in streams), any_parameter_kernels=any_kernels)
    packed = [pack(b) for b in streams]
    dense, offs = compact(enc)
    assert offs.cpu().tolist() == np.cumsum([0] + [p.size for p in packed]).tolist()
    assert np.array_equal(dense[: int(offs[-1])].cpu().numpy(), np.concatenate(packed))
    framed, foffs = compact(enc, framed=True)
    want = frame_blocks([(p, b.size) for p, b in zip(packed, streams)])
    assert int(foffs[-1]) == want.size and np.array_equal(framed[: want.size].cpu().numpy(), want)
    val, out_lens, used, status = code.decode_encoded(enc, 129, any_parameter_kernels=any_kernels)
    assert out_lens.cpu().tolist() == [len(r) for r in rows] and not status.any().item()
    assert used.cpu().tolist() == [b.size for b in streams]
    got = val.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(got[k, :len(r)], r) for k, r in enumerate(rows))


# ---- the classes ------------------------------------------------------------------------------------------------------------
CLASSES = [("golomb", 10), ("golomb", 1 << 31), ("universal", None), ("elias_delta", None)]


def coders(kind, M):
    if kind == "golomb":
        return GolombUintEncoder(M), GolombUintDecoder(M)
    if kind == "universal":
        return UniversalUintEncoder(), UniversalUintDecoder()
    return EliasDeltaUintEncoder(), EliasDeltaUintDecoder()


def mixed_blocks(kind, M):
    scale = 8.0 * min(M or 1, 1000)
    big = 40 * M if kind == "golomb" else TOP
    return [DataBlock([]), DataBlock(geometric(17, scale, 1).tolist()), DataBlock([0]), DataBlock([3, big, 0, big - 1]),
            DataBlock(geometric(5000, scale, 2).tolist()), DataBlock([]), DataBlock([1, (1 << 32) + 5, 2]),
            DataBlock(geometric(129, scale, 3).tolist()), DataBlock([np.int64(4), np.uint8(200), 7])]


@pytest.mark.parametrize("kind,M", CLASSES, ids=[f"{k}{M or ''}" for k, M in CLASSES])
def test_encode_blocks_and_decode_blocks_equal_the_loops(kind, M):
    enc, dec = coders(kind, M)
    blocks = mixed_blocks(kind, M)
    want = [enc.encode_block(b) for b in blocks]
    got = enc.encode_blocks(blocks)
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want))
    assert enc.encode_blocks([]) == [] and dec.decode_blocks([]) == []
    loop = [dec.decode_block(b) for b in want]
    batch = dec.decode_blocks(want)
    assert [(b.data_list, used) for b, used in batch] == [(b.data_list, used) for b, used in loop]
    assert [b.data_list for b, _ in batch] == [[int(x) for x in b.data_list] for b in blocks]


@pytest.mark.parametrize("kind,M", CLASSES, ids=[f"{k}{M or ''}" for k, M in CLASSES])
def test_a_block_the_loop_refuses_is_refused_alike(kind, M):
    enc, dec = coders(kind, M)
    blocks = [DataBlock([1, 2, 3]), DataBlock([4]), DataBlock([1.5, 2.0]), DataBlock([-1])]
    with pytest.raises(Exception) as loop:
        [enc.encode_block(b) for b in blocks]
    with pytest.raises(type(loop.value)) as batch:
        enc.encode_blocks(blocks)
    assert str(batch.value) == str(loop.value)
    assert enc.encode_blocks(blocks[:2]) == [enc.encode_block(b) for b in blocks[:2]]
    # a stream that ends inside a codeword: the first such block is named
    streams = [enc.encode_block(DataBlock([5, 6, 7 * (M or 1) + 3])) for _ in range(4)]
    if M != 1 << 31:  # (the host decodes that M, and reports a cut its own way)
        cut = [streams[0], streams[1][:-1], streams[2], streams[3][:-1]]
        with pytest.raises(backend_lib.SclHipError, match=r"decode_blocks: block 1: .*TRUNCATED"):
            dec.decode_blocks(cut)
