"""The fixed-width kernels (csrc/scl_fixed.hip) against the numpy restatement of tests/fixed_width_helpers.py, byte for byte,
and the classes built on them against the reference's goldens.  Every buffer the kernels write is filled with a sentinel
first and lies between guard bands: what a stream does not own must come back unchanged.  Sizes sit on the kernels' edges:
a lane packs 32 symbols, a workgroup ``FixedWidthCode.TILE``."""
import numpy as np
import pytest

from conftest import golden_ids, load_golden
from fixed_width_helpers import embed, golden_symbols, pack, pack_bits, unpack
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import EncodedBatch, FixedWidthCode, compact
from stanford_compression_library_amd.compressors import fixed_bitwidth_compressor as fbc
from stanford_compression_library_amd.compressors.fano_coder import FanoDecoder, FanoEncoder
from stanford_compression_library_amd.compressors.shannon_coder import ShannonDecoder, ShannonEncoder
from stanford_compression_library_amd.compressors.shannon_fano_elias_coder import (ShannonFanoEliasDecoder,
                                                                                   ShannonFanoEliasEncoder)
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist
from stanford_compression_library_amd.utils.bitarray_utils import BitArray
from stanford_compression_library_amd.utils.test_utils import try_file_lossless_compression

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = FixedWidthCode.TILE
GUARD, FILL = 4096, 0xA5
ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED = backend_lib.ST_CAPACITY, backend_lib.ST_SYMBOL, backend_lib.ST_TRUNCATED
LENGTHS = (0, 1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
NP_SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32}
FIXED = load_golden("fixed_bitwidth")
FAMILY = load_golden("shannon_family")
BLOCKS = [c for c in FIXED if c.kind == "block" and "raises" not in c.meta]
FAMILY_BLOCKS = [c for c in FAMILY if c.kind == "block"]


def device():
    return torch.device("cuda:0")


def torch_sym(sym_bytes):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32}[sym_bytes]


class Arena:
    """buffers between guard bands, everything pre-filled with the sentinel"""

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


def fill_value(sym_bytes):
    return int.from_bytes(bytes([FILL]) * sym_bytes, "little")


def run_encode(rows, widths, Ks, sym_bytes, stride=None, what=""):
    """index rows through ``encode_batch`` -> (slots uint8 [n, stride], nbits uint32 [n], status [n], EncodedBatch)"""
    dev, code = device(), FixedWidthCode()
    n = len(rows)
    per16 = 16 // sym_bytes
    cols = max((max(len(r) for r in rows) + per16 - 1) // per16 * per16, per16)
    stride = stride or max(code.slot_bytes(len(r), w) for r, w in zip(rows, widths))
    arena = Arena(n * stride + sym_bytes * n * cols + 32 * n + 64, dev)
    host = np.full((n, cols), fill_value(sym_bytes), NP_SYM[sym_bytes])  # what lies behind a row's length is not a symbol
    for k, r in enumerate(rows):
        host[k, :len(r)] = r
    sym = arena.take(sym_bytes * n * cols, torch_sym(sym_bytes)).view(n, cols)
    sym.copy_(torch.from_numpy(host.view({1: np.uint8, 2: np.int16, 4: np.int32}[sym_bytes])))
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    enc = EncodedBatch(arena.take(n * stride), stride, arena.take(8 * n, torch.int64), arena.take(4 * n, torch.int32),
                       arena.take(4 * n, torch.int32), n)
    code.encode_batch(sym, lens, widths, Ks, out=enc)
    torch.cuda.synchronize()
    arena.check(what)
    assert enc.bit_offset.cpu().tolist() == [8 * stride * k for k in range(n)], what
    return enc.data.cpu().numpy().reshape(n, stride), enc.nbits.cpu().numpy().view(np.uint32), enc.status.cpu().numpy(), enc


def want_slot(idx, width, stride):
    """a slot as the kernel must leave it: the stream, zero bits up to its last whole word, the sentinel behind"""
    packed, nbits = pack(idx, width)
    slot = np.full(stride, FILL, np.uint8)
    slot[: (nbits + 31) // 32 * 4] = 0
    slot[: packed.size] = packed
    return slot, nbits


def run_decode(data, offs, nbits, lens, widths, Ks, cap, sym_bytes, what=""):
    """-> (rows [n, cols] with the sentinel where nothing was stored, lens, consumed, status)"""
    dev, code = device(), FixedWidthCode()
    n = len(offs)
    per16 = 16 // sym_bytes
    cols = max((cap + per16 - 1) // per16 * per16, per16)
    arena = Arena(sym_bytes * n * cols + 16 * n + 64, dev)
    out = (arena.take(sym_bytes * n * cols, torch_sym(sym_bytes)).view(n, cols), arena.take(4 * n, torch.int32),
           arena.take(4 * n, torch.int32), arena.take(4 * n, torch.int32))
    t = lambda a, d: torch.from_numpy(np.asarray(a, d)).to(dev)  # noqa: E731
    code.decode_batch(data, t(offs, np.int64), t(np.asarray(nbits, np.uint32).view(np.int32), np.int32),
                      t(lens, np.int32) if lens is not None else None, widths, Ks, cap, out=out)
    torch.cuda.synchronize()
    arena.check(what)
    val = out[0].cpu().numpy().view(NP_SYM[sym_bytes])
    return val, out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()


def check_rows(val, rows, sym_bytes, what=""):
    for k, r in enumerate(rows):
        assert np.array_equal(val[k, :len(r)], np.asarray(r, val.dtype)), f"{what}: row {k}"
        assert (val[k, len(r):] == fill_value(sym_bytes)).all(), f"{what}: row {k}: stored past its length"


# ---- widths and lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym_bytes", [1, 2, 4])
def test_every_width_and_length(sym_bytes):
    rng = np.random.default_rng(sym_bytes)
    rows, widths, Ks = [], [], []
    for w in range(1, 8 * sym_bytes + 1):
        for K in ((1 << w), max((1 << w) - (1 << w) // 3 - 1, 1)):  # the full alphabet, and one that is no power of two
            for n in LENGTHS:
                rows.append(rng.integers(0, K, n, dtype=np.uint64))
                widths.append(w)
                Ks.append(K)
    slots, nbits, status, enc = run_encode(rows, widths, Ks, sym_bytes, what="encode")
    assert not status.any()
    for k, (r, w) in enumerate(zip(rows, widths)):
        want, nb = want_slot(r, w, enc.stride)
        assert nbits[k] == nb == len(r) * w
        assert np.array_equal(slots[k], want), f"stream {k}: width {w}, {len(r)} symbols"
    cap = max(len(r) for r in rows)
    val, lens, used, status = run_decode(enc.data, enc.bit_offset.cpu().numpy(), nbits, [len(r) for r in rows], widths, Ks,
                                         cap, sym_bytes, what="decode")
    assert not status.any()
    assert lens.tolist() == [len(r) for r in rows] and used.view(np.uint32).tolist() == nbits.tolist()
    check_rows(val, rows, sym_bytes)
    dense, offs = compact(enc)  # the EncodedBatch goes through compact() as any other
    dense, offs = dense.cpu().numpy(), offs.cpu().numpy()
    for k in (0, len(rows) // 2, len(rows) - 1):
        packed, _ = pack(rows[k], widths[k])
        assert np.array_equal(dense[offs[k]: offs[k] + packed.size], packed)


# ---- decode at any bit offset -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym_bytes,widths", [(1, (1, 3, 8)), (2, (9, 13, 16)), (4, (17, 31, 32))])
def test_decode_bit_offsets(sym_bytes, widths):
    rng = np.random.default_rng(17)
    rows, ws, offs, nbits, parts, at = [], [], [], [], [], 0
    for w in widths:
        for off in (0, 1, 7, 8, 13, 31, 127):
            for n in (33, TILE + 33):
                r = rng.integers(0, 1 << w, n, dtype=np.uint64)
                nbytes = ((off + n * w + 7) // 8 + 15) // 16 * 16 + 16  # garbage in front of and behind the stream
                parts.append(embed(pack_bits(r, w), off, nbytes, rng))
                rows.append(r), ws.append(w), offs.append(8 * at + off), nbits.append(n * w)
                at += nbytes
    # the last stream ends with the buffer, which is no whole number of 16-byte pieces
    w, n = widths[-1], 77
    r = rng.integers(0, 1 << w, n, dtype=np.uint64)
    tail = embed(pack_bits(r, w), 5, (5 + n * w + 7) // 8, rng)
    if (at + tail.size) % 16 == 0:
        tail = tail[:-1]
    parts.append(tail), rows.append(r), ws.append(w), offs.append(8 * at + 5)
    nbits.append(min(n * w, 8 * tail.size - 5))
    buf = np.concatenate(parts)
    arena = Arena(buf.size, device())  # the guard band behind the buffer is not the stream's to read: poison, not zeros
    data = arena.take(buf.size)
    data.copy_(torch.from_numpy(buf))
    val, lens, used, status = run_decode(data, offs, nbits, [len(r) for r in rows], ws, [1 << w for w in ws],
                                         max(len(r) for r in rows), sym_bytes)
    whole = [min(len(r), nb // w) for r, nb, w in zip(rows, nbits, ws)]
    assert lens.tolist() == whole and used.tolist() == [c * w for c, w in zip(whole, ws)]
    assert status.tolist() == [0 if c == len(r) else ST_TRUNCATED for c, r in zip(whole, rows)]
    check_rows(val, [r[:c] for r, c in zip(rows, whole)], sym_bytes)


# ---- ragged batches against single calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 3, 255, 257])
def test_ragged_batch_equals_single_calls(n_streams):
    rng = np.random.default_rng(n_streams)
    code = FixedWidthCode()
    widths = rng.integers(1, 17, n_streams).tolist()
    lens = rng.choice([0, 0, 1, 31, 32, 33, 100, 1000, TILE, TILE + 5], n_streams).tolist()
    if n_streams > 1:
        lens[1] = 0
    Ks = [int(rng.integers(1, (1 << w) + 1)) for w in widths]
    rows = [rng.integers(0, K, n, dtype=np.uint64) for K, n in zip(Ks, lens)]
    slots, nbits, status, enc = run_encode(rows, widths, Ks, 2)
    assert not status.any()
    singles = [code.encode_host(r, w, K) for r, w, K in zip(rows, widths, Ks)]
    for k, (packed, nb, st) in enumerate(singles):
        assert st == 0 and nb == nbits[k]
        assert np.array_equal(slots[k, :packed.size], packed)
    val, got, used, status = run_decode(enc.data, enc.bit_offset.cpu().numpy(), nbits, lens, widths, Ks, max(max(lens), 1), 2)
    assert not status.any()
    check_rows(val, rows, 2)
    for k, (packed, nb, _) in enumerate(singles):
        idx, consumed, st = code.decode_host(packed, 0, nb, lens[k], widths[k], Ks[k])
        assert st == 0 and consumed == nb == used[k] and np.array_equal(idx, rows[k])


# ---- sentinels ------------------------------------------------------------------------------------------------------------------------
def test_a_stream_that_fills_its_slot_exactly():
    rng = np.random.default_rng(3)
    rows = [rng.integers(0, 256, n, dtype=np.uint64) for n in (5, 128, 0, 127)]  # 128 symbols of 8 bits = the slot
    slots, nbits, status, enc = run_encode(rows, [8] * 4, [256] * 4, 1, stride=128)
    assert not status.any() and nbits.tolist() == [40, 1024, 0, 1016]
    for k, r in enumerate(rows):
        assert np.array_equal(slots[k], want_slot(r, 8, 128)[0]), k
    assert (slots[0, 8:] == FILL).all() and (slots[2] == FILL).all() and (slots[3, 127] == 0)


# ---- statuses, each alone, the neighbours untouched -----------------------------------------------------------------------------------
def test_encode_statuses():
    rng = np.random.default_rng(5)
    good = rng.integers(0, 5, 100, dtype=np.uint64)
    bad = good.copy()
    bad[[7, 64]] = [5, 7]  # indices >= K = 5: coded as 0
    as_zero = bad.copy()
    as_zero[[7, 64]] = 0
    slots, nbits, status, enc = run_encode([good, bad, good], [3] * 3, [5] * 3, 1)
    assert status.tolist() == [0, ST_SYMBOL, 0] and nbits.tolist() == [300] * 3
    assert np.array_equal(slots[1], want_slot(as_zero, 3, enc.stride)[0])
    assert np.array_equal(slots[0], slots[2]) and np.array_equal(slots[0], want_slot(good, 3, enc.stride)[0])
    # a slot of 16 bytes: 42 symbols of 3 bits fit (126 bits), 43 do not -- nothing is stored, nbits still reports n * w
    rows = [rng.integers(0, 8, n, dtype=np.uint64) for n in (42, 43, TILE + 1, 42)]
    slots, nbits, status, enc = run_encode(rows, [3] * 4, [8] * 4, 1, stride=16)
    assert status.tolist() == [0, ST_CAPACITY, ST_CAPACITY, 0]
    assert nbits.tolist() == [126, 129, 3 * (TILE + 1), 126]
    assert (slots[1] == FILL).all() and (slots[2] == FILL).all()
    for k in (0, 3):
        assert np.array_equal(slots[k], want_slot(rows[k], 3, 16)[0])


def test_decode_statuses():
    rng = np.random.default_rng(6)
    w, K, n = 5, 20, 200
    r = rng.integers(0, K, n, dtype=np.uint64)
    packed, nb = pack(r, w)
    piece = (packed.size + 15) // 16 * 16
    buf = np.zeros(3 * piece, np.uint8)
    for k in range(3):
        buf[k * piece: k * piece + packed.size] = packed
    offs = [8 * k * piece for k in range(3)]
    data = torch.from_numpy(buf).to(device())
    # truncated: the stream ends inside symbol 150; the 150 whole symbols in front are delivered
    val, lens, used, status = run_decode(data, offs, [nb, 150 * w + 3, nb], [n] * 3, [w] * 3, [K] * 3, n, 1)
    assert status.tolist() == [0, ST_TRUNCATED, 0] and lens.tolist() == [n, 150, n] and used.tolist() == [nb, 150 * w, nb]
    check_rows(val, [r, r[:150], r], 1)
    # capacity: more symbols than a row holds; nothing is stored past out_cap
    val, lens, used, status = run_decode(data, offs, [nb] * 3, [64, n, 64], [w] * 3, [K] * 3, 64, 1)
    assert status.tolist() == [0, ST_CAPACITY, 0] and lens.tolist() == [64] * 3 and used.tolist() == [64 * w] * 3
    check_rows(val, [r[:64]] * 3, 1)
    # symbol: an index >= K comes back as 0
    hurt = r.copy()
    hurt[[3, 199]] = [K, 31]
    buf2 = buf.copy()
    buf2[piece: piece + packed.size] = pack(hurt, w)[0]
    hurt[[3, 199]] = 0
    val, lens, used, status = run_decode(torch.from_numpy(buf2).to(device()), offs, [nb] * 3, [n] * 3, [w] * 3, [K] * 3, n, 1)
    assert status.tolist() == [0, ST_SYMBOL, 0] and lens.tolist() == [n] * 3
    check_rows(val, [r, hurt, r], 1)
    # a stream that claims bits behind the buffer's end is truncated there, and nothing behind the end is read
    val, lens, used, status = run_decode(data[: 2 * piece + 20], offs, [nb] * 3, [n] * 3, [w] * 3, [K] * 3, n, 1)
    assert status.tolist() == [0, 0, ST_TRUNCATED] and lens.tolist() == [n, n, 20 * 8 // w]
    check_rows(val, [r, r, r[: 20 * 8 // w]], 1)


# ---- buffers of a larger batch reused for a smaller one -------------------------------------------------------------------------------
def test_buffers_reused_for_a_smaller_batch():
    rng = np.random.default_rng(8)
    dev, code = device(), FixedWidthCode()
    big = [rng.integers(0, 1 << 11, n, dtype=np.uint64) for n in (TILE + 9, 500, 77, 0, 2 * TILE)]
    small = [rng.integers(0, 1 << 4, n, dtype=np.uint64) for n in (600, 3)]

    def rows_tensor(rows, cols):
        host = np.zeros((len(rows), cols), np.uint16)
        for k, r in enumerate(rows):
            host[k, :len(r)] = r
        return torch.from_numpy(host.view(np.int16)).to(dev)

    cols = 2 * TILE
    enc = code.alloc_encoded(5, cols, dev, width=11)
    lens = lambda rows: torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)  # noqa: E731
    code.encode_batch(rows_tensor(big, cols), lens(big), 11, 1 << 11, out=enc)
    before = enc.data.clone()
    part = EncodedBatch(enc.data, enc.stride, enc.bit_offset[:2], enc.nbits[:2], enc.status[:2], 2)
    code.encode_batch(rows_tensor(small, cols), lens(small), 4, 1 << 4, out=part)
    torch.cuda.synchronize()
    assert part.nbits.tolist() == [2400, 12] and part.status.tolist() == [0, 0]
    assert enc.nbits.tolist()[2:] == [77 * 11, 0, 2 * TILE * 11]
    after = enc.data.cpu().numpy()
    for k, r in enumerate(small):
        packed, nb = pack(r, 4)
        stored = (nb + 31) // 32 * 4
        slot = after[k * enc.stride: (k + 1) * enc.stride]
        assert np.array_equal(slot[:packed.size], packed) and not slot[packed.size:stored].any()
        assert np.array_equal(slot[stored:], before[k * enc.stride + stored: (k + 1) * enc.stride].cpu().numpy())
    assert np.array_equal(after[2 * enc.stride:], before[2 * enc.stride:].cpu().numpy())
    out = code.alloc_decoded(5, cols, dev, torch.int16)
    code.decode_batch(enc.data, enc.bit_offset, enc.nbits, lens(big), 11, 1 << 11, cols, out=out)
    val, got, _, status = code.decode_batch(part.data, part.bit_offset, part.nbits, lens(small), 4, 1 << 4, cols,
                                            out=(out[0][:2], out[1][:2], out[2][:2], out[3][:2]))
    assert got.tolist() == [600, 3] and status.tolist() == [0, 0]
    for k, r in enumerate(small):
        assert np.array_equal(val[k, :len(r)].cpu().numpy().view(np.uint16), r.astype(np.uint16))


# ---- one stream across the whole grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,sym_bytes", [(3, 1), (17, 4)])
def test_one_large_stream(width, sym_bytes):
    n = 1 << 22
    dev, code = device(), FixedWidthCode()
    idx = np.random.default_rng(width).integers(0, 1 << width, n, dtype=np.uint64).astype(NP_SYM[sym_bytes])
    sym = torch.from_numpy(idx.view({1: np.uint8, 4: np.int32}[sym_bytes])).to(dev).view(1, n)
    enc = code.encode_batch(sym, None, width, 1 << width)
    assert enc.status.tolist() == [0] and enc.nbits.tolist() == [n * width]
    stream = enc.data.cpu().numpy()
    # 32 symbols are `width` words: any run of whole groups stands alone in the stream
    for a, b in ((0, 2 * TILE), (n // 2 - TILE - 32, n // 2 + 64), (n - TILE - 32, n)):
        packed, _ = pack(idx[a:b], width)
        assert np.array_equal(stream[a // 32 * 4 * width: b // 32 * 4 * width], packed), (a, b)
    val, got, used, status = code.decode_encoded(enc, None, width, 1 << width, n, dtype=torch_sym(sym_bytes))
    assert status.tolist() == [0] and got.tolist() == [n]
    assert torch.equal(val.view(-1), sym.view(-1))


def test_kernel_names():
    code = FixedWidthCode()
    assert code.kernel_names(1, 1) == ("fixed_encode_kernel<unsigned char>", "fixed_decode_kernel<unsigned char>")
    assert code.kernel_names(1, 4) == ("fixed_encode_kernel<unsigned int>", "fixed_decode_kernel<unsigned int>")


# ---- the classes on the device ----------------------------------------------------------------------------------------------------------
def fixed_coders(case):
    if case.coder == "pickle":
        return fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    return fbc.TextFixedBitwidthEncoder(), fbc.TextFixedBitwidthDecoder()


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setattr(fbc, "FIXED_BLOCK_MIN", 1)


def data_section_is_the_restatement(case, enc, bits, data):
    dec = fixed_coders(case)[1]
    alphabet, used = dec.alphabet_decoder.decode_block(bits)
    assert bits[:used] == enc.alphabet_encoder.encode_block(alphabet)
    index_of = {s: i for i, s in enumerate(alphabet)}
    want = pack_bits([index_of[s] for s in data], fbc.get_alphabet_fixed_bitwidth(len(alphabet)))
    assert np.array_equal(np.asarray(bits.tolist()[used + 32:], np.uint8), want)
    return alphabet


@pytest.mark.parametrize("case", BLOCKS, ids=golden_ids(BLOCKS))
def test_classes_on_the_device_against_the_goldens(case, device_path):
    enc, dec = fixed_coders(case)
    data = golden_symbols(case)
    bits = enc.encode_block(DataBlock(data))
    alphabet = data_section_is_the_restatement(case, enc, bits, data)
    golden = BitArray.from_packed(case.arr("out"), case.nbits)
    if case.symbols == "int":  # set order of small ints is fixed: the reference's data section bit for bit
        assert alphabet == golden_symbols(case, "order")
        assert bits[len(bits) - case.n * fbc.get_alphabet_fixed_bitwidth(len(alphabet)):] == golden[case.head_bits + 32:]
    for packed, total, used in case.bits_with_garbage:  # the reference's bits, garbage behind them
        block, consumed = dec.decode_block(BitArray.from_packed(packed, total))
        assert consumed == used and block.data_list == data
    assert dec.decode_block(bits)[0].data_list == data


def test_device_path_faults(device_path):
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    bits = enc.encode_block(DataBlock([0, 1, 2, 2, 1]))
    with pytest.raises(backend_lib.SclHipError, match="TRUNCATED"):
        dec.decode_block(bits[: len(bits) - 1])
    bad = bits.copy()
    bad[len(bits) - 2:] = BitArray("11")
    with pytest.raises(IndexError):
        dec.decode_block(bad)
    with pytest.raises(IndexError):
        dec.decode_blocks([bits, bad])


def test_threshold_sides_write_the_same_bits():
    rng = np.random.default_rng(9)
    data = rng.integers(0, 300, fbc.FIXED_BLOCK_MIN).tolist()
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    at, below = enc.encode_block(DataBlock(data)), enc.encode_block(DataBlock(data[:-1]))
    alphabet = data_section_is_the_restatement(BLOCKS[0], enc, at, data)
    assert dec.decode_block(at)[0].data_list == data and dec.decode_block(below)[0].data_list == data[:-1]
    assert len(alphabet) == 300


def test_blocks_in_batched_launches_equal_the_loop():
    cases = [c for c in BLOCKS if c.coder == "pickle"]
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    blocks = [DataBlock(golden_symbols(c)) for c in cases]
    loop = [enc.encode_block(b) for b in blocks]
    batched = enc.encode_blocks(blocks)
    assert all(a == b for a, b in zip(loop, batched)) and len(batched) == len(loop)
    junk = BitArray("1011001")
    streams = [b + junk if i % 2 else b for i, b in enumerate(loop)]
    want = [dec.decode_block(s) for s in streams]
    got = dec.decode_blocks(streams)
    assert [(b.data_list, used) for b, used in got] == [(b.data_list, used) for b, used in want]
    assert [b.data_list for b, _ in got] == [b.data_list for b in blocks]
    text_enc, text_dec = fbc.TextFixedBitwidthEncoder(), fbc.TextFixedBitwidthDecoder()
    texts = [DataBlock(list(s)) for s in ("ABCCACD", "A", "hello world", "ab" * 5000)]
    coded = text_enc.encode_blocks(texts)
    assert all(a == text_enc.encode_block(b) for a, b in zip(coded, texts))
    assert [b.data_list for b, _ in text_dec.decode_blocks(coded)] == [b.data_list for b in texts]


def test_file_round_trip_on_the_device(tmp_path, device_path):
    case = next(c for c in FIXED if c.kind == "file")
    src, coded, back = tmp_path / "in.txt", tmp_path / "coded.bin", tmp_path / "back.txt"
    src.write_bytes(case.arr("text").tobytes())
    assert try_file_lossless_compression(str(src), fbc.TextFixedBitwidthEncoder(), fbc.TextFixedBitwidthDecoder(),
                                         encode_block_size=case.block_size)
    coded.write_bytes(case.arr("file").tobytes())
    fbc.TextFixedBitwidthDecoder().decode_file(str(coded), str(back))
    assert back.read_bytes() == case.arr("text").tobytes()


def test_the_reference_100k_block():
    """test_fixed_bitwidth_encode_decode of the reference: 100 000 symbols over four, 2 bits each, on the device by size"""
    case = next(c for c in BLOCKS if c.group == "reference100k")
    assert case.n >= fbc.FIXED_BLOCK_MIN
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    data = golden_symbols(case)
    bits = enc.encode_block(DataBlock(data))
    assert dec.decode_block(bits)[0].data_list == data
    assert len(bits) / case.n - 2.0 < 1e-2


FAMILY_CODERS = {"shannon": (ShannonEncoder, ShannonDecoder), "fano": (FanoEncoder, FanoDecoder),
                 "sfe": (ShannonFanoEliasEncoder, ShannonFanoEliasDecoder)}


@pytest.mark.parametrize("case", FAMILY_BLOCKS, ids=golden_ids(FAMILY_BLOCKS))
def test_shannon_family_blocks_on_the_device(case):
    table = next(c for c in FAMILY if c.id == case.table)
    values = table.arr("symbols").tolist()
    symbols = [chr(v) for v in values] if table.symbols == "str" else values
    dist = ProbabilityDist(dict(zip(symbols, table.arr("probs").tolist())))
    Enc, Dec = FAMILY_CODERS[case.coder]
    data = [symbols[i] for i in case.arr("data").tolist()]
    bits = Enc(dist).encode_block(DataBlock(data))
    assert bits == BitArray.from_packed(case.arr("out"), case.nbits)
    block, used = Dec(dist).decode_block(bits)
    assert block.data_list == data and used == case.consumed
