"""GPU: the prefix-free / Huffman coders (csrc/scl_prefix.hip) against the reference's goldens and a numpy restatement of
the stream, with both kernel forms: tuned (byte symbols) and any-parameter.  Every expectation comes from the goldens
(tables, blocks, the framed file) or from concatenating the goldens' codewords in numpy -- never from the code under test."""
import os

import numpy as np
import pytest

from conftest import frame_blocks
from prefix_helpers import code_bits, encode_numpy, goldens, make_dist, stream_bits, table_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5
ST_CAPACITY, ST_TRUNCATED, ST_STATE = 0x1, 0x4, 0x8
BLOCK_GROUPS = sorted({c.group for c in goldens()["block"]})
_models = {}


def device():
    from stanford_compression_library_amd.backend import lib

    lib.require_device()
    return torch.device("cuda:0")


def model_of(group):
    from stanford_compression_library_amd.backend.models import PrefixModel

    if group not in _models:
        case = table_case(group)
        _models[group] = (PrefixModel(case.arr("code"), case.arr("len")), code_bits(case), case)
    return _models[group]


def forms(model):
    """the kernel forms to compare: (any_parameter_kernels flag, name)"""
    return [(False, "tuned" if model.fast_path() and not model.wide else "default"), (True, "any")]


def to_rows(model, chunks, dev, pad_to=16):
    """ragged list of index arrays -> (sym tensor [n, width], lens int32 tensor, host lens)"""
    lens = np.array([len(c) for c in chunks], np.int32)
    width = max(int(lens.max(initial=0)), 1)
    width = (width + pad_to - 1) // pad_to * pad_to
    host = np.zeros((len(chunks), width), model.sym_dtype)
    for i, c in enumerate(chunks):
        host[i, :len(c)] = c
    sym = torch.from_numpy(host.view(np.int16) if model.wide else host).to(dev)
    return (sym.view(torch.uint16) if model.wide else sym), torch.from_numpy(lens).to(dev), lens


def check_encoded(enc, expected, what):
    """streams, nbits, bit offsets and status of a batch equal the restatement [(packed, nbits)]"""
    data = enc.data.cpu().numpy()
    nbits, off, status = enc.nbits.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.status.cpu().numpy()
    assert (status == 0).all(), f"{what}: status {status[status != 0][:8]}"
    assert nbits.tolist() == [nb for _, nb in expected], what
    assert off.tolist() == [8 * c * enc.stride for c in range(enc.n_chunks)], what
    for c, (packed, nb) in enumerate(expected):
        assert np.array_equal(stream_bits(data, int(off[c]), nb), packed), f"{what}: stream {c}"


def check_decoded(dec, chunks, expected, what):
    sym, lens, used, status = (t.cpu().numpy() for t in dec)
    assert (status == 0).all(), f"{what}: status {status[status != 0][:8]}"
    assert lens.tolist() == [len(c) for c in chunks], what
    assert used.tolist() == [nb for _, nb in expected], what
    for c, chunk in enumerate(chunks):
        assert np.array_equal(sym[c, :len(chunk)].astype(np.int64), np.asarray(chunk, np.int64)), f"{what}: chunk {c}"


def round_trip_both_forms(group, chunks, expected, what):
    """encode and decode `chunks` with both kernel forms; the two encoders' buffers are equal word for word"""
    dev = device()
    model, _, _ = model_of(group)
    sym, lens, host_lens = to_rows(model, chunks, dev)
    cap = max(int(host_lens.max(initial=0)), 1)
    buffers = []
    for any_par, name in forms(model):
        enc = model.alloc_encoded(len(chunks), sym.shape[1], dev)
        enc.data.zero_()
        model.encode_batch(sym, lens, out=enc, any_parameter_kernels=any_par)
        check_encoded(enc, expected, f"{what}/{name}")
        buffers.append(enc.data.cpu().numpy())
        for dec_any, dec_name in forms(model):
            dec = model.decode_encoded(enc, cap, any_parameter_kernels=dec_any)
            check_decoded(dec, chunks, expected, f"{what}/{name}->{dec_name}")
    assert np.array_equal(buffers[0], buffers[1]), f"{what}: tuned and any-parameter slots differ"
    return model


# ---- goldens ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", BLOCK_GROUPS)
def test_golden_blocks_through_the_classes(group):
    from stanford_compression_library_amd.backend.models import _any_parameter
    from stanford_compression_library_amd.compressors import HuffmanDecoder, HuffmanEncoder
    from stanford_compression_library_amd.core.data_block import DataBlock
    from stanford_compression_library_amd.utils.bitarray_utils import BitArray

    device()
    dist = make_dist(table_case(group))
    enc, dec = HuffmanEncoder(dist), HuffmanDecoder(dist)
    for any_par in (False, True):
        with _any_parameter(any_par):
            for case in (c for c in goldens()["block"] if c.group == group):
                want = BitArray.from_packed(case.arr("out"), case.nbits)
                sym = case.arr("sym").tolist()
                bits = enc.encode_block(DataBlock(sym))
                assert len(bits) == case.nbits and bits == want, (case, any_par)
                block, used = dec.decode_block(want)
                assert used == case.consumed == case.nbits and block.data_list == sym, (case, any_par)


@pytest.mark.parametrize("group", BLOCK_GROUPS)
def test_golden_blocks_through_the_batch_calls(group):
    cases = [c for c in goldens()["block"] if c.group == group]
    chunks = [c.arr("sym") for c in cases]
    expected = [(c.arr("out"), c.nbits) for c in cases]
    _, bits_of, _ = model_of(group)
    for chunk, (packed, nb) in zip(chunks, expected):  # the restatement the other tests rely on, pinned by the goldens
        mine, mine_nb = encode_numpy(bits_of, chunk)
        assert mine_nb == nb and np.array_equal(mine, packed)
    round_trip_both_forms(group, chunks, expected, group)


# ---- ragged batch: one full 256-lane workgroup and a partial one that ends in a partial wave -------------------------------
@pytest.mark.parametrize("group", ["uniform5", "random256", "random300"])
def test_ragged_batch(group):
    model, bits_of, case = model_of(group)
    rng = np.random.default_rng(case.K)
    lens = rng.integers(0, 701, 300)
    lens[:4] = [0, 1, 700, 699]
    probs = case.arr("probs")
    chunks = [rng.choice(case.K, size=int(n), p=probs) for n in lens]
    expected = [encode_numpy(bits_of, c) for c in chunks]
    round_trip_both_forms(group, chunks, expected, group)
    info = model.info()
    assert (info.K, info.max_len, info.lut_bits) == (case.K, case.max_len, min(case.max_len, 11))
    assert bool(info.fast_path) == (case.K <= 256)


def test_long_codes_leave_the_lookup_table():
    """codes of up to 27 bits, chunks made mostly of the rarest symbols: codewords straddle the 32-bit words of the
    writer and the reader, and the decoder walks the tree below its 11-bit table"""
    _, bits_of, case = model_of("skewed28")
    assert 12 <= case.max_len <= 32
    rng = np.random.default_rng(28)
    rare = np.argsort(case.arr("len"))[::-1][:8]
    chunks = []
    for n in rng.integers(0, 301, 70):
        c = rng.choice(rare, size=int(n))
        mix = rng.random(int(n)) < 0.2
        c[mix] = rng.integers(0, case.K, int(mix.sum()))
        chunks.append(c)
    chunks[0] = np.full(300, rare[0])  # the longest code back to back
    expected = [encode_numpy(bits_of, c) for c in chunks]
    round_trip_both_forms("skewed28", chunks, expected, "skewed28")


# ---- guard bands ----------------------------------------------------------------------------------------------------------
class Arena:
    """buffers carved out of one 0xA5-filled allocation with guard bands around them (as tests/test_gpu_guard_bands.py)"""

    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)
        self.pos = GUARD
        self.used = []

    def take(self, nbytes, dtype=torch.uint8):
        start = (self.pos + 255) // 256 * 256
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


def arena_encoded(arena, n, stride):
    from stanford_compression_library_amd.backend.models import EncodedBatch

    return EncodedBatch(arena.take(n * stride), stride, arena.take(8 * n, torch.int64), arena.take(4 * n, torch.int32),
                        arena.take(4 * n, torch.int32), n)


def arena_decoded(arena, n, row_stride, cap):
    rows = arena.take(n * row_stride)
    sym = torch.as_strided(rows, (n, cap), (row_stride, 1))
    return rows, (sym, arena.take(4 * n, torch.int32), arena.take(4 * n, torch.int32), arena.take(4 * n, torch.int32))


def ragged_chunks(case, rng, n_chunks, max_len):
    lens = rng.integers(0, max_len + 1, n_chunks)
    lens[:4] = [0, 1, max_len, max_len - 1]
    return [rng.choice(case.K, size=int(n), p=case.arr("probs")) for n in lens]


@pytest.mark.parametrize("any_par", [False, True], ids=["tuned", "any"])
@pytest.mark.parametrize("group", ["random17", "random256"])
def test_slots_of_exactly_slot_bytes_between_guard_bands(group, any_par):
    dev = device()
    model, bits_of, case = model_of(group)
    rng = np.random.default_rng(5)
    chunks = ragged_chunks(case, rng, 300, 333)
    # the worst case fills its slot: every symbol the longest code
    chunks[2] = np.full(333, int(np.argmax(case.arr("len"))))
    expected = [encode_numpy(bits_of, c) for c in chunks]
    sym, lens, _ = to_rows(model, chunks, dev)
    stride = model.slot_bytes(333)
    assert stride % 128 == 0 and stride >= (333 * case.max_len + 7) // 8
    arena = Arena(300 * (stride + 400) + 40 * GUARD, dev)
    enc = arena_encoded(arena, 300, stride)
    model.encode_batch(sym[:, :333], lens, out=enc, any_parameter_kernels=any_par)
    torch.cuda.synchronize()
    arena.check("encode")
    check_encoded(enc, expected, group)
    rows, out = arena_decoded(arena, 300, 336, 333)
    dec = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, 333, out=out, any_parameter_kernels=any_par)
    torch.cuda.synchronize()
    arena.check("decode")
    check_decoded(dec, chunks, expected, group)
    host = rows.cpu().numpy().reshape(300, 336)
    for c, chunk in enumerate(chunks):  # nothing behind a row's symbols
        assert (host[c, len(chunk):] == FILL).all(), c


@pytest.mark.parametrize("any_par", [False, True], ids=["tuned", "any"])
def test_short_slots_report_capacity_and_spare_their_neighbours(any_par):
    dev = device()
    model, bits_of, case = model_of("random256")
    rng = np.random.default_rng(6)
    chunks = ragged_chunks(case, rng, 300, 400)
    expected = [encode_numpy(bits_of, c) for c in chunks]
    sym, lens, _ = to_rows(model, chunks, dev)
    stride = 144  # 16-byte aligned, not a multiple of 128: most chunks do not fit
    arena = Arena(300 * stride + 40 * GUARD, dev)
    enc = arena_encoded(arena, 300, stride)
    model.encode_batch(sym, lens, out=enc, any_parameter_kernels=any_par)
    torch.cuda.synchronize()
    arena.check("encode")
    data, status, nbits = enc.data.cpu().numpy(), enc.status.cpu().numpy(), enc.nbits.cpu().numpy()
    fits = np.array([(nb + 7) // 8 <= stride for _, nb in expected])
    assert fits.any() and (~fits).any()
    assert nbits.tolist() == [nb for _, nb in expected]  # what the stream needs, also when it did not fit
    assert status.tolist() == [0 if f else ST_CAPACITY for f in fits]
    for c in np.nonzero(fits)[0]:
        assert np.array_equal(stream_bits(data, 8 * int(c) * stride, expected[c][1]), expected[c][0]), c


@pytest.mark.parametrize("row_stride", [48, 37], ids=["aligned_rows", "unaligned_rows"])
@pytest.mark.parametrize("any_par", [False, True], ids=["tuned", "any"])
def test_out_cap_below_the_count_reports_capacity(any_par, row_stride):
    dev = device()
    model, bits_of, case = model_of("random17")
    rng = np.random.default_rng(7)
    chunks = ragged_chunks(case, rng, 300, 80)
    expected = [encode_numpy(bits_of, c) for c in chunks]
    sym, lens, _ = to_rows(model, chunks, dev)
    enc = model.encode_batch(sym, lens)
    cap = 37
    arena = Arena(300 * row_stride + 40 * GUARD, dev)
    rows, out = arena_decoded(arena, 300, row_stride, cap)
    dsym, dlens, used, status = (t.cpu().numpy() for t in
                                 model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap, out=out,
                                                    any_parameter_kernels=any_par))
    arena.check("decode")
    code_len = case.arr("len")
    host = rows.cpu().numpy()
    for c, chunk in enumerate(chunks):
        n = min(len(chunk), cap)
        assert status[c] == (ST_CAPACITY if len(chunk) > cap else 0), c
        assert dlens[c] == n and np.array_equal(dsym[c, :n], chunk[:n]), c
        assert used[c] == int(code_len[chunk[:n]].sum()), c
        if row_stride > cap:  # nothing past out_cap, nothing behind a shorter row's symbols
            assert (host[c * row_stride + n:(c + 1) * row_stride] == FILL).all(), c


# ---- damaged input ----------------------------------------------------------------------------------------------------------
def decode_damaged(model, data, bit_offset, nbits, cap, what):
    """decode with both forms into guarded rows; the forms must agree; -> (sym, lens, used, status) of the first"""
    dev = data.device
    n = int(bit_offset.numel())
    results = []
    for any_par, name in forms(model):
        arena = Arena(n * (cap + 16) + 40 * GUARD, dev)
        row_stride = (cap + 15) // 16 * 16
        rows, out = arena_decoded(arena, n, row_stride, cap)
        dec = model.decode_batch(data, bit_offset, nbits, cap, out=out, any_parameter_kernels=any_par)
        torch.cuda.synchronize()  # the call returned and the device is alive
        arena.check(f"{what}/{name}")
        sym, lens, used, status = (t.cpu().numpy() for t in dec)
        assert (lens <= cap).all()
        host = rows.cpu().numpy().reshape(n, row_stride)
        for c in range(n):
            assert (host[c, lens[c]:] == FILL).all(), f"{what}/{name}: row {c} written behind its symbols"
        results.append((sym, lens, used, status))
    a, b = results
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), what
    for c in range(n):
        assert np.array_equal(a[0][c, :a[1][c]], b[0][c, :b[1][c]]), f"{what}: chunk {c}"
    return a


def damaged_base(group, n_chunks=96, max_len=120):
    dev = device()
    model, bits_of, case = model_of(group)
    rng = np.random.default_rng(9)
    chunks = ragged_chunks(case, rng, n_chunks, max_len)
    expected = [encode_numpy(bits_of, c) for c in chunks]
    sym, lens, _ = to_rows(model, chunks, dev)
    enc = model.encode_batch(sym, lens)
    check_encoded(enc, expected, group)
    return model, case, rng, chunks, expected, enc


def check_unharmed(res, chunks, expected, harmed, what):
    sym, lens, used, status = res
    for c, chunk in enumerate(chunks):
        if c in harmed:
            continue
        assert status[c] == 0 and lens[c] == len(chunk) and used[c] == expected[c][1], f"{what}: chunk {c}"
        assert np.array_equal(sym[c, :len(chunk)], chunk), f"{what}: chunk {c}"


def test_stream_cut_inside_a_codeword_is_truncated():
    model, case, rng, chunks, expected, enc = damaged_base("random17")
    code_len = case.arr("len")
    nbits = enc.nbits.cpu().numpy().copy()
    harmed = {}
    for c, chunk in enumerate(chunks):
        last = int(code_len[chunk[-1]]) if len(chunk) else 0
        if last >= 2 and c % 3 == 0:
            cut = int(rng.integers(1, last))  # 1 .. last - 1 bits of the last codeword are gone
            nbits[c] -= cut
            harmed[c] = last
    assert len(harmed) > 5
    res = decode_damaged(model, enc.data, enc.bit_offset, torch.from_numpy(nbits).to(enc.data.device), 120, "cut")
    sym, lens, used, status = res
    for c, last in harmed.items():
        assert status[c] == ST_TRUNCATED, c
        assert lens[c] == len(chunks[c]) - 1 and used[c] == expected[c][1] - last, c
        assert np.array_equal(sym[c, :lens[c]], chunks[c][:-1]), c
    check_unharmed(res, chunks, expected, harmed, "cut")


@pytest.mark.parametrize("group", ["random17", "skewed28", "one_symbol"])
def test_bit_flips_and_random_bytes_give_a_status_never_a_fault(group):
    model, case, rng, chunks, expected, enc = damaged_base(group)
    dev = enc.data.device
    min_len = int(case.arr("len").min())
    cap = 120 * int(case.max_len) // min_len + 8  # holds whatever 120 symbols' worth of bits can decode to
    allowed = {0, ST_TRUNCATED, ST_STATE}
    # bit flips in every fourth stream
    data = enc.data.cpu().numpy().copy()
    harmed = set()
    for c in range(0, len(chunks), 4):
        nb = expected[c][1]
        if nb == 0:
            continue
        for bit in rng.integers(0, nb, 3):
            pos = 8 * c * enc.stride + int(bit)
            data[pos >> 3] ^= 0x80 >> (pos & 7)
        harmed.add(c)
    res = decode_damaged(model, torch.from_numpy(data).to(dev), enc.bit_offset, enc.nbits, cap, f"{group}/flips")
    assert set(res[3].tolist()) <= allowed
    check_unharmed(res, chunks, expected, harmed, f"{group}/flips")
    # random bytes with random lengths in every other slot (descriptors included: any length the slot can hold)
    data = enc.data.cpu().numpy().copy()
    nbits = enc.nbits.cpu().numpy().copy()
    harmed = set(range(1, len(chunks), 2))
    for c in harmed:
        data[c * enc.stride:(c + 1) * enc.stride] = rng.integers(0, 256, enc.stride)
        nbits[c] = rng.integers(0, 120 * min_len + 1)
    res = decode_damaged(model, torch.from_numpy(data).to(dev), enc.bit_offset, torch.from_numpy(nbits).to(dev), cap,
                         f"{group}/random")
    assert set(res[3].tolist()) <= allowed  # (the one-symbol code: 0 or STATE -- a 1 bit has no child to go to)
    assert (res[2] <= nbits).all()
    check_unharmed(res, chunks, expected, harmed, f"{group}/random")


# ---- compaction: dense = BitArray.tobytes() of every block back to back, framed = the reference's file records ------------
@pytest.mark.parametrize("framed", [False, True], ids=["dense", "framed"])
def test_compaction_with_zero_length_streams(framed):
    from stanford_compression_library_amd.backend.models import compact

    dev = device()
    model, bits_of, case = model_of("random17")
    rng = np.random.default_rng(10)
    chunks = ragged_chunks(case, rng, 70, 90)
    chunks[5] = chunks[6] = chunks[69] = np.zeros(0, np.int64)  # empty blocks: inside, adjacent, last
    expected = [encode_numpy(bits_of, c) for c in chunks]
    assert expected[0][1] == 0
    sym, lens, _ = to_rows(model, chunks, dev)
    enc = model.encode_batch(sym, lens)
    out, offsets = compact(enc, framed=framed)
    want = frame_blocks(expected) if framed else np.concatenate([p for p, _ in expected])
    offsets = offsets.cpu().numpy()
    assert offsets[-1] == want.size
    assert np.array_equal(out.cpu().numpy()[:want.size], want)
    sizes = [(4 + (nb + 3 + 7) // 8) if framed else (nb + 7) // 8 for _, nb in expected]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()


# ---- files: the plain block loop of DataEncoder / DataDecoder ---------------------------------------------------------------
def test_encode_file_equals_the_reference_and_round_trips(tmp_path):
    from stanford_compression_library_amd.compressors import HuffmanDecoder, HuffmanEncoder
    from stanford_compression_library_amd.core.prob_dist import ProbabilityDist

    device()
    case = goldens()["file"][0]
    dist = ProbabilityDist({c: float(p) for c, p in zip(case.chars, case.arr("probs"))})
    text = case.arr("text").tobytes().decode("ascii")
    src, dst, back = (str(tmp_path / n) for n in ("in.txt", "out.bin", "back.txt"))
    with open(src, "w", newline="") as f:
        f.write(text)
    HuffmanEncoder(dist).encode_file(src, dst, block_size=case.block_size)
    assert np.array_equal(np.fromfile(dst, np.uint8), case.arr("encoded"))
    HuffmanDecoder(dist).decode_file(dst, back)
    assert open(back, newline="").read() == text
    # a few KB, several blocks and a short last one
    rng = np.random.default_rng(12)
    long_text = "".join(rng.choice(list(case.chars), size=5000, p=case.arr("probs")))
    with open(src, "w", newline="") as f:
        f.write(long_text)
    HuffmanEncoder(dist).encode_file(src, dst, block_size=1024)
    HuffmanDecoder(dist).decode_file(dst, back)
    assert open(back, newline="").read() == long_text
    assert os.path.getsize(dst) < len(long_text)
