"""The integer codes (Golomb, universal, Elias-delta) on the device: one block across the whole grid (csrc/scl_uint_block.hip)
against the restatement of tests/uint_code_helpers.py and the reference's goldens -- the bits, the values, and for damaged
streams the (values, consumed, status) of the sequential decoder.  Sizes sit on the kernels' edges: an encoder tile is 4096
values, 16 a thread; a decoder thread owns 128 bits, a decoder workgroup 32 768."""
import numpy as np
import pytest

from conftest import golden_ids
from stanford_compression_library_amd.backend.models import UintCode
from stanford_compression_library_amd.compressors import _uint_block
from stanford_compression_library_amd.compressors import (GolombUintDecoder, GolombUintEncoder, UniversalUintDecoder,
                                                          UniversalUintEncoder)
from stanford_compression_library_amd.compressors.elias_delta_uint_coder import EliasDeltaUintDecoder, EliasDeltaUintEncoder
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.utils.bitarray_utils import BitArray
from stanford_compression_library_amd.utils.test_utils import try_lossless_compression
from uint_code_helpers import (CODE_IDS, CODES, GOLDENS, ST_CAPACITY, ST_SIZE, ST_TRUNCATED, codeword, decode_stream,
                               encode_bits, geometric, golden_code, golomb_params, length_boundaries, pack)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5
TILE, PER_THREAD, SUB, GROUP = 4096, 16, 128, 32768
BIG_OFFSET = (1 << 32) + 5


def device():
    return torch.device("cuda:0")


def coders(kind, M):
    if kind == "golomb":
        return GolombUintEncoder(M), GolombUintDecoder(M)
    if kind == "universal":
        return UniversalUintEncoder(), UniversalUintDecoder()
    return EliasDeltaUintEncoder(), EliasDeltaUintDecoder()


class Arena:
    """buffers between guard bands (the pattern of test_gpu_prefix_block.py)"""

    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes + 16 * GUARD,), FILL, dtype=torch.uint8, device=dev)
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


def value_tensor(values, dev):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)).to(dev)


def draw(kind, M, n, seed=0):
    """n values of up to 32 bits: a geometric source around the code's own scale, every tenth a length boundary"""
    rng = np.random.default_rng(seed + n)
    values = geometric(n, mean=8.0 * (M or 1), seed=seed + n).astype(np.int64)
    edges = np.array([v for v in length_boundaries(kind, M) if codeword(kind, M, v)[1] <= 32], np.int64)
    mix = rng.random(n) < 0.1
    values[mix] = rng.choice(edges, int(mix.sum()))
    keep = np.array([codeword(kind, M, int(v))[1] <= 32 for v in values], bool)
    values[~keep] = 0
    return values


def block_encode(code, values, cap, what):
    """the code under test, its output between guard bands -> (the bytes of the whole buffer, nbits, status)"""
    dev = device()
    arena = Arena(cap + 4 * GUARD, dev)
    out = arena.take(max(cap, 4), align=4)
    meta = code.encode_block_into(value_tensor(values, dev), out, out_cap_bytes=cap)
    torch.cuda.synchronize()
    arena.check(what)
    nbits, status = (int(v) for v in meta.cpu())
    return out.cpu().numpy(), nbits, status & 0xFFFFFFFF


def check_encode(code, kind, M, values, what):
    want_bits, _ = encode_bits(kind, M, values)
    want, nbits = pack(want_bits), int(want_bits.size)
    nbytes = (nbits + 7) // 8
    reach = 4 * len(values)  # the call zeroes its output up to the longest possible stream, 32 bits a value
    for cap in sorted({nbytes, (nbytes + 3) // 4 * 4, nbytes + 7, reach + 61}):  # a multiple of 4 and not, exact and roomy
        raw, got_bits, status = block_encode(code, values, cap, f"{what}/cap{cap}")
        assert (got_bits, status) == (nbits, 0), (what, cap)
        assert np.array_equal(raw[:nbytes], want), (what, cap)
        assert not raw[nbytes:min(reach, cap)].any(), (what, cap)
        assert (raw[reach:cap] == FILL).all(), (what, cap)  # nothing is touched behind what the call may zero
    return want_bits


def stream_at(bits, bit_offset, dev, big=None):
    """the bits at bit ``bit_offset`` of a device buffer, ones in front and behind -> (uint8 tensor, its bytes)"""
    lead = bit_offset & 7
    body = pack(np.concatenate([np.ones(lead, np.uint8), bits, np.ones(77, np.uint8)]))
    body = np.concatenate([body, np.full((-body.size) % 4 + 4, 0xFF, np.uint8)])
    first = bit_offset >> 3
    if big is not None:
        big[first:first + body.size] = torch.from_numpy(body).to(dev)
        return big[:first + body.size]
    data = torch.full((first + body.size,), 0xFF, dtype=torch.uint8, device=dev)
    data[first:] = torch.from_numpy(body).to(dev)
    return data


def block_decode(code, data, bit_offset, nbits, cap, what):
    """the code under test, its output between guard bands -> (values, n_out, consumed, status, sync_passes)"""
    arena = Arena(max(cap, 1) * 4 + 4 * GUARD, data.device)
    out = arena.take(max(cap, 1) * 4, torch.int32)
    _, n_out, consumed, status, passes = code.decode_block_device(data, nbits, bit_offset, out_cap=cap, out=out)
    torch.cuda.synchronize()
    arena.check(what)
    assert n_out <= cap, what
    raw = out.view(torch.uint8).cpu().numpy()
    assert (raw[n_out * 4:] == FILL).all(), f"{what}: values stored behind n_out"
    return raw[:n_out * 4].view(np.uint32), n_out, consumed, status, passes


def check_decode(code, kind, M, bits, nbits, cap, what, bit_offset=0, big=None, want=None):
    """the device against the sequential decoder, field for field"""
    if want is None:
        want = decode_stream(kind, M, bits, nbits=nbits, cap=cap)
    data = stream_at(bits, bit_offset, device(), big)
    got = block_decode(code, data, bit_offset, nbits, cap, what)
    assert np.array_equal(got[0], want[0]), what
    assert (got[1], got[2], got[3]) == (len(want[0]), want[1], want[2]), (what, got[1:], want[1:])
    return got


@pytest.fixture(scope="module")
def big_buffer():
    """512 MiB and a little: a stream that starts behind bit 2^32"""
    buf = torch.full(((BIG_OFFSET >> 3) + (1 << 20),), 0xFF, dtype=torch.uint8, device=device())
    yield buf
    del buf
    torch.cuda.empty_cache()


# ---- 1. the goldens, through the C ABI and through the classes ---------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_goldens(case, monkeypatch):
    kind, M = golden_code(case)
    code = UintCode(kind, M)
    values = case.arr("values")
    golden_bits = np.unpackbits(case.arr("out"))[:case.nbits]
    if case.device:
        raw, nbits, status = block_encode(code, values, (case.nbits + 7) // 8, repr(case))
        assert (nbits, status) == (case.nbits, 0)
        assert np.array_equal(raw[:(case.nbits + 7) // 8], case.arr("out"))
        got = check_decode(code, kind, M, golden_bits, case.nbits, max(len(values), 1), repr(case))
        assert np.array_equal(got[0], values) and got[2:4] == (case.nbits, 0)
    elif int(values.max()) < (1 << 32):  # a codeword above 32 bits: refused whole on encode, named on decode
        raw, nbits, status = block_encode(code, values, 64, repr(case))
        assert (nbits, status) == (0, ST_SIZE) and not raw[:min(64, 4 * len(values))].any()
        if case.nbits < (1 << 16):
            assert check_decode(code, kind, M, golden_bits, case.nbits, len(values), repr(case))[3] == ST_SIZE
    monkeypatch.setattr(_uint_block, "UINT_BLOCK_MIN", 0)
    enc, dec = coders(kind, M)
    bits = enc.encode_block(DataBlock([int(v) for v in values]))
    assert len(bits) == case.nbits and np.array_equal(bits.packed(), case.arr("out"))
    block, used = dec.decode_block(bits)
    assert block.data_list == [int(v) for v in values] and used == case.nbits


# ---- 2. sizes around a thread's 16 values and a tile's 4096 -------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_sizes(kind, M, big_buffer):
    code = UintCode(kind, M)
    for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5):
        values = draw(kind, M, n)
        what = f"{kind}{M}/{n}"
        if n == 0:
            raw, nbits, status = block_encode(code, values, 8, what)
            assert (nbits, status) == (0, 0) and (raw == FILL).all()
            for off in (0, 5):
                got = block_decode(code, stream_at(np.zeros(0, np.uint8), off, device()), off, 0, 4, what)
                assert got[1:4] == (0, 0, 0)
            continue
        bits = check_encode(code, kind, M, values, what)
        for off in (0, 5, BIG_OFFSET):
            got = check_decode(code, kind, M, bits, bits.size, n, f"{what}@{off}", off, big_buffer if off > 64 else None,
                               want=(values.astype(np.uint32), int(bits.size), 0))
            assert got[3] == 0


# ---- 3. extreme tiles ----------------------------------------------------------------------------------------------------------
def test_a_tile_of_32_bit_codewords():
    """universal, every x in [2^15, 2^16): a tile fills its 4096 words of LDS to the last"""
    code = UintCode("universal")
    values = np.concatenate([np.arange(1 << 15, (1 << 15) + TILE), np.random.default_rng(1).integers(1 << 15, 1 << 16, TILE + 17)])
    assert all(codeword("universal", None, int(v))[1] == 32 for v in values[::97])
    bits = check_encode(code, "universal", None, values, "32-bit")
    assert bits.size == 32 * values.size
    check_decode(code, "universal", None, bits, bits.size, values.size, "32-bit", 5, want=(values.astype(np.uint32), int(bits.size), 0))


def test_a_stream_of_1_bit_codewords():
    """Golomb M = 1, all zeros: 16 codewords in half a word on encode, 128 values in every decoder thread"""
    code = UintCode("golomb", 1)
    for n in (31, 2 * TILE + 33, 2 * GROUP + SUB + 1):
        values = np.zeros(n, np.int64)
        bits = check_encode(code, "golomb", 1, values, f"1-bit/{n}")
        assert bits.size == n and not bits.any()
        check_decode(code, "golomb", 1, bits, n, n, f"1-bit/{n}", 0, want=(values.astype(np.uint32), n, 0))


def test_all_zero_universal_values_need_no_second_pass():
    """every universal length is even (len_gcd = 2): starts on even bits are codeword starts, so pass 0 is exact"""
    code = UintCode("universal")
    n = (2 * GROUP + 70) // 2
    values = np.zeros(n, np.int64)
    bits = check_encode(code, "universal", None, values, "zeros")
    for off in (0, 5):
        got = check_decode(code, "universal", None, bits, bits.size, n, f"zeros@{off}", off, want=(values.astype(np.uint32), 2 * n, 0))
        assert got[4] == 0


# ---- 4. workgroup edges --------------------------------------------------------------------------------------------------------
def long_value(kind, M):
    """a value whose codeword has 24 bits or more"""
    x = {"universal": 3000, "elias_delta": 1 << 15}.get(kind, (27 - golomb_params(M or 1)[0]) * (M or 1))
    assert 24 <= codeword(kind, M, x)[1] <= 32
    return x


def stream_of(kind, M, target, seed):
    """values whose codewords take exactly ``target`` bits, with a codeword of 24 bits or more across every multiple of GROUP"""
    rng = np.random.default_rng(seed)
    pool = draw(kind, M, 4096, seed)
    min_len = codeword(kind, M, 0)[1]
    values, total, boundary = [], 0, GROUP

    def add(x):
        nonlocal total
        values.append(int(x))
        total += codeword(kind, M, int(x))[1]

    while total + 70 < target:
        if total + 70 >= boundary and boundary + 40 < target:
            while total <= boundary - 24:
                add(0)
            add(long_value(kind, M))
            assert total > boundary
            boundary += GROUP
        else:
            add(pool[rng.integers(pool.size)])
    while target - total > 32:
        add(0)
    left = target - total
    if kind == "golomb":
        add((left - min_len) * M)
    else:
        for _ in range(left // min_len):
            add(0)
    assert total == target, (kind, M, target, total)
    return np.array(values, np.int64)


@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_workgroup_edges(kind, M):
    """the result equals the sequential decode whatever the passes had to correct; a codeword across a workgroup boundary
    moves the next workgroup's start, so streams past one workgroup report a pass"""
    code = UintCode(kind, M)
    for target in (GROUP - 1, GROUP, GROUP + 1, 100000):
        if kind == "universal":
            target += target & 1  # its lengths are even: 32 768, 32 768, 32 770
        values = stream_of(kind, M, target, target)
        bits, ends = encode_bits(kind, M, values)
        assert bits.size == target
        for off in (0, 13):
            got = check_decode(code, kind, M, bits, target, values.size, f"{kind}{M}/{target}@{off}", off,
                               want=(values.astype(np.uint32), target, 0))
            if target <= GROUP:
                assert got[4] == 0  # one workgroup: no pass behind the first
            elif target == 100000:  # a codeword lies across every boundary: the guess of the workgroup behind it is wrong
                assert not {GROUP, 2 * GROUP, 3 * GROUP} & set(ends.tolist())
                assert got[4] >= 1
        if target == 100000:  # cut inside the codeword across the last boundary, and inside the last one
            across = int(np.searchsorted(ends, 3 * GROUP, side="right"))
            inside = int(ends[across]) - 1
            for cut in (3 * GROUP - 1, min(3 * GROUP + 1, inside), inside, target - 1):
                want = decode_stream(kind, M, bits, nbits=cut, cap=values.size)
                assert want[2] == ST_TRUNCATED or cut == target - 1  # (the last codeword may be a single bit)
                check_decode(code, kind, M, bits, cut, values.size, f"{kind}{M}/cut{cut}", 0, want=want)


# ---- 5. damaged streams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_truncated_at_every_bit(kind, M):
    """in_nbits cut inside the unary part, the length field, the remainder, Golomb's extra bit: TRUNCATED, consumed at the
    codeword's start, the whole values in front of it delivered"""
    code = UintCode(kind, M)
    b, cutoff = golomb_params(M) if kind == "golomb" else (0, 0)
    values = [5 * (M or 1) + (M or 1) - 1, 0, 3 * (M or 1) + max(cutoff - 1, 0), long_value(kind, M), 1, 2 * (M or 1) + (M or 1) // 2]
    bits, ends = encode_bits(kind, M, values)
    met = set()
    for cut in range(1, bits.size + 1):
        want = decode_stream(kind, M, bits, nbits=cut, cap=len(values))
        check_decode(code, kind, M, bits, cut, len(values), f"{kind}{M}/cut{cut}", 3, want=want)
        met.add(want[2])
        if want[2] == ST_TRUNCATED:
            assert want[1] == max([0] + [int(e) for e in ends if e <= cut])
    assert met == {0, ST_TRUNCATED}


@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_over_long_prefix_is_size(kind, M):
    """a prefix that announces more than 32 bits, alone and behind two workgroups of good codewords"""
    code = UintCode(kind, M)
    b, cutoff = golomb_params(M) if kind == "golomb" else (0, 0)
    too_long = {"universal": 1 << 16, "elias_delta": (1 << 24) - 1}.get(kind, (32 - b) * (M or 1))
    assert codeword(kind, M, too_long)[1] > 32
    for front in (np.array([3, 0, 7], np.int64), stream_of(kind, M, 2 * GROUP + 500, 9)):
        bits, ends = encode_bits(kind, M, list(front) + [too_long, 1, 2])
        want = decode_stream(kind, M, bits, cap=front.size + 3)
        assert (len(want[0]), want[1], want[2]) == (front.size, int(ends[front.size - 1]), ST_SIZE)
        check_decode(code, kind, M, bits, bits.size, front.size + 3, f"{kind}{M}/long{front.size}", 0, want=want)
    # the run of the prefix alone: 40 ones (Elias-delta: zeros) and more of the stream in sight
    run = np.full(40, 0 if kind == "elias_delta" else 1, np.uint8)
    bits = np.concatenate([encode_bits(kind, M, [4])[0], run, 1 - run[:8]])
    want = decode_stream(kind, M, bits, cap=9)
    assert want[2] == ST_SIZE and len(want[0]) == 1
    check_decode(code, kind, M, bits, bits.size, 9, f"{kind}{M}/run", 0, want=want)


@pytest.mark.parametrize("kind,M", [CODES[3], CODES[4], CODES[7], CODES[8]], ids=[CODE_IDS[i] for i in (3, 4, 7, 8)])
def test_out_cap_below_the_count(kind, M):
    code = UintCode(kind, M)
    values = draw(kind, M, 2 * TILE + 77, 3)
    bits, ends = encode_bits(kind, M, values)
    assert bits.size > GROUP
    n = values.size
    for cap in (n - 1, n // 2, 1, 0):
        want = (values[:cap].astype(np.uint32), int(ends[cap - 1]) if cap else 0, ST_CAPACITY)
        check_decode(code, kind, M, bits, bits.size, cap, f"{kind}{M}/cap{cap}", 5, want=want)
    got = check_decode(code, kind, M, bits, bits.size, n + 100, f"{kind}{M}/roomy", 5, want=(values.astype(np.uint32), int(bits.size), 0))
    assert got[1] == n


@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_encode_refuses_without_storing(kind, M):
    """out_cap_bytes one byte short: CAPACITY and the length needed; one value above the limit in the last tile: SIZE and
    nbits 0.  Either way no codeword reaches the output: it holds the zeros the call lays down, the filler behind them"""
    code = UintCode(kind, M)
    values = draw(kind, M, 2 * TILE + 100, 4)
    bits, _ = encode_bits(kind, M, values)
    nbytes = (bits.size + 7) // 8
    for cap in (nbytes - 1, (nbytes - 1) // 4 * 4, 5):
        raw, nbits, status = block_encode(code, values, cap, f"{kind}{M}/short{cap}")
        assert (nbits, status) == (bits.size, ST_CAPACITY)
        assert not raw[:cap].any() and (raw[cap:] == FILL).all()
    b, cutoff = golomb_params(M) if kind == "golomb" else (0, 0)
    bad = values.copy()
    bad[-3] = {"universal": 1 << 16, "elias_delta": (1 << 24) - 1}.get(kind, (32 - b) * (M or 1))
    raw, nbits, status = block_encode(code, bad, nbytes + 64, f"{kind}{M}/size")
    assert (nbits, status) == (0, ST_SIZE)
    assert not raw[:nbytes + 64].any()
    bad[0] = (1 << 32) - 1  # and the largest uint32, in the first tile
    assert block_encode(code, bad, nbytes + 64, f"{kind}{M}/size2")[1:] == (0, ST_SIZE)


@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_encode_size_and_capacity_at_once(kind, M):
    """a value without a codeword of 32 bits in the last tile and five bytes of room: SIZE stops the coding, so nbits is 0
    and the capacity is never looked at -- not CAPACITY, not both"""
    code = UintCode(kind, M)
    b, cutoff = golomb_params(M) if kind == "golomb" else (0, 0)
    bad = draw(kind, M, 2 * TILE + 100, 4)
    bad[-3] = {"universal": 1 << 16, "elias_delta": (1 << 24) - 1}.get(kind, (32 - b) * (M or 1))
    raw, nbits, status = block_encode(code, bad, 5, f"{kind}{M}/size+capacity")
    assert (nbits, status) == (0, ST_SIZE)
    assert not raw[:5].any() and (raw[5:] == FILL).all()


@pytest.mark.parametrize("kind,M", CODES, ids=CODE_IDS)
def test_exact_fit_through_the_tail_word(kind, M):
    """out_cap_bytes = the stream's bytes, 1, 2 and 3 mod 4: the last word reaches the output through the tail kernel, byte
    by byte, and the byte behind the cap stays; the decoder then reads the same bytes with in_size_bytes cutting its last
    word (the byte-wise tail of its window)"""
    code = UintCode(kind, M)
    dev = device()
    values = draw(kind, M, 2 * TILE + 60, 8)
    bits, ends = encode_bits(kind, M, values)
    nbytes = (ends + 7) // 8
    for r in (1, 2, 3):
        hits = np.nonzero(nbytes[2 * TILE:] % 4 == r)[0]
        assert hits.size, f"no prefix of {r} mod 4 bytes"
        n = 2 * TILE + int(hits[-1]) + 1
        nbits = int(ends[n - 1])
        cap = (nbits + 7) // 8
        assert cap % 4 == r
        arena = Arena(cap + 4 * GUARD, dev)
        out = arena.take(cap, align=4)  # the guard starts at the byte behind the cap
        meta = code.encode_block_into(value_tensor(values[:n], dev), out, out_cap_bytes=cap)
        torch.cuda.synchronize()
        arena.check(f"{kind}{M}/fit{r}")
        assert tuple(int(v) for v in meta.cpu()) == (nbits, 0)
        assert np.array_equal(out.cpu().numpy(), pack(bits[:nbits]))
        assert out.numel() == cap
        got = block_decode(code, out, 0, nbits, n, f"{kind}{M}/fit{r}/decode")
        assert got[1:4] == (n, nbits, 0) and np.array_equal(got[0], values[:n].astype(np.uint32))


# ---- 6. scratch reused from a larger block ---------------------------------------------------------------------------------------
def test_scratch_reused_from_a_larger_block():
    dev = device()
    kind, M = "golomb", 10
    code = UintCode(kind, M)
    large, small = draw(kind, M, 5 * TILE + 3, 6), draw(kind, M, TILE + 9, 7)
    nbytes = int(code._L.scl_uint_block_scratch_bytes(large.size, 32 * large.size))
    scratch = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    for values in (large, small, large[:17], small):
        want, _ = encode_bits(kind, M, values)
        out = torch.full((4 * values.size + 16,), FILL, dtype=torch.uint8, device=dev)
        nbits, status = (int(v) for v in code.encode_block_into(value_tensor(values, dev), out, scratch=scratch).cpu())
        assert (nbits, status) == (want.size, 0)
        assert np.array_equal(out.cpu().numpy()[:(nbits + 7) // 8], pack(want))
        got, n_out, consumed, status, _ = code.decode_block_device(out, nbits, scratch=scratch)
        assert (n_out, consumed, status) == (values.size, nbits, 0)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), values.astype(np.uint32))


# ---- 7. the classes, end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("golomb", 6), ("universal", None), ("elias_delta", None)], ids=["golomb6", "universal", "elias"])
def test_class_round_trip_of_a_geometric_block(kind, M):
    values = geometric(1 << 20, 8.0, seed=20)
    assert values.size >= _uint_block.UINT_BLOCK_MIN
    enc, dec = coders(kind, M)
    taken = []
    real = UintCode.encode_host

    def spy(self, v):
        taken.append(len(v))
        return real(self, v)

    UintCode.encode_host = spy
    try:
        ok, used, bits = try_lossless_compression(DataBlock(values.tolist()), enc, dec)
    finally:
        UintCode.encode_host = real
    assert ok and taken == [values.size]  # the device coded it
    head = 4096  # the first values, against the restatement
    want, ends = encode_bits(kind, M, values[:head])
    assert np.array_equal(bits._b[:want.size], want)
    assert used == len(bits)


def test_class_falls_back_to_the_host_for_long_codewords(monkeypatch):
    """a block the device answers with SIZE, and one with a value of 2^32: the host's bits, the same as the symbol calls"""
    monkeypatch.setattr(_uint_block, "UINT_BLOCK_MIN", 64)
    for kind, M in (("golomb", 10), ("universal", None), ("elias_delta", None)):
        enc, dec = coders(kind, M)
        for extra in (1 << 26, (1 << 32) + 1):
            if kind == "golomb":
                extra = 400 + (extra >> 26)  # 41 and more ones
            values = list(range(100)) + [extra] + list(range(50))
            bits = enc.encode_block(DataBlock(values))
            want, _ = encode_bits(kind, M, values)
            assert np.array_equal(bits._b, want)
            block, used = dec.decode_block(bits)
            assert block.data_list == values and used == want.size
    enc, dec = coders("golomb", 10)
    bits = enc.encode_block(DataBlock(list(range(200))))
    with pytest.raises(Exception) as err:
        dec.decode_block(BitArray._wrap(bits._b[:-2].copy()))
    assert "TRUNCATED" in str(err.value)
