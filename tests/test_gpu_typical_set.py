"""The typical-set coder on the device (csrc/scl_typical.hip): the tables the three kernels build against the rule on the CPU,
the classes against the reference's goldens, and the block coder against the restatement of tests/typical_set_helpers.py --
the bits, the symbols, and for damaged streams the (symbols, consumed, status) of the sequential decoder.  Sizes sit on the
kernels' edges: a table tile is 4096 tuples; an encoder tile is 4096 chunks, 16 a thread; a decoder thread owns 128 bits, a
decoder workgroup 32 768.  No test provokes a GPU fault: damaged streams are valid memory with wrong bits, under guard bands."""
import random

import numpy as np
import pytest

from conftest import golden_ids
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import TypicalSetModel
from stanford_compression_library_amd.compressors.typical_set_coder import (TypicalSetCoderParams, TypicalSetDecoder,
                                                                            TypicalSetEncoder, is_typical)
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist
from stanford_compression_library_amd.utils.bitarray_utils import BitArray
from stanford_compression_library_amd.utils.test_utils import get_random_data_block, try_lossless_compression
from typical_set_helpers import (ALL_ATYPICAL, COPRIME, EQUAL_LENGTHS, GOLDENS, GROUP, NONE, NOT_POWER_OF_TWO, ONE_BIT,
                                 SHARED_GCD, ST_CAPACITY, ST_STATE, ST_SYMBOL, ST_TRUNCATED, SUB, TABLE_TILE, TILE, decode_stream,
                                 encode_bits, golden_dist, golden_flags, golden_model, host_tables, mixed_block, pack, tables_of)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5


def device():
    return torch.device("cuda:0")


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


# ---- 1. the tables, white box --------------------------------------------------------------------------------------------------
def check_tables(model_args, what):
    """the device tables of a model against scl_typical_table_host, the failure naming the stage that differs"""
    nlp, n, entropy, eps = model_args
    want_rank, want_count = TypicalSetModel.table_host(nlp, n, entropy, eps)
    model = TypicalSetModel(nlp, n, entropy, eps)
    info = model.info()
    assert (info.K, info.n, info.N) == (len(nlp), n, len(nlp) ** n), what
    assert info.count == want_count, f"{what}: stage count: {info.count} typical tuples, the host rule finds {want_count}"
    rank, inv = model.tables()
    assert rank.size == info.N and inv.size == want_count
    flags, want_flags = rank != NONE, want_rank != NONE
    assert np.array_equal(flags, want_flags), \
        f"{what}: stage rank: {int((flags != want_flags).sum())} tuples classified differently, first {int(np.flatnonzero(flags != want_flags)[0])}"
    assert np.array_equal(rank, want_rank), \
        f"{what}: stage scan: the flags agree, the numbers differ first at tuple {int(np.flatnonzero(rank != want_rank)[0])}"
    assert np.array_equal(inv, np.flatnonzero(want_flags).astype(np.uint32)), f"{what}: stage inverse"
    bt = backend_lib.load().scl_typical_index_bits_host(want_count)
    assert (info.bt, info.bo) == (bt, backend_lib.load().scl_typical_index_bits_host(info.N)), what
    assert (model.bt is None) == (want_count == 0)
    model.close()
    return want_count


@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_tables_equal_the_host_rule_at_every_golden(case):
    assert check_tables(golden_model(case), repr(case)) == case.count


def random_model(K, n, eps, seed):
    """nlp of K random symbols and a window around their mean, which is the mean of s / n over all tuples; ``eps`` in units of
    the standard deviation of s / n there (-1 and 2 as they are: the empty and the full set), so that half a deviation holds
    a part of the tuples, not all"""
    nlp = np.random.default_rng(seed).random(K) * 2.0
    return nlp, n, float(nlp.mean()), eps if eps in (-1.0, 2.0) else eps * float(nlp.std()) / np.sqrt(n)


TABLE_SIZES = [(1, 1), (2, 1), (TABLE_TILE - 1, 1), (TABLE_TILE, 1), (TABLE_TILE + 1, 1), (3, 10), (7, 5), (4096, 2), (256, 3),
               (2, 24), (65536, 1)]


@pytest.mark.parametrize("K,n", TABLE_SIZES, ids=[f"{K}^{n}" for K, n in TABLE_SIZES])
def test_tables_equal_the_host_rule_at_the_tile_edges_and_the_cap(K, n):
    count = check_tables(random_model(K, n, 0.5, K + n), f"{K}^{n}")
    assert K ** n < 4 or 0 < count < K ** n, "the window holds some tuples and not all"
    if K ** n <= 1 << 16 or (K, n) == (4096, 2):  # (at the cap: a full set is an inverse of 2^24 entries, bt = 24)
        assert check_tables(random_model(K, n, -1.0, 1), f"{K}^{n}/empty") == 0
        assert check_tables(random_model(K, n, 2.0, 2), f"{K}^{n}/full") == K ** n


# ---- 2. the classes --------------------------------------------------------------------------------------------------------------
def coders_of(case):
    dist = ProbabilityDist(golden_dist(case))
    params = TypicalSetCoderParams(case.n, case.eps, dist)
    return dist, TypicalSetEncoder(params), TypicalSetDecoder(params)


@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_classes_give_the_golden_bits_and_decode_them(case):
    dist, enc, dec = coders_of(case)
    assert enc.index_bitlen_typical == (None if case.bt < 0 else case.bt) == dec.index_bitlen_typical
    assert enc.index_bitlen_overall == case.bo == dec.index_bitlen_overall
    assert enc._model.wide == (case.K > 256)
    alphabet = dist.alphabet
    data = [alphabet[i] for i in case.arr("data").tolist()]
    bits = enc.encode_block(DataBlock(data))
    assert len(bits) == case.nbits and np.array_equal(bits.packed(), case.arr("out"))
    back, used = dec.decode_block(bits)
    assert back.data_list == data and used == len(bits)
    if case.K ** case.n <= 729:  # the views of the device tables are the reference's four dicts
        flags = golden_flags(case)
        chunks = list(enc.index_overall)
        assert [enc.index_overall[c] for c in chunks] == list(range(len(chunks)))
        assert [c in enc.index_typical for c in chunks] == flags.tolist()
        assert dec.inverse_index_typical == {i: c for c, i in enc.index_typical.items()}
        assert dec.inverse_index_overall == dict(enumerate(chunks))


def test_classes_edges_and_errors():
    dist = ProbabilityDist({"A": 0.6, "B": 0.3, "C": 0.1})
    params = TypicalSetCoderParams(3, 0.2, dist)  # 3 typical chunks of 27: two index bits, of which 11 names none
    enc, dec = TypicalSetEncoder(params), TypicalSetDecoder(params)
    assert len(enc.encode_block(DataBlock([]))) == 0
    back, used = dec.decode_block(BitArray(""))
    assert back.data_list == [] and used == 0
    with pytest.raises(AssertionError):
        enc.encode_block(DataBlock(["A", "B"]))
    with pytest.raises(KeyError):
        enc.encode_block(DataBlock(["A", "B", "Z"]))
    bits = enc.encode_block(DataBlock(list("ABAAACCCCAAB")))
    with pytest.raises(backend_lib.SclHipError, match="TRUNCATED"):
        dec.decode_block(BitArray._wrap(bits._b[:-1].copy()))
    bt, bo = enc.index_bitlen_typical, enc.index_bitlen_overall
    count = len(enc.index_typical)
    assert 0 < count < (1 << bt) and 27 < (1 << bo)
    with pytest.raises(KeyError):  # a typical index outside the set
        dec.decode_block(bits + BitArray("0" + "1" * bt))
    with pytest.raises(backend_lib.SclHipError, match="STATE"):  # an overall index of K^n and more
        dec.decode_block(bits + BitArray("1" + "1" * bo))
    empty = TypicalSetCoderParams(3, -1.0, dist)
    assert TypicalSetEncoder(empty).index_bitlen_typical is None
    with pytest.raises(backend_lib.SclHipError, match="STATE"):  # flag 0 with an empty typical set
        TypicalSetDecoder(empty).decode_block(BitArray("0" * 8))


REFERENCE_DISTS = [{"A": 0.6, "B": 0.3, "C": 0.1}, {"A": 0.6, "B": 0.4}, {"A": 0.99, "B": 0.01}, {"A": 1}]


@pytest.mark.parametrize("prob_dict", REFERENCE_DISTS, ids=["abc631", "ab64", "ab99", "a1"])
def test_typical_set_coder_roundtrip(prob_dict):
    """the reference's test_typical_set_coder_roundtrip, one distribution a case"""
    prob_dist = ProbabilityDist(prob_dict)
    for eps in [0.0, 0.01, 0.1, 0.2, 2.0]:
        for n in [1, 3, 6, 10]:
            data_block = get_random_data_block(prob_dist, 1000 * n, seed=0)
            params = TypicalSetCoderParams(n, eps, prob_dist)
            is_lossless, _, _ = try_lossless_compression(data_block, TypicalSetEncoder(params), TypicalSetDecoder(params))
            assert is_lossless, "Lossless compression failed"


def test_is_typical():
    """the reference's test_is_typical"""
    prob_dist = ProbabilityDist({"A": 0.6, "B": 0.3, "C": 0.1})
    eps = 0.01
    n = 30
    chunk = ["A"] * n
    assert is_typical(chunk, prob_dist, eps) == False  # noqa: E712
    num_As = int(0.7 * n)
    num_Cs = n - num_As
    chunk = ["A"] * num_As + ["C"] * num_Cs
    assert is_typical(chunk, prob_dist, eps) == False  # noqa: E712
    random.shuffle(chunk)
    assert is_typical(chunk, prob_dist, eps) == False  # noqa: E712
    random.shuffle(chunk)
    assert is_typical(chunk, prob_dist, eps) == False  # noqa: E712
    num_As = int(0.6 * n)
    num_Bs = int(0.3 * n)
    num_Cs = n - num_As - num_Bs
    chunk = ["A"] * num_As + ["B"] * num_Bs + ["C"] * num_Cs
    assert is_typical(chunk, prob_dist, eps) == True  # noqa: E712
    random.shuffle(chunk)
    assert is_typical(chunk, prob_dist, eps) == True  # noqa: E712
    random.shuffle(chunk)
    assert is_typical(chunk, prob_dist, eps) == True  # noqa: E712


# ---- 3. the block coder through device tensors -----------------------------------------------------------------------------------
class Coder:
    """a device model and the restated tables of the same inputs"""

    def __init__(self, model_args):
        self.model = TypicalSetModel(*model_args)
        self.K, self.n, self.rank, self.inv, self.bt, self.bo = host_tables(model_args)
        assert (self.model.bt, self.model.bo, self.model.count) == (self.bt, self.bo, len(self.inv))

    def sym_tensor(self, idx):
        a = np.ascontiguousarray(idx, dtype=self.model.sym_dtype)
        return torch.from_numpy(a.view(np.int16) if self.model.wide else a).to(device())

    def bits_of(self, idx):
        return encode_bits(idx, self.K, self.n, self.rank, self.bt, self.bo)

    def sequential(self, bits, nbits, cap_symbols):
        return decode_stream(bits, nbits, self.K, self.n, self.inv, self.bt, self.bo, cap_symbols)


def block_encode(coder, idx, cap, what, scratch=None):
    """the code under test, its output between guard bands -> (the bytes of the whole buffer, nbits, status)"""
    arena = Arena(cap + 4 * GUARD, device())
    out = arena.take(max(cap, 4), align=4)
    meta = coder.model.encode_block_into(coder.sym_tensor(idx), out, out_cap_bytes=cap, scratch=scratch)
    torch.cuda.synchronize()
    arena.check(what)
    nbits, status = (int(v) for v in meta.cpu())
    return out.cpu().numpy(), nbits, status & 0xFFFFFFFF


def check_encode(coder, idx, what, want_idx=None, want_status=0):
    want_bits, _ = coder.bits_of(idx if want_idx is None else want_idx)
    want, nbits = pack(want_bits), int(want_bits.size)
    nbytes = (nbits + 7) // 8
    chunks = len(idx) // coder.n
    reach = ((chunks * (1 + coder.bo) + 7) // 8 + 3) // 4 * 4  # the call zeroes its output up to the longest possible stream
    for cap in sorted({nbytes, (nbytes + 3) // 4 * 4, nbytes + 7, reach + 61}):  # a multiple of 4 and not, exact and roomy
        raw, got_bits, status = block_encode(coder, idx, cap, f"{what}/cap{cap}")
        assert (got_bits, status) == (nbits, want_status), (what, cap)
        assert np.array_equal(raw[:nbytes], want), (what, cap)
        assert not raw[nbytes:min(reach, cap)].any(), (what, cap)
        assert (raw[reach:cap] == FILL).all(), (what, cap)  # nothing is touched behind what the call may zero
    return want_bits


def stream_at(bits, bit_offset):
    """the bits at bit ``bit_offset`` of a device buffer, ones in front and behind"""
    body = pack(np.concatenate([np.ones(bit_offset & 7, np.uint8), bits, np.ones(77, np.uint8)]))
    return torch.from_numpy(np.concatenate([np.full(bit_offset >> 3, 0xFF, np.uint8), body])).to(device())


def block_decode(coder, data, bit_offset, nbits, cap, what, scratch=None):
    """the code under test, its output between guard bands -> (symbols, n_out, consumed, status, sync_passes)"""
    size = np.dtype(coder.model.sym_dtype).itemsize
    arena = Arena(max(cap, 1) * size + 4 * GUARD, data.device)
    out = arena.take(max(cap, 1) * size, torch.int16 if coder.model.wide else torch.uint8)
    _, n_out, consumed, status, passes = coder.model.decode_block_device(data, nbits, bit_offset, out_cap=cap, out=out,
                                                                         scratch=scratch)
    torch.cuda.synchronize()
    arena.check(what)
    assert n_out <= cap and n_out % coder.n == 0, what
    raw = out.view(torch.uint8).cpu().numpy()
    assert (raw[n_out * size:] == FILL).all(), f"{what}: symbols stored behind n_out"
    return raw[:n_out * size].view(coder.model.sym_dtype), n_out, consumed, status, passes


def check_decode(coder, bits, nbits, cap, what, bit_offset=0, want=None):
    """the device against the sequential decoder, field for field"""
    if want is None:
        want = coder.sequential(bits, nbits, cap)
    got = block_decode(coder, stream_at(bits, bit_offset), bit_offset, nbits, cap, what)
    assert np.array_equal(got[0], want[0]), what
    assert (got[1], got[2], got[3]) == (len(want[0]), want[1], want[2]), (what, got[1:], want[1:])
    return got


EDGE_CHUNKS = (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, SUB - 1, SUB + 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1)


@pytest.mark.parametrize("model_args,bit", [(ONE_BIT, 0), (ALL_ATYPICAL, 1)], ids=["one_typical", "all_atypical"])
def test_block_edges_with_one_bit_a_chunk(model_args, bit):
    """{A: 1}, n = 1 codes one bit a chunk, so the chunk counts set the stream lengths exactly: both sides of an encoder
    tile, of a decoder thread's 128 bits and of a decoder workgroup's 32 768"""
    coder = Coder(model_args)
    for chunks in EDGE_CHUNKS:
        idx = np.zeros(chunks, np.int64)
        what = f"{chunks} chunks of bit {bit}"
        if chunks == 0:
            raw, nbits, status = block_encode(coder, idx, 8, what)
            assert (nbits, status) == (0, 0) and (raw == FILL).all()
            for off in (0, 5):
                assert block_decode(coder, stream_at(np.zeros(0, np.uint8), off), off, 0, 4, what)[1:4] == (0, 0, 0)
            continue
        bits = check_encode(coder, idx, what)
        assert bits.size == chunks and (bits == bit).all()
        for off in (0, 5):
            got = check_decode(coder, bits, chunks, chunks, f"{what}@{off}", off, want=(idx, chunks, 0))
            assert got[4] == 0  # every bit is a codeword start: the first pass is exact


@pytest.mark.parametrize("name,model_args", [("equal", EQUAL_LENGTHS), ("gcd4", SHARED_GCD), ("coprime", COPRIME),
                                             ("k3", NOT_POWER_OF_TWO)])
def test_blocks_that_mix_both_flags(name, model_args):
    coder = Coder(model_args)
    for chunks in (1, 15, 17, TILE + 1, 3 * TILE + 5):
        idx = mixed_block(model_args, chunks)
        bits = check_encode(coder, idx, f"{name}/{chunks}")
        for off in (0, 13):
            got = check_decode(coder, bits, bits.size, idx.size, f"{name}/{chunks}@{off}", off, want=(idx, int(bits.size), 0))
            if name == "equal":
                assert got[4] == 0  # one length: pass 0 starts every thread on a codeword
    assert bits.size > GROUP  # the largest block spans decoder workgroups


# ---- 4. faults -------------------------------------------------------------------------------------------------------------------
def test_a_cut_codeword_is_truncated():
    coder = Coder(COPRIME)
    idx = mixed_block(COPRIME, 2 * TILE + 77, seed=3)
    bits, ends = coder.bits_of(idx)
    assert bits.size > GROUP
    for cut in (int(ends[-1]) - 1, int(ends[-2]) + 1, int(ends[4000]) + 2, 3, 1):
        want = coder.sequential(bits, cut, idx.size)
        assert want[2] == ST_TRUNCATED and want[1] == max([0] + [int(e) for e in ends if e <= cut][-1:])
        check_decode(coder, bits, cut, idx.size, f"cut{cut}", 5, want=want)
    # whole codewords of one length up to the cut: the default capacity is not reached either (TRUNCATED, not CAPACITY)
    equal = Coder(EQUAL_LENGTHS)
    idx = mixed_block(EQUAL_LENGTHS, 3)
    bits, _ = equal.bits_of(idx)
    back, used, status = equal.model.decode_host(pack(bits[:-1]), bits.size - 1)
    assert (used, status) == (10, ST_TRUNCATED) and np.array_equal(back, idx[:8])


def test_state_at_the_sequentially_first_bad_codeword():
    as_bits = lambda s: np.array(list(map(int, s)), np.uint8)  # noqa: E731
    k3 = Coder(NOT_POWER_OF_TWO)
    assert (k3.bt, k3.bo, len(k3.inv)) == (3, 5, 7)
    bad = {"typical index >= count": as_bits("0111"), "overall index >= N": as_bits("111011"),
           "overall index 31": as_bits("111111")}
    for front_chunks in (3, 2 * TILE + 9):
        front = mixed_block(NOT_POWER_OF_TWO, front_chunks, seed=5)
        good, ends = k3.bits_of(front)
        for what, word in bad.items():
            bits = np.concatenate([good, word, good[:int(ends[1])], bad["overall index 31"], good[:int(ends[0])]])
            want = k3.sequential(bits, bits.size, front.size + 40)
            assert (want[1], want[2]) == (good.size, ST_STATE) and np.array_equal(want[0], front)
            check_decode(k3, bits, bits.size, front.size + 40, f"{what}/{front_chunks}", 3, want=want)
    none = Coder(ALL_ATYPICAL)
    for ones in (0, 5, GROUP + 17):
        bits = np.concatenate([np.ones(ones, np.uint8), as_bits("0"), np.ones(9, np.uint8)])
        want = (np.zeros(ones, np.int64), ones, ST_STATE)
        check_decode(none, bits, bits.size, bits.size, f"flag 0 on an empty set behind {ones}", 0, want=want)


def test_a_symbol_outside_the_alphabet_is_coded_as_symbol_0():
    coder = Coder(NOT_POWER_OF_TWO)
    idx = mixed_block(NOT_POWER_OF_TWO, 2 * TILE + 9, seed=6)
    for at in (0, idx.size - 2):
        bad = idx.copy()
        bad[at] = 3 if at else 255
        clean = idx.copy()
        clean[at] = 0
        check_encode(coder, bad, f"symbol {bad[at]} at {at}", want_idx=clean, want_status=ST_SYMBOL)
    wide = Coder(golden_model(next(c for c in GOLDENS if c.group == "k300" and c.n == 2)))
    idx = np.array([5, 299, 300, 7, 65535, 0], np.int64)
    check_encode(wide, idx, "uint16 symbols 300 and 65535", want_idx=np.array([5, 299, 0, 7, 0, 0]), want_status=ST_SYMBOL)


def test_out_cap_short_of_the_stream():
    coder = Coder(SHARED_GCD)
    idx = mixed_block(SHARED_GCD, 2 * TILE + 77, seed=7)
    n = coder.n
    bits, ends = coder.bits_of(idx)
    chunks = idx.size // n
    for cap_chunks in (chunks - 1, chunks // 2, 1, 0):
        for spare in (0, n - 1):  # out_cap counts symbols: a part of a chunk holds none
            cap = cap_chunks * n + spare
            want = (idx[:cap_chunks * n], int(ends[cap_chunks - 1]) if cap_chunks else 0, ST_CAPACITY)
            check_decode(coder, bits, bits.size, cap, f"cap {cap_chunks} chunks + {spare}", 5, want=want)
    got = check_decode(coder, bits, bits.size, idx.size + 100, "roomy", 5, want=(idx, int(bits.size), 0))
    assert got[1] == idx.size
    nbytes = (bits.size + 7) // 8
    for cap in (nbytes - 1, (nbytes - 1) // 4 * 4, 5):  # the encoder: CAPACITY, the length needed, nothing stored
        raw, nbits, status = block_encode(coder, idx, cap, f"short{cap}")
        assert (nbits, status) == (bits.size, ST_CAPACITY)
        assert not raw[:cap].any() and (raw[cap:] == FILL).all()


# ---- 5. buffers and conventions --------------------------------------------------------------------------------------------------
def test_scratch_reused_from_a_larger_call():
    coder = Coder(COPRIME)
    large, small = mixed_block(COPRIME, 5 * TILE + 3, seed=8), mixed_block(COPRIME, TILE + 9, seed=9)
    nbytes = int(coder.model._L.scl_typical_block_scratch_bytes(coder.model._h, large.size, (large.size // coder.n) * 7))
    scratch = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=device())
    for idx in (large, small, large[:17 * coder.n], small):
        want, _ = coder.bits_of(idx)
        raw, nbits, status = block_encode(coder, idx, (want.size + 7) // 8 + 9, "reuse", scratch=scratch)
        assert (nbits, status) == (want.size, 0) and np.array_equal(raw[:(nbits + 7) // 8], pack(want))
        got = block_decode(coder, stream_at(want, 3), 3, nbits, idx.size, "reuse", scratch=scratch)
        assert got[1:4] == (idx.size, nbits, 0) and np.array_equal(got[0], idx)


def test_uint16_symbols_through_the_block_calls():
    """300 symbols: the indices travel as uint16, the host calls and the device calls alike"""
    for case in (c for c in GOLDENS if c.group == "k300"):
        coder = Coder(golden_model(case))
        assert coder.model.wide and coder.model.sym_dtype == np.uint16
        idx = case.arr("data").astype(np.int64)
        bits = check_encode(coder, idx, repr(case))
        assert np.array_equal(pack(bits), case.arr("out"))
        check_decode(coder, bits, bits.size, idx.size, repr(case), 11, want=(idx, int(bits.size), 0))
        packed, nbits, status = coder.model.encode_host(idx)
        assert (nbits, status) == (case.nbits, 0) and np.array_equal(packed, case.arr("out"))
        back, used, status = coder.model.decode_host(packed, nbits)
        assert (used, status) == (nbits, 0) and np.array_equal(back, idx)


def test_entry_points_refuse_before_the_device():
    """a block that is no whole number of chunks, a uint8 call on a wide model, a scratch that is too small"""
    L = backend_lib.load()
    coder = Coder(COPRIME)
    dev = device()
    sym = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.zeros(256, dtype=torch.uint8, device=dev)
    meta = torch.zeros(4, dtype=torch.int64, device=dev)
    scratch = coder.model.block_scratch(60, 1024, dev)
    h = coder.model._h

    def encode(n_symbols, scratch_bytes):
        return L.scl_typical_encode_block(h, sym.data_ptr(), n_symbols, out.data_ptr(), 256, meta.data_ptr(),
                                          meta.data_ptr() + 8, scratch.data_ptr(), scratch_bytes, None)

    assert encode(61, scratch.numel()) == backend_lib.E_PARAM and "multiple of the chunk length" in backend_lib.last_error()
    assert encode(60, 8) == backend_lib.E_PARAM and "scratch" in backend_lib.last_error()
    assert L.scl_typical_decode_block(h, out.data_ptr(), 256, 0, 1024, sym.data_ptr(), 64, meta.data_ptr(), scratch.data_ptr(),
                                      1024, None) == backend_lib.E_PARAM
    assert "scratch" in backend_lib.last_error()
    wide = Coder(golden_model(next(c for c in GOLDENS if c.group == "k300" and c.n == 1)))
    assert L.scl_typical_encode_block(wide.model._h, sym.data_ptr(), 60, out.data_ptr(), 256, meta.data_ptr(),
                                      meta.data_ptr() + 8, scratch.data_ptr(), scratch.numel(), None) == backend_lib.E_PARAM
    assert "_u16" in backend_lib.last_error()
    torch.cuda.synchronize()
