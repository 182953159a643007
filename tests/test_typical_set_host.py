"""The typical-set coder without a device: the package's ProbabilityDist against the goldens' float64 inputs, the rule on the
CPU (``scl_typical_table_host``) and its numpy restatement against every golden set, the four misreadings told apart, the
index widths, the restated coder against the goldens' bits, the refused parameters, and the properties of the builders that
tests/test_gpu_typical_set.py relies on."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_ids
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import TypicalSetModel
from stanford_compression_library_amd.compressors import typical_set_coder as tsc
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist
from typical_set_helpers import (ALL_ATYPICAL, COPRIME, EQUAL_LENGTHS, GOLDENS, GROUP, MISREADINGS, NONE, NOT_POWER_OF_TWO,
                                 ONE_BIT, SHARED_GCD, SUB, TILE, ceil_log2, decode_stream, encode_bits, golden_dist,
                                 golden_flags, golden_model, host_tables, mixed_block, pack, tables_of, typical_flags, widths)


@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_prob_dist_gives_the_goldens_inputs_bit_for_bit(case):
    params = tsc.TypicalSetCoderParams(case.n, case.eps, ProbabilityDist(golden_dist(case)))
    nlp, entropy = tsc.model_inputs(params)
    assert np.array_equal(nlp.view(np.uint64), case.arr("nlp").view(np.uint64))
    assert np.array_equal(np.array([entropy], np.float64).view(np.uint64), case.arr("entropy").view(np.uint64))


@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_host_rule_and_restatement_equal_the_golden_sets(case):
    nlp, n, entropy, eps = golden_model(case)
    want = golden_flags(case)
    assert int(want.sum()) == case.count
    rank, count = TypicalSetModel.table_host(nlp, n, entropy, eps)
    assert count == case.count
    assert np.array_equal(rank != NONE, want)
    assert np.array_equal(rank, tables_of(want)[0])
    _, count_only = TypicalSetModel.table_host(nlp, n, entropy, eps, want_rank=False)
    assert count_only == case.count
    assert np.array_equal(typical_flags(nlp, n, entropy, eps), want)
    bt, bo = widths(case.count, case.K ** case.n)
    assert (-1 if bt is None else bt, bo) == (case.bt, case.bo)


@pytest.mark.parametrize("reading", MISREADINGS)
def test_every_misreading_is_told_from_the_rule_by_a_golden(reading):
    caught = [repr(c) for c in GOLDENS if c.K ** c.n <= 60000 and
              not np.array_equal(typical_flags(*golden_model(c), reading=reading), golden_flags(c))]
    print(reading, "caught by", len(caught), "goldens:", caught[:6])
    assert caught, f"no golden tells the misreading {reading!r} from the rule"


def test_index_widths_equal_the_reference_expression():
    L = backend_lib.load()
    xs = [1, 2, 3] + [v for k in range(2, 25) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    for x in xs:
        assert L.scl_typical_index_bits_host(x) == ceil_log2(x), x
    assert L.scl_typical_index_bits_host(0) == NONE


@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_restated_coder_gives_the_golden_bits(case):
    rank, inv, count = tables_of(golden_flags(case))
    bt, bo = widths(count, case.K ** case.n)
    data = case.arr("data").astype(np.int64)
    assert data.size == 200 * case.n
    bits, ends = encode_bits(data, case.K, case.n, rank, bt, bo)
    assert bits.size == case.nbits == int(ends[-1])
    assert np.array_equal(pack(bits), case.arr("out"))
    if case.id % 7 == 0:  # the sequential decoder is a Python loop: a sample of the cases
        back, used, status = decode_stream(bits, bits.size, case.K, case.n, inv, bt, bo, data.size)
        assert (used, status) == (case.nbits, 0) and np.array_equal(back, data)


def test_refused_parameters_need_no_device():
    L = backend_lib.load()
    h = C.c_void_p()
    count = C.c_uint32()

    def nlp_of(values):
        return np.ascontiguousarray(values, np.float64).ctypes.data_as(backend_lib._f64p)

    refused = [
        ("K = 0", (nlp_of([0.5]), 0, 1, 1.0, 0.1), "alphabet"),
        ("n = 0", (nlp_of([1.0, 1.0]), 2, 0, 1.0, 0.1), "chunks of 0"),
        ("K > 65536", (nlp_of(np.ones(65537)), 65537, 1, 1.0, 0.1), "65536"),
        ("K^n > 2^24", (nlp_of([1.0, 1.0]), 2, 25, 1.0, 0.1), "2^24"),
        ("K^n > 2^24, K = 4097", (nlp_of(np.ones(4097)), 4097, 2, 1.0, 0.1), "2^24"),
        ("K^n overflows 64 bits", (nlp_of(np.ones(65536)), 65536, 5, 1.0, 0.1), "2^24"),
        ("nlp = inf", (nlp_of([1.0, np.inf]), 2, 2, 1.0, 0.1), "not finite"),
        ("nlp = nan", (nlp_of([np.nan, 1.0]), 2, 2, 1.0, 0.1), "not finite"),
        ("entropy = nan", (nlp_of([1.0, 1.0]), 2, 2, np.nan, 0.1), "finite"),
        ("eps = inf", (nlp_of([1.0, 1.0]), 2, 2, 1.0, np.inf), "finite"),
    ]
    for what, args, word in refused:
        assert L.scl_typical_model_create(*args, C.byref(h)) == backend_lib.E_PARAM, what
        message = backend_lib.last_error()
        assert message.startswith("typical_model_create:") and word in message, (what, message)
        assert not h.value
        assert L.scl_typical_table_host(*args, None, C.byref(count)) == backend_lib.E_PARAM, what
        assert backend_lib.last_error().startswith("typical_table_host:")
    assert L.scl_typical_model_create(None, 2, 2, 1.0, 0.1, C.byref(h)) == backend_lib.E_PARAM
    # a negative eps is legal: the empty set
    assert L.scl_typical_table_host(nlp_of([1.0, 1.0]), 2, 3, 1.0, -1.0, None, C.byref(count)) == 0 and count.value == 0
    # 2^24 tuples exactly are taken
    assert L.scl_typical_table_host(nlp_of([1.0, 1.0]), 2, 24, 1.0, 0.0, None, C.byref(count)) == 0 and count.value == 1 << 24
    # the block entry points refuse a null model before any device call
    for name in ("scl_typical_encode_block", "scl_typical_decode_block", "scl_typical_encode_block_host",
                 "scl_typical_decode_block_host", "scl_typical_encode_block_u16", "scl_typical_decode_block_host_u16"):
        fn = getattr(L, name)
        assert fn(*[None if t is not C.c_uint64 else 0 for t in fn.argtypes]) == backend_lib.E_PARAM, name
        assert backend_lib.last_error().startswith(name[len("scl_"):] + ":"), backend_lib.last_error()
    assert L.scl_typical_block_scratch_bytes(None, 10, 10) == 0


def test_the_classes_name_the_limit_above_which_they_do_not_enumerate():
    two = ProbabilityDist({"A": 0.5, "B": 0.5})
    for Coder in (tsc.TypicalSetEncoder, tsc.TypicalSetDecoder):
        with pytest.raises(NotImplementedError, match="2\\^24"):
            Coder(tsc.TypicalSetCoderParams(25, 0.1, two))
    wide = ProbabilityDist({i: 1.0 / 65537 for i in range(65537)})
    with pytest.raises(NotImplementedError, match="65536"):
        tsc.TypicalSetEncoder(tsc.TypicalSetCoderParams(1, 0.1, wide))


def test_reference_functions_on_the_host():
    """the reference's test_is_typical, and generate_typical_set_coder_lookup_tables against a golden"""
    import random

    dist = ProbabilityDist({"A": 0.6, "B": 0.3, "C": 0.1})
    n = 30
    assert not tsc.is_typical(["A"] * n, dist, 0.01)
    chunk = ["A"] * 21 + ["C"] * 9
    for _ in range(3):
        assert not tsc.is_typical(chunk, dist, 0.01)
        random.shuffle(chunk)
    chunk = ["A"] * 18 + ["B"] * 9 + ["C"] * 3
    for _ in range(3):
        assert tsc.is_typical(chunk, dist, 0.01)
        random.shuffle(chunk)
    case = next(c for c in GOLDENS if c.group == "abc631" and c.n == 6 and c.eps == 0.1)
    typical, overall = tsc.generate_typical_set_coder_lookup_tables(tsc.TypicalSetCoderParams(6, 0.1, dist))
    flags = golden_flags(case)
    assert len(typical) == case.count and len(overall) == 3 ** 6
    chunks = list(overall)
    assert [overall[c] for c in chunks] == list(range(3 ** 6))
    assert [c in typical for c in chunks] == flags.tolist()
    assert [typical[c] for c in chunks if c in typical] == list(range(case.count))


def test_builders_have_the_properties_the_gpu_tests_rely_on():
    want = {"ONE_BIT": (ONE_BIT, 1, 1, 1, 1), "ALL_ATYPICAL": (ALL_ATYPICAL, 0, None, 1, 1),
            "EQUAL_LENGTHS": (EQUAL_LENGTHS, 14, 5, 5, 5), "SHARED_GCD": (SHARED_GCD, 7, 4, 8, 4),
            "COPRIME": (COPRIME, 6, 4, 7, 1), "NOT_POWER_OF_TWO": (NOT_POWER_OF_TWO, 7, 4, 6, 2)}
    for name, (model, count, len_t, len_o, gcd) in want.items():
        K, n, rank, inv, bt, bo = host_tables(model)
        assert len(inv) == count, name
        assert (None if bt is None else 1 + bt, 1 + bo) == (len_t, len_o), name
        assert np.gcd(len_t or len_o, len_o) == gcd, name
        # the C rule agrees with the restatement on these hand-made inputs too
        c_rank, c_count = TypicalSetModel.table_host(*model)
        assert c_count == count and np.array_equal(c_rank, rank), name
    assert 3 ** 3 < 1 << host_tables(NOT_POWER_OF_TWO)[5]  # indices 27..31 exist and are no tuples
    for model in (EQUAL_LENGTHS, SHARED_GCD, COPRIME, NOT_POWER_OF_TWO):
        K, n, rank, inv, bt, bo = host_tables(model)
        idx = mixed_block(model, 2 * TILE + 5)
        assert idx.size == (2 * TILE + 5) * n and idx.max() < K
        flags = rank[np.asarray([int("".join(map(str, c)), K) for c in idx.reshape(-1, n)[:500]])] != NONE
        assert 100 < flags.sum() < 400, "both flags, mixed"
    # one bit a chunk: the chunk counts of the block-edge test ARE its stream lengths
    for model, bit in ((ONE_BIT, 0), (ALL_ATYPICAL, 1)):
        K, n, rank, inv, bt, bo = host_tables(model)
        for chunks in (1, SUB + 1, GROUP - 1, 2 * GROUP + 1):
            bits, ends = encode_bits(np.zeros(chunks, np.int64), K, n, rank, bt, bo)
            assert bits.size == chunks and (bits == bit).all() and int(ends[-1]) == chunks
