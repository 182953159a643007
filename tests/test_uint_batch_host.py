"""The batched integer coders (csrc/scl_uint.hip) without a device: the rule without the 32-bit limit
(``scl_uint_fields_host`` / ``scl_uint_decode_wide_one_host``) against the plain-Python restatement, the restatement against
the reference's goldens, the host's length formula, the argument checks of the batch entry points, and the classes' refusal
to code a batch without a device."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_ids
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import UintCode
from stanford_compression_library_amd.compressors import _uint_block
from stanford_compression_library_amd.compressors import GolombUintEncoder, UniversalUintEncoder
from stanford_compression_library_amd.compressors.elias_delta_uint_coder import EliasDeltaUintEncoder
from stanford_compression_library_amd.core.data_block import DataBlock
from uint_batch_helpers import (BATCH_GOLDENS, CODES, EDGE_MS, ST_SIZE, ST_TRUNCATED, TOP, WIDE_GOLDENS, as_text, codeword,
                                codeword_length, decode_one_wide, decode_stream_wide, golden_bits, golden_code, stream_bits)
from uint_code_helpers import length_boundaries, pack

RULE_CODES = sorted(set(CODES) | {("golomb", M) for M in EDGE_MS}, key=lambda c: (c[0], c[1] or 0))
RULE_IDS = [f"{k}{M or ''}" for k, M in RULE_CODES]


def rule_values(kind, M):
    wide = [int(v) for c in WIDE_GOLDENS if golden_code(c) == (kind, M) for v in c.arr("values")]
    return sorted(set(length_boundaries(kind, M)) | set(wide) | {TOP, TOP - 1, 1 << 31, 0, 1})


# ---- the codeword in pieces ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", RULE_CODES, ids=RULE_IDS)
def test_fields_concatenated_are_the_codeword(kind, M):
    code = UintCode(kind, M)
    met_wide = 0
    for x in rule_values(kind, M):
        run, ((f0, n0), (f1, n1)) = code.fields(x)
        assert n0 <= 32 and n1 <= 32 and f0 < (1 << n0) and f1 < (1 << n1), (x, run, f0, n0, f1, n1)
        assert run + n0 + n1 == codeword_length(kind, M, x), x
        tail = (f0 << n1) | f1
        if kind == "golomb":  # (x / M ones are compared as a count: no integer of 2^32 bits)
            assert (run, n1) == (x // M, 0) and (tail, n0) == codeword(kind, M, x % M), x
        else:
            assert run == 0 and (tail, n0 + n1) == codeword(kind, M, x), x
        if run + n0 + n1 <= 32:  # the block kernels' form of the same codeword
            assert code.codeword(x) == ((((1 << run) - 1) << (n0 + n1)) | tail, run + n0 + n1), x
        else:
            met_wide += 1
            assert code.codeword(x)[1] == 0, x
    assert met_wide  # the 32-bit limit was crossed


# ---- one codeword read sequentially ----------------------------------------------------------------------------------------
def check_reads(code, kind, M, bits, totals):
    """the host export against the restatement on the first ``total`` bits of the 0/1 array ``bits``, for every total given,
    read from bit 0 and from an odd bit position behind a few ones -> the verdicts"""
    text, at0, at13 = as_text(bits), pack(bits), pack(np.concatenate([np.ones(13, np.uint8), bits]))
    out = []
    for total in totals:
        want = decode_one_wide(kind, M, text, 0, total)
        assert code.decode_wide_one(at0, 0, total) == want, (kind, M, total, want)
        assert code.decode_wide_one(at13, 13, total) == want, (kind, M, total, want)
        out.append(want)
    return out


@pytest.mark.parametrize("kind,M", RULE_CODES, ids=RULE_IDS)
def test_decode_wide_one_equals_the_restatement_on_codewords_and_their_cuts(kind, M):
    code = UintCode(kind, M)
    values = [x for x in rule_values(kind, M) if codeword_length(kind, M, x) <= 4200]
    assert any(codeword_length(kind, M, x) > 32 for x in values)
    for x in values:
        bits = stream_bits(kind, M, [x])
        follow = np.concatenate([bits, np.array([1, 0, 1, 1, 0, 0, 1, 0] * 9, np.uint8)])  # what lies behind is not looked at
        cuts = range(1, bits.size) if bits.size <= 70 else sorted({*range(1, 34), *range(bits.size - 34, bits.size)})
        got = check_reads(code, kind, M, follow, [*cuts, bits.size])
        assert got[-1] == (0, bits.size, x), (x, got[-1])
        assert all(g[0] == ST_TRUNCATED for g in got[:-1]), x


def golomb_text(M, q, r):
    v, n = codeword("golomb", M, r)
    return "1" * q + format(v, f"0{n}b")


M3 = 3 << 18  # b = 19, cutoff = 2^18: 2^32 - 1 = 5461 * M3 + (cutoff - 1), the last short remainder
ANNOUNCING = [
    ("universal", None, "1" * 32 + "0" * 40, ST_SIZE),           # the 32nd one
    ("universal", None, "1" * 31 + "0" + "1" * 32, 0),            # L = 32 is the last that fits
    ("universal", None, "1" * 31, ST_TRUNCATED),
    ("elias_delta", None, "000000" + "1" * 60, ST_SIZE),          # the 6th zero
    ("elias_delta", None, "00000", ST_TRUNCATED),
    ("elias_delta", None, "00000" + "100010" + "0" * 40, ST_SIZE),          # n + 1 = 34: n = 33
    ("elias_delta", None, "00000" + "100001" + "0" * 31 + "1", ST_SIZE),    # n = 32 with a low field != 0: 2^32 and more
    ("elias_delta", None, "00000" + "100001" + "0" * 32, 0),                 # n = 32, low field 0: 2^32 - 1
    ("elias_delta", None, "00000" + "100001" + "0" * 31, ST_TRUNCATED),
    ("golomb", 1 << 30, "1111" + "0" * 31, ST_SIZE),              # M * q = 2^32 at the 4th one
    ("golomb", 1 << 30, "111", ST_TRUNCATED),
    ("golomb", (1 << 31) - 1, golomb_text((1 << 31) - 1, 2, (1 << 31) - 2), ST_SIZE),  # M * q + r = 2^32 + 2^31 - 4
    ("golomb", (1 << 31) - 1, golomb_text((1 << 31) - 1, 2, 1), 0),                    # 2^32 - 1
    ("golomb", (1 << 31) - 1, "111", ST_SIZE),
    ("golomb", M3, golomb_text(M3, 5461, (1 << 18) - 1), 0),      # 2^32 - 1 ...
    ("golomb", M3, golomb_text(M3, 5461, 1 << 18), ST_SIZE),      # ... and 2^32: the remainder carries it over
    ("golomb", M3, "1" * 5462, ST_SIZE),                          # the one that makes M * q >= 2^32
    ("golomb", M3, "1" * 5461, ST_TRUNCATED),
]


@pytest.mark.parametrize("kind,M,text,status", ANNOUNCING, ids=[f"{a[0]}{a[1] or ''}-{i}" for i, a in enumerate(ANNOUNCING)])
def test_decode_wide_one_on_announcing_prefixes(kind, M, text, status):
    bits = np.frombuffer(text.encode(), np.uint8) - ord("0")
    want, = check_reads(UintCode(kind, M), kind, M, bits, [bits.size])
    assert want[0] == status, want
    if status == 0:
        assert want[1] == bits.size


# ---- the restatement is the reference's code -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BATCH_GOLDENS, ids=golden_ids(BATCH_GOLDENS))
def test_restatement_reproduces_the_goldens(case):
    kind, M = golden_code(case)
    values = [int(v) for v in case.arr("values")]
    bits = stream_bits(kind, M, values)
    assert bits.size == case.nbits and np.array_equal(pack(bits), case.arr("out"))
    got, used, status = decode_stream_wide(kind, M, golden_bits(case))
    assert (got.tolist(), used, status) == (values, case.nbits, 0)


# ---- the host's length formula ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", RULE_CODES, ids=RULE_IDS)
def test_length_formula_equals_the_restatement(kind, M):
    values = rule_values(kind, M) + np.random.default_rng(3).integers(0, 1 << 32, 2000).tolist()
    got = _uint_block.code_lengths(UintCode(kind, M), np.array(values, np.int64))
    assert got.tolist() == [codeword_length(kind, M, x) for x in values]


def test_slot_bytes_is_the_longest_codeword_times_the_count():
    for kind, M in RULE_CODES:
        code = UintCode(kind, M)
        for n, top in ((0, 0), (1, 0), (1000, 255), (1024, TOP), (3, 1 << 20)):
            want = ((n * codeword_length(kind, M, top) + 7) // 8 + 4 + 127) // 128 * 128
            assert code.slot_bytes(n, top) == want, (kind, M, n, top)
    L = backend_lib.load()
    assert L.scl_uint_slot_bytes(None, 5, 5) == 0
    for bad in (backend_lib.UintCodeStruct(0, 0), backend_lib.UintCodeStruct(0, 1 << 31), backend_lib.UintCodeStruct(3, 1)):
        assert L.scl_uint_slot_bytes(C.byref(bad), 5, 5) == 0


# ---- the argument checks run before any device call ------------------------------------------------------------------------
P = 0x10000  # a pointer value that is never followed: every call below is refused, or has no chunk to code


def encode_args(code, out_stride=128, n_chunks=1, d_val=P, d_out=P):
    return [code, d_val, 4, None, 4, n_chunks, d_out, out_stride, P, P, P, None]


def decode_args(code, n_chunks=1, d_in=P, d_out=P):
    return [code, d_in, 128, P, P, n_chunks, d_out, 4, 4, P, P, P, None]


BAD_CODES = [("a null code", None), ("M = 0", (0, 0)), ("M = 2^31", (0, 1 << 31)), ("an unknown kind", (3, 1))]


@pytest.mark.parametrize("what,code", BAD_CODES, ids=[b[0] for b in BAD_CODES])
@pytest.mark.parametrize("name", ["scl_uint_encode_batch", "scl_uint_decode_batch", "scl_uint_kernel_names"])
def test_batch_entry_points_refuse_a_bad_code(name, what, code):
    L = backend_lib.load()
    ref = C.byref(backend_lib.UintCodeStruct(*code)) if code else None
    buf = C.create_string_buffer(160)
    args = {"scl_uint_encode_batch": encode_args(ref), "scl_uint_decode_batch": decode_args(ref),
            "scl_uint_kernel_names": [ref, 1, buf, buf, 160]}[name]
    assert getattr(L, name)(*args) == backend_lib.E_PARAM, what
    assert backend_lib.last_error().startswith(name[len("scl_"):] + ":"), backend_lib.last_error()


@pytest.mark.parametrize("out_stride", [0, 8, 120, 1 << 29, (1 << 29) + 16])
def test_encode_batch_refuses_a_bad_out_stride(out_stride):
    L = backend_lib.load()
    code = C.byref(backend_lib.UintCodeStruct(1, 1))
    assert L.scl_uint_encode_batch(*encode_args(code, out_stride=out_stride)) == backend_lib.E_PARAM
    assert backend_lib.last_error().startswith("uint_encode_batch: bad out_stride"), backend_lib.last_error()


def test_batch_entry_points_refuse_null_and_misaligned_pointers():
    L = backend_lib.load()
    code = C.byref(backend_lib.UintCodeStruct(2, 1))
    for args in (encode_args(code, d_val=None), encode_args(code, d_out=None), encode_args(code, d_out=P + 8),
                 encode_args(code, d_val=P + 2)):
        assert L.scl_uint_encode_batch(*args) == backend_lib.E_PARAM
        assert backend_lib.last_error().startswith("uint_encode_batch:"), backend_lib.last_error()
    for args in (decode_args(code, d_in=None), decode_args(code, d_out=None), decode_args(code, d_in=P + 2),
                 decode_args(code, d_out=P + 2)):
        assert L.scl_uint_decode_batch(*args) == backend_lib.E_PARAM
        assert backend_lib.last_error().startswith("uint_decode_batch:"), backend_lib.last_error()
    # what the checks let through, with no chunk to code: nothing is launched
    assert L.scl_uint_encode_batch(*encode_args(code, n_chunks=0, out_stride=(1 << 29) - 16)) == backend_lib.OK
    assert L.scl_uint_decode_batch(*decode_args(code, n_chunks=0)) == backend_lib.OK


def test_kernel_names_follow_the_threads_switch():
    code = UintCode("golomb", 6)
    assert code.kernel_names(1) == ("uint_encode_fast_kernel", "uint_decode_fast_kernel")
    assert code.kernel_names(1, any_parameter_kernels=True) == ("uint_encode_kernel", "uint_decode_kernel")


# ---- the classes ------------------------------------------------------------------------------------------------------------
ENCODERS = [lambda: GolombUintEncoder(6), UniversalUintEncoder, EliasDeltaUintEncoder]


@pytest.mark.parametrize("make", ENCODERS, ids=["golomb", "universal", "elias_delta"])
def test_blocks_that_need_no_launch_need_no_device(make, monkeypatch):
    """empty blocks, values of 2^32 and more and an empty list take ``encode_block``: no batch call is made"""
    def refuse(*a, **k):
        raise AssertionError("a batched launch was made")

    monkeypatch.setattr(UintCode, "encode_batch", refuse)
    monkeypatch.setattr(UintCode, "decode_batch", refuse)
    enc = make()
    blocks = [DataBlock([]), DataBlock([1, (1 << 32) + 5, 2]), DataBlock([])]
    assert enc.encode_blocks([]) == []
    assert enc.encode_blocks(blocks) == [enc.encode_block(b) for b in blocks]


def test_golomb_m_of_2_31_takes_the_host_route(monkeypatch):
    monkeypatch.setattr(UintCode, "encode_batch", None)
    enc = GolombUintEncoder(1 << 31)
    blocks = [DataBlock([5, 1 << 31, (1 << 32) - 1])]
    assert enc.encode_blocks(blocks) == [enc.encode_block(b) for b in blocks]


@pytest.mark.parametrize("make", ENCODERS, ids=["golomb", "universal", "elias_delta"])
def test_a_batch_fails_loudly_without_gpu(make):
    """no quiet host route: a qualifying batch needs the device"""
    if backend_lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(backend_lib.SclHipError):
        make().encode_blocks([DataBlock([1, 2, 3]), DataBlock([4])])
