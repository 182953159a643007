"""The integer codes (Golomb, universal, Elias-delta) without a device: the restatement against the reference's goldens, the
rule the kernels compile (``scl_uint_codeword_host`` / ``scl_uint_decode_one_host``) against the restatement, the refused
parameters, and the classes' host path bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_ids
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend.models import UintCode
from stanford_compression_library_amd.compressors import _uint_block
from stanford_compression_library_amd.compressors import (GolombUintDecoder, GolombUintEncoder, UniversalUintDecoder,
                                                          UniversalUintEncoder)
from stanford_compression_library_amd.compressors.elias_delta_uint_coder import EliasDeltaUintDecoder, EliasDeltaUintEncoder
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.utils.bitarray_utils import BitArray
from uint_code_helpers import (CODE_IDS, CODES, GOLDENS, KIND_ID, ST_SIZE, ST_TRUNCATED, codeword, codeword_length, decode_one,
                               decode_stream, encode_bits, golden_code, length_boundaries, pack)

RULE_CODES = CODES + [("golomb", (1 << 31) - 1)]
RULE_IDS = CODE_IDS + ["golomb2^31-1"]


def coders(kind, M):
    if kind == "golomb":
        return GolombUintEncoder(M), GolombUintDecoder(M)
    if kind == "universal":
        return UniversalUintEncoder(), UniversalUintDecoder()
    return EliasDeltaUintEncoder(), EliasDeltaUintDecoder()


@pytest.fixture
def host_only(monkeypatch):
    """any call into the device route fails the test"""
    def refuse(*a, **k):
        raise AssertionError("the device route was taken")

    monkeypatch.setattr(_uint_block, "UINT_BLOCK_MIN", 1 << 62)
    monkeypatch.setattr(UintCode, "encode_host", refuse)
    monkeypatch.setattr(UintCode, "decode_host", refuse)


# ---- the restatement is the reference's code -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_restatement_reproduces_the_golden(case):
    kind, M = golden_code(case)
    values = [int(v) for v in case.arr("values")]
    bits, ends = encode_bits(kind, M, values)
    assert bits.size == case.nbits and np.array_equal(pack(bits), case.arr("out"))
    assert np.array_equal(np.diff(ends, prepend=0), case.arr("lens"))
    if case.device:
        got, used, status = decode_stream(kind, M, bits)
        assert (got.tolist(), used, status) == (values, case.nbits, 0)
    else:  # the first codeword above 32 bits stops the device's decoder, with what came before delivered
        first = int(np.flatnonzero(case.arr("lens") > 32)[0])
        got, used, status = decode_stream(kind, M, bits)
        assert (got.tolist(), used, status) == (values[:first], int(ends[first - 1]) if first else 0, ST_SIZE)


# ---- the rule the kernels compile ----------------------------------------------------------------------------------------
def rule_values(kind, M):
    return sorted(set(range(4096)) | set(length_boundaries(kind, M)) | {(1 << 32) - 1, 1 << 31})


@pytest.mark.parametrize("kind,M", RULE_CODES, ids=RULE_IDS)
def test_codeword_rule_equals_the_restatement(kind, M):
    code = UintCode(kind, M)
    met_long = 0
    for x in rule_values(kind, M):
        got = code.codeword(x)
        if codeword_length(kind, M, x) > 32:
            met_long += 1
            assert got[1] == 0, (x, got)
        else:
            assert got == codeword(kind, M, x), (x, got)
    assert met_long  # the limit itself was crossed


@pytest.mark.parametrize("kind,M", RULE_CODES, ids=RULE_IDS)
def test_decode_rule_equals_the_restatement(kind, M):
    """the codeword of every x < 4096 and of every length boundary +- 1, in front of ones and in front of zeros: whole
    (rem = its length, 32 and more) and cut; for x < 300 and the boundaries cut at every length, for the rest cut once, one
    bit short.  Codewords above 32 bits are the prefixes that announce too much"""
    code = UintCode(kind, M)
    statuses = set()
    edges = set(length_boundaries(kind, M))
    for x in rule_values(kind, M):
        if x >= 1 << 31 and kind == "golomb" and M < 1 << 16:
            continue  # (2^15 ones and more: nothing the 64 bits below do not show for x < 4096 already)
        v, n = codeword(kind, M, x)
        every_cut = set(range(1, min(n, 32) + 1)) | {2, 33, 40} if x < 300 or x in edges else set()
        head = format(v >> max(n - 64, 0), f"0{min(n, 64)}b")  # the first 64 bits of the codeword
        for fill in ("0", "1"):
            text = (head + fill * 64)[:64]
            for rem in sorted({1, n - 1, n, n + 1, 32} | every_cut):
                if not 1 <= rem <= 64:
                    continue
                want = decode_one(kind, M, text, 0, rem)
                got = code.decode_one(int(text[:32], 2), rem)
                assert got == want, (x, fill, rem, got, want)
                statuses.add(want[0])
                if n <= 32 and rem >= n:
                    assert want == (0, n, x)
    assert statuses == {0, ST_TRUNCATED, ST_SIZE}


def test_reciprocal_division_equals_floor_division():
    """Golomb's x / M by the host-computed reciprocal, through the codeword (q ones in front): at and around every multiple
    of M that a 32-bit codeword reaches, for M around powers of two, small, prime and the largest"""
    Ms = [3, 5, 6, 7, 9, 10, 11, 641, 1000, 65535, 65537, (1 << 20) + 7, (1 << 30) - 1, (1 << 30) + 1, (1 << 31) - 1]
    for M in Ms:
        code = UintCode("golomb", M)
        b = M.bit_length() - 1
        for q in range(0, 34 - b):
            for x in (q * M - 1, q * M, q * M + 1, q * M + M // 2, q * M + M - 1):
                if not 0 <= x < (1 << 32):
                    continue
                got_bits, got_len = code.codeword(x)
                if codeword_length("golomb", M, x) > 32:
                    assert got_len == 0, (M, x)
                else:
                    assert (got_bits, got_len) == codeword("golomb", M, x), (M, x)
                    ones = got_len - len(format(got_bits, f"0{got_len}b").lstrip("1"))
                    assert ones == x // M, (M, x)
        for x in ((1 << 32) - 1, (1 << 32) - M, M * ((1 << 32) // M) - 1):  # the largest quotients: refused, not wrapped
            want_len = codeword_length("golomb", M, x)
            assert code.codeword(x)[1] == (want_len if want_len <= 32 else 0), (M, x)


# ---- refused parameters: SCL_E_PARAM, the entry point named, no device --------------------------------------------------
def test_refused_parameters():
    L = backend_lib.load()
    good = backend_lib.UintCodeStruct(0, 10)
    room = (C.c_uint8 * 192)()
    buf = (C.c_uint8 * 64).from_address((C.addressof(room) + 63) & ~63)  # 64-byte aligned, so p + 1 .. p + 4 are not
    val = (C.c_uint32 * 16)()
    n64, st32, a32 = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    p = C.addressof(buf)  # a host address stands in for the device pointers: every check comes before the first device call
    bad_codes = [backend_lib.UintCodeStruct(0, 0), backend_lib.UintCodeStruct(0, 1 << 31),
                 backend_lib.UintCodeStruct(0, (1 << 32) - 1), backend_lib.UintCodeStruct(3, 10), None]

    def calls(code):
        c = C.byref(code) if code is not None else None
        return {
            "uint_encode_block": lambda: L.scl_uint_encode_block(c, p, 16, p, 64, p, p, p, 4096, None),
            "uint_decode_block": lambda: L.scl_uint_decode_block(c, p, 64, 0, 100, p, 16, p, p, 4096, None),
            "uint_encode_block_host": lambda: L.scl_uint_encode_block_host(c, val, 16, buf, 64, C.byref(n64), C.byref(st32)),
            "uint_decode_block_host": lambda: L.scl_uint_decode_block_host(c, buf, 100, val, 16, C.byref(n64), C.byref(n64),
                                                                           C.byref(st32)),
            "uint_codeword_host": lambda: L.scl_uint_codeword_host(c, 5, C.byref(a32), C.byref(st32)),
            "uint_decode_one_host": lambda: L.scl_uint_decode_one_host(c, 5, 32, C.byref(a32), C.byref(st32)),
        }

    for code in bad_codes:
        for name, call in calls(code).items():
            assert call() == backend_lib.E_PARAM, (name, code and (code.kind, code.M))
            assert backend_lib.last_error().startswith(name + ":"), backend_lib.last_error()
    g = C.byref(good)
    refused = {
        "uint_encode_block": [
            lambda: L.scl_uint_encode_block(g, None, 16, p, 64, p, p, p, 4096, None),       # null values
            lambda: L.scl_uint_encode_block(g, p, 16, None, 64, p, p, p, 4096, None),       # null output
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, None, p, p, 4096, None),       # null nbits
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p, None, p, 4096, None),       # null status
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p, p, None, 4096, None),       # null scratch
            lambda: L.scl_uint_encode_block(g, p, 1 << 32, p, 64, p, p, p, 1 << 40, None),  # 2^32 values
            lambda: L.scl_uint_encode_block(g, p, 16, p + 2, 64, p, p, p, 4096, None),      # misaligned output
            lambda: L.scl_uint_encode_block(g, p + 2, 16, p, 64, p, p, p, 4096, None),      # misaligned values
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p + 4, p, p, 4096, None),      # misaligned nbits (8 bytes)
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p, p + 2, p, 4096, None),      # misaligned status
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p, p, p + 4, 4096, None),      # misaligned scratch (8 bytes)
            lambda: L.scl_uint_encode_block(g, p, 16, p, 64, p, p, p, 8, None),             # scratch too small
        ],
        "uint_decode_block": [
            lambda: L.scl_uint_decode_block(g, None, 64, 0, 100, p, 16, p, p, 4096, None),
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, None, 16, p, p, 4096, None),
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p, 16, None, p, 4096, None),
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p, 16, p, None, 4096, None),
            lambda: L.scl_uint_decode_block(g, p, 1 << 50, 0, 1 << 46, p, 16, p, p, 1 << 50, None),  # 2^46 bits
            lambda: L.scl_uint_decode_block(g, p + 1, 64, 0, 100, p, 16, p, p, 4096, None),          # misaligned input
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p + 2, 16, p, p, 4096, None),          # misaligned values
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p, 16, p + 4, p, 4096, None),          # misaligned result (8)
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p, 16, p, p + 4, 4096, None),          # misaligned scratch (8)
            lambda: L.scl_uint_decode_block(g, p, 64, 0, 100, p, 16, p, p, 8, None),                 # scratch too small
            lambda: L.scl_uint_decode_block(g, p, 12, 0, 100, p, 16, p, p, 4096, None),              # ends behind the input
        ],
        "uint_encode_block_host": [
            lambda: L.scl_uint_encode_block_host(g, None, 16, buf, 64, C.byref(n64), C.byref(st32)),
            lambda: L.scl_uint_encode_block_host(g, val, 16, None, 64, C.byref(n64), C.byref(st32)),
            lambda: L.scl_uint_encode_block_host(g, val, 16, buf, 64, None, C.byref(st32)),
            lambda: L.scl_uint_encode_block_host(g, val, 16, buf, 64, C.byref(n64), None),
            lambda: L.scl_uint_encode_block_host(g, val, 1 << 32, buf, 64, C.byref(n64), C.byref(st32)),
        ],
        "uint_decode_block_host": [
            lambda: L.scl_uint_decode_block_host(g, None, 100, val, 16, C.byref(n64), C.byref(n64), C.byref(st32)),
            lambda: L.scl_uint_decode_block_host(g, buf, 100, None, 16, C.byref(n64), C.byref(n64), C.byref(st32)),
            lambda: L.scl_uint_decode_block_host(g, buf, 100, val, 16, None, C.byref(n64), C.byref(st32)),
            lambda: L.scl_uint_decode_block_host(g, buf, 100, val, 16, C.byref(n64), C.byref(n64), None),
            lambda: L.scl_uint_decode_block_host(g, buf, 1 << 46, val, 16, C.byref(n64), C.byref(n64), C.byref(st32)),
        ],
        "uint_codeword_host": [lambda: L.scl_uint_codeword_host(g, 5, None, C.byref(st32))],
        "uint_decode_one_host": [lambda: L.scl_uint_decode_one_host(g, 5, 32, None, C.byref(st32)),
                                 lambda: L.scl_uint_decode_one_host(g, 5, 0, C.byref(a32), C.byref(st32))],
    }
    for name, tries in refused.items():
        for i, call in enumerate(tries):
            assert call() == backend_lib.E_PARAM, (name, i)
            assert backend_lib.last_error().startswith(name + ":"), backend_lib.last_error()
    assert L.scl_uint_block_scratch_bytes(0, 0) >= 64
    with pytest.raises(backend_lib.SclHipError):
        UintCode("golomb", 0)
    with pytest.raises(backend_lib.SclHipError):
        UintCode("golomb", 1 << 31)


# ---- the classes' host path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDENS, ids=golden_ids(GOLDENS))
def test_classes_host_path_reproduces_the_golden(case, host_only):
    kind, M = golden_code(case)
    enc, dec = coders(kind, M)
    values = [int(v) for v in case.arr("values")]
    bits = enc.encode_block(DataBlock(values))
    assert len(bits) == case.nbits and np.array_equal(bits.packed(), case.arr("out"))
    block, used = dec.decode_block(bits)
    assert block.data_list == values and used == case.nbits
    ends = np.cumsum(case.arr("lens"))
    for i in range(0, len(values), max(1, len(values) // 7)):  # single values: the symbol calls
        word = bits[int(ends[i - 1]) if i else 0: int(ends[i])]
        assert enc.encode_symbol(values[i]) == word
        assert dec.decode_symbol(word + BitArray("10")) == (values[i], len(word))


def test_host_path_codes_huge_integers_symbol_by_symbol(host_only):
    for kind, M in (("golomb", 1 << 70), ("golomb", 1000003), ("universal", None)):
        enc, dec = coders(kind, M)
        values = [3, (1 << 80) + 12345, 0, 1 << 63]
        if kind == "golomb" and M < (1 << 60):
            values = [3, 1 << 33, 0]
        bits = enc.encode_block(DataBlock(values))
        words = [codeword(kind, M, v) for v in values]
        assert bits.to01() == "".join(format(v, f"0{n}b") for v, n in words)
        block, used = dec.decode_block(bits)
        assert block.data_list == values and used == len(bits)


def test_decode_symbol_on_the_references_examples():
    uni = UniversalUintDecoder()
    for x, word in ((0, "00"), (1, "01"), (2, "1010"), (3, "1011"), (4, "110100"), (100, "11111101100100")):
        assert UniversalUintEncoder().encode_symbol(x) == BitArray(word)
        assert uni.decode_symbol(BitArray(word + "01")) == (x, len(word))
    for M, pairs in ((4, ((0, "000"), (1, "001"), (4, "1000"), (102, "1" * 25 + "0" + "10"))),
                     (10, ((2, "0010"), (7, "01101"), (26, "1101100"), (102, "11111111110010")))):
        for x, word in pairs:
            assert GolombUintEncoder(M).encode_symbol(x) == BitArray(word)
            assert GolombUintDecoder(M).decode_symbol(BitArray(word + "10")) == (x, len(word))
    with pytest.raises(AssertionError):
        GolombUintEncoder(0)
    with pytest.raises(AssertionError):
        UniversalUintEncoder().encode_symbol(-1)


@pytest.mark.parametrize("kind,M", [("golomb", 10), ("golomb", 4), ("universal", None)], ids=["golomb10", "golomb4", "universal"])
def test_host_path_names_a_truncated_stream(kind, M, host_only):
    """cut inside the unary part, the remainder and Golomb's extra bit: the error ``PrefixModel.decode_host`` raises"""
    enc, dec = coders(kind, M)
    values = [5, 0, 97, 8]
    bits, ends = encode_bits(kind, M, values)
    for cut in range(1, bits.size):
        want = decode_stream(kind, M, bits, nbits=cut)
        if want[2] == 0:
            assert dec.decode_block(BitArray._wrap(bits[:cut].copy()))[0].data_list == want[0].tolist()
        else:
            assert want[2] == ST_TRUNCATED
            with pytest.raises(backend_lib.SclHipError) as err:
                dec.decode_block(BitArray._wrap(bits[:cut].copy()))
            assert err.value.code == backend_lib.E_CHUNK and "TRUNCATED" in str(err.value)


def test_elias_delta_below_the_threshold_stays_on_the_host(monkeypatch):
    """LZ77's counts keep their path: below UINT_BLOCK_MIN the device route is never called"""
    def refuse(*a, **k):
        raise AssertionError("the device route was taken")

    monkeypatch.setattr(_uint_block, "device_encode", refuse)
    monkeypatch.setattr(_uint_block, "device_decode", refuse)
    n = _uint_block.UINT_BLOCK_MIN - 1
    values = (np.arange(n) % 3).tolist()  # 0 -> 1 bit: n values in fewer than 3 n bits
    bits = EliasDeltaUintEncoder().encode_block(DataBlock(values))
    want, _ = encode_bits("elias_delta", None, values)
    assert np.array_equal(bits._b, want)
    short = bits[: int(encode_bits("elias_delta", None, values[: n // 4])[0].size)]
    assert len(short) < _uint_block.UINT_BLOCK_MIN
    assert EliasDeltaUintDecoder().decode_block(short)[0].data_list == values[: n // 4]
    with pytest.raises(AssertionError, match="device route"):
        EliasDeltaUintEncoder().encode_block(DataBlock(values + [1]))
    assert KIND_ID["elias_delta"] == backend_lib.UINT_ELIAS_DELTA
