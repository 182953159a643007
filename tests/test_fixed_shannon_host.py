"""Fixed-width coder and Shannon / Fano / Shannon-Fano-Elias codes without a GPU: the three code constructions against the
reference's tables, the host helpers they stand on, the numpy restatement of the fixed-width pack against the reference's
data sections, the parameter refusals of the new entry points, and the classes' host path (blocks below
``FIXED_BLOCK_MIN``) against the reference's bits.  Goldens: tools/gen_fixed_shannon_goldens.py."""
import ctypes as C
import pickle

import numpy as np
import pytest

from conftest import golden_ids, load_golden
from fixed_width_helpers import golden_symbols, pack, pack_bits, unpack
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.compressors import fixed_bitwidth_compressor as fbc
from stanford_compression_library_amd.compressors.fano_coder import FanoDecoder, FanoEncoder, FanoTree
from stanford_compression_library_amd.compressors.shannon_coder import ShannonDecoder, ShannonEncoder
from stanford_compression_library_amd.compressors.shannon_fano_elias_coder import (ShannonFanoEliasDecoder,
                                                                                   ShannonFanoEliasEncoder)
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.core.prob_dist import ProbabilityDist
from stanford_compression_library_amd.external_compressors.pickle_external import PickleDecoder, PickleEncoder
from stanford_compression_library_amd.utils.bitarray_utils import (BitArray, bitarrays_to_float, float_to_bitarrays,
                                                                   uint_to_bitarray)

FIXED = load_golden("fixed_bitwidth")
FAMILY = load_golden("shannon_family")
BLOCKS = [c for c in FIXED if c.kind == "block" and "raises" not in c.meta]
REFUSED = [c for c in FIXED if c.kind == "block" and "raises" in c.meta]
TABLES = [c for c in FAMILY if c.kind == "table"]
CODERS = {"shannon": (ShannonEncoder, ShannonDecoder), "fano": (FanoEncoder, FanoDecoder),
          "sfe": (ShannonFanoEliasEncoder, ShannonFanoEliasDecoder)}


def fixed_coders(case):
    if case.coder == "pickle":
        return fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    return fbc.TextFixedBitwidthEncoder(), fbc.TextFixedBitwidthDecoder()


def family_dist(case):
    """(ProbabilityDist, symbols) of a golden table, the probabilities bit for bit"""
    values = case.arr("symbols").tolist()
    symbols = [chr(v) for v in values] if case.symbols == "str" else values
    return ProbabilityDist(dict(zip(symbols, case.arr("probs").tolist()))), symbols


def golden_bits(case):
    return BitArray.from_packed(case.arr("out"), case.nbits)


# ---- the goldens hold what the issue asks for --------------------------------------------------------------------------------
def test_golden_coverage():
    sizes = {len(set(c.arr("data").tolist())) for c in BLOCKS if c.symbols == "int"}
    assert {1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 65536} <= sizes
    assert {c.n for c in FIXED if c.kind == "block"} >= {0, 1, 7, 100}
    assert any(c.kind == "file" for c in FIXED) and REFUSED
    assert max(int(c.arr("len").max()) for c in TABLES if "raises" not in c.meta and c.coder == "shannon") == 20
    assert {c.coder for c in TABLES} == set(CODERS)


# ---- the three constructions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLES, ids=golden_ids(TABLES))
def test_code_tables_equal_the_reference(case):
    dist, symbols = family_dist(case)
    Enc, Dec = CODERS[case.coder]
    if "raises" in case.meta:
        with pytest.raises(Exception) as e:
            Enc(dist)
        assert type(e.value).__name__ == case.raises
        return
    enc = Enc(dist)
    table = enc._code_table()
    want = [symbols[i] for i in case.arr("order").tolist()]
    if case.coder != "fano":  # (a Fano table comes off the tree, the others are dicts in the reference's key order)
        assert list(table) == want
    assert set(table) == set(want)
    for s, code, length in zip(want, case.arr("code").tolist(), case.arr("len").tolist()):
        assert enc.encode_symbol(s) == uint_to_bitarray(int(code), bit_width=int(length)), s
        assert table[s] == enc.encode_symbol(s)
    dec = Dec(dist)
    for s in want:  # single symbols, trailing bits behind them
        word = enc.encode_symbol(s)
        assert dec.decode_symbol(word + BitArray("0110100111")) == (s, len(word))


def test_the_reference_expected_codewords():
    """test_shannon_coding / test_fano_coding of the reference, the codeword half (the round trips need the device)"""
    dists = [{"A": 0.5, "B": 0.5}, {"A": 0.3, "B": 0.3, "C": 0.4}, {"A": 0.5, "B": 0.25, "C": 0.12, "D": 0.13},
             {"A": 0.9, "B": 0.1}]
    shannon = [{"A": "0", "B": "1"}, {"A": "01", "B": "10", "C": "00"}, {"A": "0", "B": "10", "C": "1110", "D": "110"},
               {"A": "0", "B": "1110"}]
    fano = [{"A": "0", "B": "1"}, {"A": "10", "B": "11", "C": "0"}, {"A": "0", "B": "10", "C": "111", "D": "110"},
            {"A": "0", "B": "1"}]
    for d, s, f in zip(dists, shannon, fano):
        dist = ProbabilityDist(d)
        assert {k: ShannonEncoder(dist).encode_symbol(k).to01() for k in d} == s
        assert {k: FanoEncoder(dist).encode_symbol(k).to01() for k in d} == f


def test_fano_split_takes_the_first_minimum():
    # cumulative probabilities 0, 0.25, 0.5, 0.75: 0.5 is nearest, the cut is in front of the third symbol
    dist = ProbabilityDist({"a": 0.25, "b": 0.25, "c": 0.25, "d": 0.25})
    left, right = FanoTree._split_prob_dist_into_two(dist)
    assert (list(left), list(right)) == (["a", "b"], ["c", "d"])
    # 0, 0.4, 0.6: 0.4 and 0.6 are equally near in exact arithmetic, not in double: |0.4 - 0.5| = 0.09999999999999998 wins
    dist = ProbabilityDist({"a": 0.4, "b": 0.2, "c": 0.4})
    left, right = FanoTree._split_prob_dist_into_two(ProbabilityDist.get_sorted_prob_dist(dist.prob_dict, descending=True))
    assert (list(left), list(right)) == (["a"], ["c", "b"])


def test_codewords_the_kernels_cannot_carry_name_the_symbol():
    with pytest.raises(ValueError, match="'only'"):
        ShannonEncoder(ProbabilityDist({"only": 1.0}))
    # 33 bits and more: ProbabilityDist refuses p < 1e-6, so such a table can only be handed over
    from stanford_compression_library_amd.compressors.prefix_free_compressors import code_table_arrays

    with pytest.raises(NotImplementedError, match="'x'"):
        code_table_arrays({"x": BitArray("0" * 33), "y": BitArray("1")})


# ---- host helpers --------------------------------------------------------------------------------------------------------------
def test_float_to_bitarrays():
    assert float_to_bitarrays(0.5, 1) == (BitArray("0"), BitArray("1"))
    assert float_to_bitarrays(0.3, 8)[1] == BitArray("01001100")
    assert float_to_bitarrays(5.625, 4) == (BitArray("101"), BitArray("1010"))
    # the product is taken in double and truncated: 0.7 * 2^20 = 734003.2 -> 734003
    assert float_to_bitarrays(0.7, 20)[1] == uint_to_bitarray(734003, 20)
    for x, p in ((0.0, 3), (0.999, 10), (3.125, 5), (0.1 + 0.2, 30)):
        whole, frac = float_to_bitarrays(x, p)
        assert len(frac) == p
        back = bitarrays_to_float(whole, frac)
        assert 0 <= x - back < 2.0 ** -p


def test_pickle_coder():
    enc, dec = PickleEncoder(), PickleDecoder()
    for data in ([3, "alpha", "33.2313241234"], {"A": 1.111, "B": 0.3412452}, list(range(300))):
        bits = enc.encode_block(data)
        raw = pickle.dumps(data)
        assert bits == uint_to_bitarray(8 * len(raw), 32) + BitArray.from_packed(np.frombuffer(raw, np.uint8), 8 * len(raw))
        assert dec.decode_block(bits + BitArray("101111")) == (data, len(bits))
    assert len(PickleEncoder(length_bitwidth=16).encode_block([1])) == 16 + 8 * len(pickle.dumps([1]))


def test_text_alphabet_coder():
    """test_alphabet_encode_decode of the reference"""
    enc, dec = fbc.TextAlphabetEncoder(), fbc.TextAlphabetDecoder()
    bits = enc.encode_block(["A", "B", "C"])
    assert bits.tobytes() == b"\x03ABC"
    assert dec.decode_block(bits) == (["A", "B", "C"], 32)
    assert dec.decode_block(bits + BitArray("1")) == (["A", "B", "C"], 32)


def test_bit_width():
    widths = {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 16: 4, 17: 5, 255: 8, 256: 8, 257: 9, 1000: 10, 65536: 16}
    for size, w in widths.items():
        assert fbc.get_alphabet_fixed_bitwidth(size) == w
    with pytest.raises(OverflowError):
        fbc.get_alphabet_fixed_bitwidth(0)


# ---- the restatement against the reference's data sections ---------------------------------------------------------------------
@pytest.mark.parametrize("case", BLOCKS, ids=golden_ids(BLOCKS))
def test_restatement_equals_the_reference_data_section(case):
    order = case.arr("order").tolist()
    width = fbc.get_alphabet_fixed_bitwidth(len(order))
    index_of = {s: i for i, s in enumerate(order)}
    idx = np.array([index_of[s] for s in case.arr("data").tolist()], np.uint64)
    all_bits = np.unpackbits(case.arr("out"))[: case.nbits]
    start = case.head_bits + 32
    assert int.from_bytes(np.packbits(all_bits[case.head_bits: start]).tobytes(), "big") == case.n
    assert case.nbits == start + case.n * width
    assert np.array_equal(pack_bits(idx, width), all_bits[start:])
    packed, nbits = pack(idx, width)
    assert nbits == case.n * width and np.array_equal(unpack(packed, 0, case.n, width), idx)
    assert np.array_equal(unpack(case.arr("out"), start, case.n, width), idx)


# ---- the classes below the device threshold --------------------------------------------------------------------------------------
SMALL = [c for c in BLOCKS if c.n < fbc.FIXED_BLOCK_MIN]


def our_sections(case, bits):
    """(alphabet in OUR header order, bits in front of the data section) parsed from our own block"""
    _, dec = fixed_coders(case)
    alphabet, used = dec.alphabet_decoder.decode_block(bits)
    return alphabet, used + 32


@pytest.mark.parametrize("case", SMALL, ids=golden_ids(SMALL))
def test_host_path_encodes_the_reference_bits(case):
    enc, dec = fixed_coders(case)
    data = golden_symbols(case)
    bits = enc.encode_block(DataBlock(data))
    alphabet, start = our_sections(case, bits)
    # the header: the alphabet coder's own bits for the order this interpreter's set gave
    assert bits[: start - 32] == enc.alphabet_encoder.encode_block(alphabet)
    assert sorted(alphabet) == sorted(golden_symbols(case, "order"))
    # the data section: the restatement with that order
    index_of = {s: i for i, s in enumerate(alphabet)}
    width = fbc.get_alphabet_fixed_bitwidth(len(alphabet))
    want = pack_bits([index_of[s] for s in data], width)
    assert np.array_equal(np.asarray(bits.tolist()[start:], np.uint8), want)
    if case.symbols == "int":  # set order of small ints is fixed: the reference's data section bit for bit
        assert alphabet == golden_symbols(case, "order")
        assert bits[start:] == golden_bits(case)[case.head_bits + 32:]
        if case.coder == "text" or pickle.dumps(alphabet) == golden_bits(case)[32: case.head_bits].tobytes():
            assert bits == golden_bits(case)
    assert dec.decode_block(bits)[0].data_list == data


@pytest.mark.parametrize("case", SMALL, ids=golden_ids(SMALL))
def test_host_path_decodes_the_reference_bits(case):
    _, dec = fixed_coders(case)
    for packed, total, used in case.bits_with_garbage:  # trailing garbage behind the block
        block, consumed = dec.decode_block(BitArray.from_packed(packed, total))
        assert consumed == used
        assert block.data_list == golden_symbols(case)


@pytest.mark.parametrize("case", REFUSED, ids=golden_ids(REFUSED))
def test_what_the_reference_refuses_is_refused(case):
    enc, _ = fixed_coders(case)
    with pytest.raises(Exception) as e:
        enc.encode_block(DataBlock(golden_symbols(case)))
    assert type(e.value).__name__ == case.raises


def test_host_path_faults():
    enc, dec = fbc.FixedBitwidthEncoder(), fbc.FixedBitwidthDecoder()
    bits = enc.encode_block(DataBlock([0, 1, 2, 2, 1]))  # 3 symbols in 2 bits: index 3 has no symbol
    with pytest.raises(backend_lib.SclHipError, match="TRUNCATED"):
        dec.decode_block(bits[: len(bits) - 1])
    bad = bits.copy()
    bad[len(bits) - 2:] = BitArray("11")
    with pytest.raises(IndexError):
        dec.decode_block(bad)
    with pytest.raises(NotImplementedError):
        enc.encode_block(DataBlock(list(range(65537))))


def test_golden_file_decodes(tmp_path):
    case = next(c for c in FIXED if c.kind == "file")
    coded, back = tmp_path / "coded.bin", tmp_path / "back.txt"
    coded.write_bytes(case.arr("file").tobytes())
    fbc.TextFixedBitwidthDecoder().decode_file(str(coded), str(back))
    assert back.read_bytes() == case.arr("text").tobytes()
    # and our own file, block loop and framing included (test_text_fixed_bitwidth_file_encode_decode of the reference)
    from stanford_compression_library_amd.utils.test_utils import try_file_lossless_compression

    src = tmp_path / "in.txt"
    src.write_bytes(case.arr("text").tobytes())
    assert try_file_lossless_compression(str(src), fbc.TextFixedBitwidthEncoder(), fbc.TextFixedBitwidthDecoder(),
                                         encode_block_size=case.block_size)


# ---- every SCL_E_PARAM refusal, no device ------------------------------------------------------------------------------------------
A16 = 0x1000  # an aligned address nothing dereferences: the checks come first


def _arr(values, ctype):
    return (ctype * len(values))(*values)


def enc_args(**over):
    a = dict(d_sym=A16, sym_stride=64, d_lens=None, chunk_len=64, widths=[3], K=[5], n_chunks=1, d_out=A16, out_stride=64,
             d_bit_off=A16, d_nbits=A16, d_status=A16)
    a.update(over)
    w = _arr(a["widths"], C.c_uint32) if a["widths"] is not None else None
    k = _arr(a["K"], C.c_uint64) if a["K"] is not None else None
    return [a["d_sym"], a["sym_stride"], a["d_lens"], a["chunk_len"], w, k, a["n_chunks"], a["d_out"], a["out_stride"],
            a["d_bit_off"], a["d_nbits"], a["d_status"], None]


def dec_args(**over):
    a = dict(d_in=A16, in_size=64, d_bit_off=A16, d_in_nbits=A16, d_lens=None, widths=[3], K=[5], n_chunks=1, d_out=A16,
             out_stride=64, out_cap=64, d_out_lens=A16, d_consumed=A16, d_status=A16)
    a.update(over)
    w = _arr(a["widths"], C.c_uint32) if a["widths"] is not None else None
    k = _arr(a["K"], C.c_uint64) if a["K"] is not None else None
    return [a["d_in"], a["in_size"], a["d_bit_off"], a["d_in_nbits"], a["d_lens"], w, k, a["n_chunks"], a["d_out"],
            a["out_stride"], a["out_cap"], a["d_out_lens"], a["d_consumed"], a["d_status"], None]


ENC_REFUSALS = [dict(d_sym=None), dict(d_out=None), dict(d_bit_off=None), dict(d_nbits=None), dict(d_status=None),
                dict(widths=None), dict(K=None), dict(widths=[0]), dict(widths=[33]), dict(K=[0]), dict(K=[9]),
                dict(out_stride=24), dict(out_stride=0), dict(sym_stride=7), dict(d_sym=A16 + 4), dict(d_out=A16 + 8)]
DEC_REFUSALS = [dict(d_in=None), dict(d_bit_off=None), dict(d_in_nbits=None), dict(d_out=None), dict(d_out_lens=None),
                dict(d_consumed=None), dict(d_status=None), dict(widths=None), dict(K=None), dict(widths=[0]),
                dict(widths=[33]), dict(K=[0]), dict(K=[9]), dict(out_stride=7), dict(d_in=A16 + 4), dict(d_out=A16 + 8)]


@pytest.mark.parametrize("suffix", ["", "_u16", "_u32"])
def test_batch_entry_points_refuse_bad_arguments(suffix):
    L = backend_lib.load()
    for op, make, cases in (("encode", enc_args, ENC_REFUSALS), ("decode", dec_args, DEC_REFUSALS)):
        name = f"scl_fixed_{op}_batch{suffix}"
        for over in cases:
            assert getattr(L, name)(*make(**over)) == backend_lib.E_PARAM, (name, over)
            assert backend_lib.last_error().startswith(name[len("scl_"):] + ":"), (over, backend_lib.last_error())
        # a width the rows cannot hold: 9 through uint8, 17 through uint16; uint32 rows hold all
        for w, refused in ((9, suffix == ""), (17, suffix in ("", "_u16")), (32, suffix != "_u32")):
            rc = getattr(L, name)(*make(widths=[w], K=[2], n_chunks=0 if not refused else 1))
            assert (rc == backend_lib.E_PARAM) == refused, (name, w)
        # K = 2^w is the largest, at w = 32 too


def test_largest_alphabet_is_accepted_and_one_more_refused():
    L = backend_lib.load()
    w, k = _arr([32], C.c_uint32), _arr([(1 << 32) + 1], C.c_uint64)
    assert L.scl_fixed_encode_batch_u32(A16, 64, None, 64, w, k, 1, A16, 64, A16, A16, A16, None) == backend_lib.E_PARAM
    assert "alphabet size" in backend_lib.last_error()


def test_too_many_workgroups_are_refused():
    L = backend_lib.load()
    n = 1 << 12
    w, k = _arr([1] * n, C.c_uint32), _arr([2] * n, C.c_uint64)
    # 2^12 streams of 2^32 - 1 symbols, 2^19 tiles each: 2^31 workgroups, one too many
    assert L.scl_fixed_encode_batch(A16, 1 << 32, None, 0xFFFFFFFF, w, k, n, A16, 64, A16, A16, A16, None) == backend_lib.E_PARAM
    assert "workgroups" in backend_lib.last_error()


def test_other_entry_points_refuse_bad_arguments():
    L = backend_lib.load()
    assert L.scl_fixed_slot_bytes(100, 0) == 0 and L.scl_fixed_slot_bytes(100, 33) == 0
    assert L.scl_fixed_slot_bytes(1 << 32, 1) == 0 and L.scl_fixed_slot_bytes(1 << 27, 32) == 0
    assert L.scl_fixed_slot_bytes(0, 5) == 16 and L.scl_fixed_slot_bytes(32, 3) == 16 and L.scl_fixed_slot_bytes(43, 3) == 32
    buf = C.create_string_buffer(160)
    assert L.scl_fixed_kernel_names(3, 1, buf, buf, 160) == backend_lib.E_PARAM
    assert L.scl_fixed_kernel_names(1, 1, None, None, 160) == backend_lib.E_PARAM
    assert L.scl_fixed_kernel_names(1, 1, buf, None, 8) == backend_lib.E_PARAM
    assert L.scl_fixed_kernel_names(2, 1, buf, None, 160) == 0 and buf.value == b"fixed_encode_kernel<unsigned short>"
    idx, out = np.zeros(4, np.uint32), np.zeros(32, np.uint8)
    nb, st, n_out = C.c_uint64(), C.c_uint32(), C.c_uint64()
    for w, K in ((0, 1), (33, 1), (3, 0), (3, 9)):
        assert L.scl_fixed_encode_host(backend_lib.u32_ptr(idx), 4, w, K, backend_lib.u8_ptr(out), 32, C.byref(nb),
                                       C.byref(st)) == backend_lib.E_PARAM
        assert backend_lib.last_error().startswith("fixed_encode_host:")
        assert L.scl_fixed_decode_host(backend_lib.u8_ptr(out), 0, 12, 4, w, K, backend_lib.u32_ptr(idx), 4, C.byref(n_out),
                                       C.byref(nb), C.byref(st)) == backend_lib.E_PARAM
        assert backend_lib.last_error().startswith("fixed_decode_host:")
    assert L.scl_fixed_encode_host(None, 4, 3, 5, backend_lib.u8_ptr(out), 32, C.byref(nb), C.byref(st)) == backend_lib.E_PARAM


def test_a_block_from_the_threshold_on_needs_the_device():
    data = DataBlock([i % 3 for i in range(fbc.FIXED_BLOCK_MIN)])
    below = fbc.FixedBitwidthEncoder().encode_block(DataBlock(data.data_list[:-1]))  # the host's, with or without a device
    if backend_lib.device_count() > 0:  # both paths write the same bits: the longer block starts with the shorter one's
        at = fbc.FixedBitwidthEncoder().encode_block(data)
        head = len(below) - 2 * (data.size - 1)
        assert len(at) == len(below) + 2 and at[head:len(below)] == below[head:]
        return
    with pytest.raises(backend_lib.SclHipError):
        fbc.FixedBitwidthEncoder().encode_block(data)
