"""Prefix-free / Huffman coders, host side (no GPU): the trees and tables equal the reference's (goldens), the C ABI
validates a code table before it touches a device, and the new entry points check their arguments."""
import ctypes

import numpy as np
import pytest

from prefix_helpers import goldens, make_dist, table_case
from conftest import golden_ids
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.compressors import (HuffmanDecoder, HuffmanEncoder, HuffmanTree, PrefixFreeTree)
from stanford_compression_library_amd.compressors.prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder
from stanford_compression_library_amd.utils.bitarray_utils import BitArray

TABLES = goldens()["table"]


@pytest.mark.parametrize("case", TABLES, ids=golden_ids(TABLES))
def test_huffman_table_equals_the_reference(case):
    """every tie decided as the reference decides it: same codewords, same key order (DFS, left first)"""
    table = HuffmanTree(make_dist(case)).get_encoding_table()
    assert list(table) == case.arr("order").tolist()
    code, length = case.arr("code"), case.arr("len")
    for s, bits in table.items():
        assert len(bits) == length[s] and int(bits.to01(), 2) == code[s], s


def test_one_symbol_alphabet_is_the_code_0():
    tree = HuffmanTree(make_dist(table_case("one_symbol")))
    assert tree.get_encoding_table() == {0: BitArray("0")}
    assert tree.root_node.right_child is None and tree.root_node.left_child.is_leaf_node


@pytest.mark.parametrize("group", ["dyadic4", "ties16", "random17", "skewed28"])
def test_tree_from_code_round_trips(group):
    table = HuffmanTree(make_dist(table_case(group))).get_encoding_table()
    rebuilt = PrefixFreeTree.build_prefix_free_tree_from_code(table).get_encoding_table()
    assert rebuilt == table and list(rebuilt) == list(table)  # a DFS of the same tree: same key order
    with pytest.raises(AssertionError):
        PrefixFreeTree.build_prefix_free_tree_from_code({"A": "01"})


def test_decode_symbol_returns_symbol_and_length():
    dist = make_dist(table_case("random17"))
    enc, dec = HuffmanEncoder(dist), HuffmanDecoder(dist)
    assert isinstance(enc, PrefixFreeEncoder) and isinstance(dec, PrefixFreeDecoder)
    for s in dist.alphabet:
        code = enc.encode_symbol(s)
        assert code == enc.encoding_table[s]
        assert dec.decode_symbol(code + BitArray("0110")) == (s, len(code))
        assert dec.tree.decode_symbol(code) == (s, len(code))


def test_codes_longer_than_32_bits_are_refused_by_name():
    case = table_case("skewed40")
    assert case.max_len > 32
    dist = make_dist(case)
    from stanford_compression_library_amd.core.data_block import DataBlock

    with pytest.raises(NotImplementedError, match=f"{case.max_len} bits"):
        HuffmanEncoder(dist).encode_block(DataBlock([0, 1]))
    with pytest.raises(NotImplementedError, match=f"{case.max_len} bits"):
        HuffmanDecoder(dist).decode_block(BitArray("0"))


def _create(codes, lens, K=None):
    L = backend_lib.load()
    h = ctypes.c_void_p()
    c = (ctypes.c_uint32 * max(len(codes), 1))(*codes)
    n = (ctypes.c_uint8 * max(len(lens), 1))(*lens)
    rc = L.scl_prefix_model_create(c, n, len(codes) if K is None else K, ctypes.byref(h))
    return rc, backend_lib.last_error()


def test_model_create_validates_before_it_touches_a_device():
    E = backend_lib.E_PARAM
    rc, msg = _create([0b0, 0b01], [1, 2])  # "0" is a prefix of "01"
    assert rc == E and "prefix" in msg
    rc, msg = _create([0b01, 0b0], [2, 1])  # the same, the longer code first
    assert rc == E and "prefix" in msg
    rc, msg = _create([0b10, 0b10], [2, 2])  # equal codewords
    assert rc == E and "prefix" in msg
    rc, msg = _create([0, 1], [0, 1])  # a length of zero
    assert rc == E and "0 bits" in msg
    rc, msg = _create([0, 1], [33, 1])
    assert rc == E and "33 bits" in msg
    rc, msg = _create([], [], K=0)
    assert rc == E and "alphabet size 0" in msg
    rc, msg = _create([0, 1], [1, 1], K=65537)
    assert rc == E and "65537" in msg


PREFIX_BATCH_ENTRY_POINTS = [f"scl_prefix_{op}_batch{form}" for form in ("", "_u16") for op in ("encode", "decode")]


@pytest.mark.parametrize("name", PREFIX_BATCH_ENTRY_POINTS)
def test_prefix_batch_entry_points_refuse_a_null_model(name):
    L = backend_lib.load()
    fn = getattr(L, name)
    assert fn(*[None if t is ctypes.c_void_p else 0 for t in fn.argtypes]) == backend_lib.E_PARAM
    assert backend_lib.last_error().startswith(name[len("scl_"):] + ":"), backend_lib.last_error()


def test_prefix_calls_without_a_model():
    L = backend_lib.load()
    assert L.scl_prefix_slot_bytes(None, 100) == 0
    assert L.scl_prefix_model_info(None, None) == backend_lib.E_PARAM
    L.scl_prefix_model_destroy(None)
