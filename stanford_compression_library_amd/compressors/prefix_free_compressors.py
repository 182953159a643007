"""Prefix-free codes with the reference's class API, coded by the gfx950 kernels.

Drop-in for reference scl/compressors/prefix_free_compressors.py: ``PrefixFreeEncoder`` (:17-50),
``PrefixFreeDecoder`` (:53-88), ``PrefixFreeTree`` (:91-224).  A subclass supplies the code (``encode_symbol`` /
``decode_symbol``, or a ``tree`` / ``encoding_table`` attribute); ``encode_block`` / ``decode_block`` upload the code
table once and run on the device.  Kernels: ``csrc/scl_prefix.hip``.

The stream is the block's codewords back to back: no size header, so ``decode_block`` needs the exact bit length and
tolerates no trailing bits -- as in the reference.
"""
from __future__ import annotations

import abc
from dataclasses import dataclass
from typing import Any, Mapping, Tuple

import numpy as np

from ..backend.models import PrefixModel
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..utils.bitarray_utils import BitArray
from ._common import check_alphabet, indices_to_block, symbols_to_indices

__all__ = ["BinaryNode", "PrefixFreeTree", "PrefixFreeEncoder", "PrefixFreeDecoder", "MAX_CODE_BITS"]

MAX_CODE_BITS = 32  # the kernels carry a codeword in one 32-bit word


@dataclass
class BinaryNode:
    """node of a binary code tree: a leaf carries its symbol in ``id`` (reference scl/utils/tree_utils.py)"""

    id: Any = None
    left_child: Any = None
    right_child: Any = None

    @property
    def is_leaf_node(self) -> bool:
        return self.left_child is None and self.right_child is None


class PrefixFreeTree:
    """a prefix-free code as a binary tree: left edge = bit 0, right edge = bit 1"""

    def __init__(self, root_node: BinaryNode):
        self.root_node = root_node

    def get_encoding_table(self) -> Mapping[Any, BitArray]:
        """{symbol: codeword}, in depth-first order, left subtree first (the reference's key order)"""
        table = {}
        stack = [(self.root_node, "")]
        while stack:
            node, code = stack.pop()
            if node.is_leaf_node:
                table[node.id] = BitArray(code)
                continue
            if node.right_child is not None:
                stack.append((node.right_child, code + "1"))
            if node.left_child is not None:
                stack.append((node.left_child, code + "0"))
        return table

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        """-> (symbol, number of bits of its codeword), read from the front of ``encoded_bitarray``"""
        node, used = self.root_node, 0
        while not node.is_leaf_node:
            node = node.right_child if encoded_bitarray[used] else node.left_child
            used += 1
        return node.id, used

    @classmethod
    def build_prefix_free_tree_from_code(cls, codes: Mapping[Any, BitArray]) -> "PrefixFreeTree":
        tree = PrefixFreeTree(BinaryNode())
        for symbol, code in codes.items():
            assert isinstance(code, BitArray), "code should be a bitarray"
            node = tree.root_node
            for bit in code:
                side = "right_child" if bit else "left_child"
                if getattr(node, side) is None:
                    setattr(node, side, BinaryNode())
                node = getattr(node, side)
            node.id = symbol
        return tree


def code_table_arrays(table: Mapping[Any, BitArray]):
    """{symbol: codeword} -> (alphabet in table order, uint32 codes, uint8 lengths); a codeword longer than the kernels'
    32 bits raises ``NotImplementedError`` naming its length"""
    alphabet = list(table)
    check_alphabet(alphabet)
    codes, lengths = np.zeros(len(alphabet), np.uint32), np.zeros(len(alphabet), np.uint8)
    for i, s in enumerate(alphabet):
        bits = table[s]
        if len(bits) > MAX_CODE_BITS:
            raise NotImplementedError(f"symbol {s!r} has a codeword of {len(bits)} bits: the gfx950 kernels code up to "
                                      f"{MAX_CODE_BITS} bits per symbol")
        codes[i] = int(bits.to01(), 2) if len(bits) else 0
        lengths[i] = len(bits)
    return alphabet, codes, lengths


class _PrefixDevice:
    """the device model of a coder object, made from its code table on first use"""

    _model = None

    def _code_table(self) -> Mapping[Any, BitArray]:
        table = getattr(self, "encoding_table", None)
        if table is None:
            table = self.tree.get_encoding_table()
        return table

    def _device_model(self) -> PrefixModel:
        if self._model is None:
            self._alphabet, codes, lengths = code_table_arrays(self._code_table())
            self._index_of = {s: i for i, s in enumerate(self._alphabet)}
            self._model = PrefixModel(codes, lengths)
        return self._model


class PrefixFreeEncoder(_PrefixDevice, DataEncoder):
    @abc.abstractmethod
    def encode_symbol(self, s) -> BitArray:
        """the codeword of one symbol"""

    def encode_block(self, data_block: DataBlock) -> BitArray:
        """the codewords of the block back to back -- prefix_free_compressors.py:31-50"""
        model = self._device_model()
        packed, nbits = model.encode_host(symbols_to_indices(data_block, self._index_of))
        return BitArray.from_packed(packed, nbits)


class PrefixFreeDecoder(_PrefixDevice, DataDecoder):
    @abc.abstractmethod
    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        """-> (symbol, bits consumed) from the front of the bits"""

    def decode_block(self, bitarray: BitArray) -> Tuple[DataBlock, int]:
        """-> (DataBlock, num_bits_consumed): every bit of ``bitarray`` is decoded -- prefix_free_compressors.py:67-88"""
        model = self._device_model()
        idx, used = model.decode_host(bitarray.packed(), len(bitarray), max_block_size=getattr(self, "max_block_size", None))
        return indices_to_block(idx, self._alphabet), used
