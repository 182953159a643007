"""The reference's simple universal code of unsigned integers, with its class API; large blocks are coded by the gfx950
kernels.

Drop-in for reference scl/compressors/universal_uint_coder.py: ``UniversalUintEncoder`` (:26-61), ``UniversalUintDecoder``
(:64-112).  With L = the bit length of x (1 for 0), x is coded as L - 1 ones, a zero, and x in L bits:
0 -> 00, 1 -> 01, 2 -> 1010, 3 -> 1011, 4 -> 110100.

``encode_block`` / ``decode_block`` run on the device (csrc/scl_uint_block.hip) from ``UINT_BLOCK_MIN`` values / bits on and
on the host below it and for values of 2^16 and more (codewords above 32 bits): compressors/_uint_block.py.

``encode_blocks`` / ``decode_blocks`` code many blocks at a time, one wavefront lane per block (csrc/scl_uint.hip, every
uint32 value): ``_uint_block.UintBatchMixin``.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..backend.models import UintCode
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray
from . import _uint_block
from .elias_delta_uint_coder import bit_length

__all__ = ["UniversalUintEncoder", "UniversalUintDecoder"]


class _UniversalDevice(_uint_block.UintBatchMixin):
    _code = None

    def _uint_code(self) -> UintCode:
        if self._code is None:
            self._code = UintCode("universal")
        return self._code


class UniversalUintEncoder(_UniversalDevice, DataEncoder):
    def encode_symbol(self, x: int) -> BitArray:
        assert isinstance(x, int)
        assert x >= 0
        symbol = uint_to_bitarray(x)
        return BitArray((len(symbol) - 1) * "1" + "0") + symbol

    def encode_block(self, data_block: DataBlock) -> BitArray:
        data = data_block.data_list
        if len(data) == 0:
            return BitArray("")
        bits = _uint_block.device_encode(self._uint_code(), data)
        if bits is not None:
            return bits
        x = _uint_block.as_vector(data)
        if x is None:  # huge integers, or what encode_symbol asserts on
            out = BitArray("")
            for v in data:
                out += self.encode_symbol(v)
            return out
        L = np.maximum(bit_length(x), 1)
        return BitArray._wrap(_uint_block.lay_unary_then(L - 1, x, L + 1))  # the zero leads x's field


class UniversalUintDecoder(_UniversalDevice, DataDecoder):
    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[int, int]:
        used = 0
        while encoded_bitarray[used] != 0:
            used += 1
        used += 1
        ones = used
        return bitarray_to_uint(encoded_bitarray[used: used + ones]), used + ones

    def decode_block(self, bitarray: BitArray) -> Tuple[DataBlock, int]:
        """every bit of ``bitarray`` is decoded; a stream that ends inside a codeword raises what
        ``PrefixModel.decode_host`` raises for it"""
        got = _uint_block.device_decode(self._uint_code(), bitarray)
        if got is not None:
            return got
        text, total = bitarray.to01(), len(bitarray)
        out, used = [], 0
        while used < total:
            zero = text.find("0", used)
            L = zero - used + 1
            if zero < 0 or zero + 1 + L > total:
                raise _uint_block.truncated("UniversalUintDecoder.decode_block")
            out.append(int(text[zero + 1: zero + 1 + L], 2))
            used = zero + 1 + L
        return DataBlock(out), used
