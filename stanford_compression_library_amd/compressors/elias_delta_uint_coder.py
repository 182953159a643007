"""Elias-delta code of unsigned integers, with the reference's class API (host numpy).

Drop-in for reference scl/compressors/elias_delta_uint_coder.py: ``EliasDeltaUintEncoder`` (:37-64),
``EliasDeltaUintDecoder`` (:67-115).  x >= 0 is coded through y = x + 1: with n = bit length of y minus one and l = bit
length of (n + 1) minus one, the codeword is l zeros, n + 1 in l + 1 bits, and the n bits of y below its leading one.
LZ77 codes its symbol counts with it (a few hundred values per block), so small blocks are host code: whole blocks are laid
out with array operations, one pass per bit of the longest codeword.  From ``UINT_BLOCK_MIN`` values (on decode: bits) on a
block goes to the gfx950 kernels (csrc/scl_uint_block.hip, routed by compressors/_uint_block.py), which write and read the
same bits; a block with a codeword above 32 bits (x >= 2^24 - 1) comes back to the host.  Such a block needs the device:
without one the call raises ``SclHipError``, it does not fall back.

``encode_blocks`` / ``decode_blocks`` code many blocks at a time, one wavefront lane per block (csrc/scl_uint.hip, every
uint32 value): ``_uint_block.UintBatchMixin``.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray
from . import _uint_block

__all__ = ["EliasDeltaUintEncoder", "EliasDeltaUintDecoder"]

_VECTOR_LIMIT = 1 << 50  # below it a codeword (<= 61 bits) fits one uint64


def scatter_codewords(values: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """bits (uint8 0/1) of the codewords back to back: codeword i = the ``lengths[i]`` low bits of ``values[i]``, most
    significant first"""
    values, lengths = np.asarray(values, np.uint64), np.asarray(lengths, np.int64)
    ends = np.cumsum(lengths)
    starts = ends - lengths
    bits = np.zeros(int(ends[-1]) if lengths.size else 0, np.uint8)
    for j in range(int(lengths.max(initial=0))):
        has = lengths > j
        bits[starts[has] + j] = (values[has] >> (lengths[has] - 1 - j).astype(np.uint64)) & np.uint64(1)
    return bits


def bit_length(v: np.ndarray) -> np.ndarray:
    """exact bit length of every (positive, < 2^63) entry of an integer array"""
    v = np.asarray(v, np.int64)
    b = np.floor(np.log2(np.maximum(v, 1).astype(np.float64))).astype(np.int64)  # off by at most one near powers of two
    b += (v >> np.minimum(b + 1, 62)) > 0
    b -= (v >> b) == 0
    return b + 1


def _device(coder, size: int):
    """(the router, the device's code of this coder object) for a block of ``size`` values / bits, (None, None) below the
    threshold"""
    if size < _uint_block.UINT_BLOCK_MIN:
        return None, None
    return _uint_block, coder._uint_code()


class _EliasDeltaDevice(_uint_block.UintBatchMixin):
    _code = None

    def _uint_code(self):
        if self._code is None:
            self._code = _uint_block.UintCode("elias_delta")
        return self._code


class EliasDeltaUintEncoder(_EliasDeltaDevice, DataEncoder):
    def encode_symbol(self, x: int) -> BitArray:
        assert isinstance(x, int)
        assert x >= 0
        y = uint_to_bitarray(x + 1)
        m = uint_to_bitarray(len(y))  # n + 1 = the bit length of y
        return BitArray((len(m) - 1) * "0") + m + y[1:]

    def encode_block(self, data_block: DataBlock) -> BitArray:
        data = data_block.data_list
        if len(data) == 0:
            return BitArray("")
        route, code = _device(self, len(data))
        if route is not None:
            bits = route.device_encode(code, data)
            if bits is not None:
                return bits
        assert all(isinstance(x, (int, np.integer)) and x >= 0 for x in data)
        if max(data) >= _VECTOR_LIMIT:
            out = BitArray("")
            for x in data:
                out += self.encode_symbol(int(x))
            return out
        y = np.asarray(data, np.int64) + 1
        n = bit_length(y) - 1
        l = bit_length(n + 1) - 1
        low = y - (np.int64(1) << n)
        value = ((n + 1) << n) | low  # the l leading zeros are the codeword's own high bits
        return BitArray._wrap(scatter_codewords(value, 2 * l + 1 + n))


class EliasDeltaUintDecoder(_EliasDeltaDevice, DataDecoder):
    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[int, int]:
        used = 0
        while encoded_bitarray[used] != 1:
            used += 1
        l = used
        n = bitarray_to_uint(encoded_bitarray[used: used + l + 1]) - 1
        used += l + 1
        y = 1 if n == 0 else bitarray_to_uint(BitArray("1") + encoded_bitarray[used: used + n])
        return y - 1, used + n

    def decode_block(self, bitarray: BitArray) -> Tuple[DataBlock, int]:
        """every bit of ``bitarray`` is decoded (reference :98-115)"""
        route, code = _device(self, len(bitarray))
        if route is not None:
            got = route.device_decode(code, bitarray)
            if got is not None:
                return got
        bits = bitarray._b
        total = int(bits.size)
        ones = np.flatnonzero(bits)
        text = bitarray.to01()
        out, used = [], 0
        while used < total:
            at = int(np.searchsorted(ones, used))
            if at == ones.size:
                raise IndexError("bitarray index out of range")  # zeros to the end: what indexing past it raises
            first_one = int(ones[at])
            l = first_one - used
            n = int(text[first_one: first_one + l + 1], 2) - 1
            used = first_one + l + 1
            low = text[used: used + n]
            out.append((1 << n) + (int(low, 2) if low else 0) - 1 if n else 0)
            used += n
        return DataBlock(out), used
