"""Golomb code of unsigned integers with the reference's class API; large blocks are coded by the gfx950 kernels.

Drop-in for reference scl/compressors/golomb_coder.py: ``GolombCodeParams`` (:34-51), ``GolombUintEncoder`` (:54-93),
``GolombUintDecoder`` (:96-145).  x >= 0 is coded as q = x // M ones and a zero, then the remainder r = x % M in truncated
binary: with b = floor(log2 M) and cutoff = 2^(b+1) - M, r in b bits if M is a power of two (a Rice code) or r < cutoff,
else r + cutoff in b + 1 bits.

``encode_block`` / ``decode_block`` run on the device (csrc/scl_uint_block.hip) from ``UINT_BLOCK_MIN`` values / bits on and
on the host below it, for codewords above 32 bits and for values of 2^32 and more: compressors/_uint_block.py.  The stream
is the block's codewords back to back either way; ``decode_block`` reads every bit it is given.

``encode_blocks`` / ``decode_blocks`` code many blocks at a time, one wavefront lane per block (csrc/scl_uint.hip, every
uint32 value): ``_uint_block.UintBatchMixin``.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..backend.models import UintCode
from ..core.data_block import DataBlock
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray
from . import _uint_block
from .prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder

__all__ = ["GolombCodeParams", "GolombUintEncoder", "GolombUintDecoder"]


class GolombCodeParams:
    """M, b = floor(log2 M) (exact: the reference takes the logarithm of a float), cutoff = 2^(b+1) - M"""

    def __init__(self, M: int):
        assert M > 0
        self.M = M
        self.b = int(M).bit_length() - 1
        self.cutoff = 2 ** (self.b + 1) - self.M
        self.rice_code = self.cutoff == self.M


class _GolombDevice(_uint_block.UintBatchMixin):
    _code = None

    def _uint_code(self) -> UintCode:
        """the device's code; an M it does not take (2^31 and more) raises, and the block goes to the host"""
        if self._code is None:
            self._code = UintCode("golomb", self.params.M)
        return self._code

    def _on_device(self) -> bool:
        return self.params.M < (1 << 31)

    def _batch_code(self):
        return self._uint_code() if self._on_device() else None


class GolombUintEncoder(_GolombDevice, PrefixFreeEncoder):
    def __init__(self, M: int):
        self.params = GolombCodeParams(M)

    def encode_symbol(self, x: int) -> BitArray:
        assert x >= 0
        assert isinstance(x, int)
        q, r = x // self.params.M, x % self.params.M
        unary = BitArray(q * "1" + "0")
        if self.params.rice_code or r < self.params.cutoff:
            # (b = 0 for M = 1: no remainder bits, where the reference's uint_to_bitarray asserts on a width of 0)
            return unary + (uint_to_bitarray(r, bit_width=self.params.b) if self.params.b else BitArray(""))
        return unary + uint_to_bitarray(r + self.params.cutoff, bit_width=self.params.b + 1)

    def encode_block(self, data_block: DataBlock) -> BitArray:
        data = data_block.data_list
        if len(data) == 0:
            return BitArray("")
        if self._on_device():
            bits = _uint_block.device_encode(self._uint_code(), data)
            if bits is not None:
                return bits
        p = self.params
        x = _uint_block.as_vector(data) if p.M < _uint_block.VECTOR_LIMIT else None
        if x is None:  # huge integers, or what encode_symbol asserts on
            out = BitArray("")
            for v in data:
                out += self.encode_symbol(v if isinstance(v, int) else int(v) if isinstance(v, np.integer) else v)
            return out
        q = x // p.M
        r = x - q * p.M
        longer = (r >= p.cutoff) & (not p.rice_code)
        # the zero that ends the unary part leads the remainder's field
        return BitArray._wrap(_uint_block.lay_unary_then(q, np.where(longer, r + p.cutoff, r), 1 + p.b + longer))


class GolombUintDecoder(_GolombDevice, PrefixFreeDecoder):
    def __init__(self, M: int):
        self.params = GolombCodeParams(M)

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[int, int]:
        used = 0
        while encoded_bitarray[used] != 0:
            used += 1
        q = used
        used += 1
        p = self.params
        r = bitarray_to_uint(encoded_bitarray[used: used + p.b]) if p.b else 0
        used += p.b
        if not p.rice_code and r >= p.cutoff:
            r = 2 * r + int(encoded_bitarray[used]) - p.cutoff
            used += 1
        return p.M * q + r, used

    def decode_block(self, bitarray: BitArray) -> Tuple[DataBlock, int]:
        """every bit of ``bitarray`` is decoded; a stream that ends inside a codeword raises what
        ``PrefixModel.decode_host`` raises for it"""
        if self._on_device():
            got = _uint_block.device_decode(self._uint_code(), bitarray)
            if got is not None:
                return got
        p = self.params
        text, total = bitarray.to01(), len(bitarray)
        out, used = [], 0
        while used < total:
            zero = text.find("0", used)
            if zero < 0 or zero + 1 + p.b > total:
                raise _uint_block.truncated("GolombUintDecoder.decode_block")
            q, used = zero - used, zero + 1
            r = int(text[used: used + p.b], 2) if p.b else 0
            used += p.b
            if not p.rice_code and r >= p.cutoff:
                if used >= total:
                    raise _uint_block.truncated("GolombUintDecoder.decode_block")
                r = 2 * r + int(text[used]) - p.cutoff
                used += 1
            out.append(p.M * q + r)
        return DataBlock(out), used
