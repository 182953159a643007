"""``PickleEncoder`` / ``PickleDecoder``: any Python object as its pickle, behind a length field.

Drop-in for reference scl/external_compressors/pickle_external.py.  Host code: side information (an alphabet, a
distribution) is a few bytes, and its bits are the interpreter's -- ``pickle.dumps`` with the default protocol -- so the
stream of one interpreter version need not equal that of another.
"""
from __future__ import annotations

import pickle
from typing import Any, Tuple

import numpy as np

from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray

__all__ = ["PickleEncoder", "PickleDecoder"]


class PickleEncoder(DataEncoder):
    def __init__(self, length_bitwidth: int = 32):
        self.length_bitwidth = length_bitwidth

    def encode_block(self, data: Any) -> BitArray:
        """``length_bitwidth`` bits holding the pickle's length in BITS, then the pickle"""
        payload = np.frombuffer(pickle.dumps(data), dtype=np.uint8)
        nbits = 8 * payload.size
        assert nbits < (1 << self.length_bitwidth)
        return uint_to_bitarray(nbits, bit_width=self.length_bitwidth) + BitArray.from_packed(payload, nbits)


class PickleDecoder(DataDecoder):
    def __init__(self, length_bitwidth: int = 32):
        self.length_bitwidth = length_bitwidth

    def decode_block(self, bitarray: BitArray) -> Tuple[Any, int]:
        """-> (the object, bits consumed); bits behind the pickle are left alone"""
        head = self.length_bitwidth
        nbits = bitarray_to_uint(bitarray[:head])
        data = pickle.loads(bitarray[head: head + nbits].tobytes())
        return data, head + nbits
