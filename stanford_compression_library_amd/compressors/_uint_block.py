"""What the three integer coders (Golomb, universal, Elias-delta) share: the choice between the device and the host for a
block, and the host's array layout of "a run of ones, then a few bits".

The device (``backend.models.UintCode``, csrc/scl_uint_block.hip) codes uint32 values whose codewords fit 32 bits; the host
codes everything else: a block below ``UINT_BLOCK_MIN`` values (on decode: bits), a block the device answers with
``ST_SIZE``, and values of 2^32 and more.  Both write the reference's stream, so the choice never shows in the bits.

The choice is made by size alone, never by what hardware is there: from ``UINT_BLOCK_MIN`` on a block NEEDS the device, and
without one (or without memory on it) the call raises ``SclHipError`` like every other coder of this package -- there is no
quiet way back to the host.  That holds for the Elias-delta classes too, which were pure host code before they had this
route, and so for an LZ77 counts section of ``UINT_BLOCK_MIN`` bits and more (the LZ77 classes need the device anyway).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from ..backend import lib as _lib
from ..backend.models import UintCode
from ..core.data_block import DataBlock
from ..utils.bitarray_utils import BitArray
from .elias_delta_uint_coder import scatter_codewords

# A block of at least this many values -- on decode: a stream of at least this many bits -- goes to the device.  Measured,
# not chosen: encode_block / decode_block end to end, host path against device path, 1 Ki to 1 Mi values in steps of 4x, best
# of 3 (tools/bench_uint_codes.py, profiles/uint_codes_bench.txt); the smallest swept size from
# which the device was never the slower one, for any of the three codes, on encode and on decode.  At 1 Ki values the host
# still wins Golomb's encode (0.111 against 0.117 ms); from 4 Ki on the device wins every row, 2x on encode and 6x to 33x on
# decode there already.
UINT_BLOCK_MIN = 1 << 12

VECTOR_LIMIT = 1 << 62  # below it the host's int64 arithmetic holds a value and its remainder code


def truncated(what: str) -> _lib.SclHipError:
    """what a stream that ends inside a codeword raises: the error of ``PrefixModel.decode_host`` for the same fault"""
    return _lib.SclHipError(_lib.E_CHUNK, what, f"{what}: chunk status 0x{_lib.ST_TRUNCATED:x} TRUNCATED")


def lay_unary_then(ones: np.ndarray, values: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """bits (uint8 0/1) of the codewords back to back: codeword i = ``ones[i]`` ones, then the ``lengths[i]`` low bits of
    ``values[i]``, most significant first"""
    ones, lengths = np.asarray(ones, np.int64), np.asarray(lengths, np.int64)
    tails = scatter_codewords(values, lengths)
    bits = np.ones(int(ones.sum()) + tails.size, np.uint8)
    bits[np.repeat(np.cumsum(ones), lengths) + np.arange(tails.size)] = tails
    return bits


def as_vector(data) -> Optional[np.ndarray]:
    """the block as an int64 array if every value is an integer in [0, VECTOR_LIMIT), else None"""
    if not all(isinstance(x, (int, np.integer)) for x in data):
        return None
    if min(data) < 0 or max(data) >= VECTOR_LIMIT:
        return None
    return np.asarray(data, np.int64)


def device_encode(code: UintCode, data) -> Optional[BitArray]:
    """the block through the device, or None: the host codes it (a small block, a value the device does not carry, or
    anything the host's own checks have to refuse)"""
    if len(data) < UINT_BLOCK_MIN:
        return None
    values = np.asarray(data)
    if values.dtype.kind not in "iu" or int(values.min()) < 0 or int(values.max()) >= (1 << 32):
        return None
    packed, nbits, status = code.encode_host(values.astype(np.uint32))
    if status & _lib.ST_SIZE:
        return None
    if status:
        raise _lib.SclHipError(_lib.E_CHUNK, "scl_uint_encode_block_host", f"block status 0x{status:x}")
    return BitArray.from_packed(packed, nbits)


def device_decode(code: UintCode, bitarray: BitArray) -> Optional[Tuple[DataBlock, int]]:
    """the stream through the device, or None: the host decodes it (a short stream, or one with a codeword above 32 bits)"""
    nbits = len(bitarray)
    if nbits < UINT_BLOCK_MIN:
        return None
    values, used, status = code.decode_host(bitarray.packed(), nbits)
    if status & _lib.ST_SIZE:
        return None
    if status & _lib.ST_TRUNCATED:
        raise truncated("scl_uint_decode_block_host")
    if status:
        raise _lib.SclHipError(_lib.E_CHUNK, "scl_uint_decode_block_host", f"block status 0x{status:x}")
    return DataBlock(values.tolist()), used
