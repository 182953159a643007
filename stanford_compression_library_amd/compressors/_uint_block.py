"""What the three integer coders (Golomb, universal, Elias-delta) share: the choice between the device and the host for a
block, and the host's array layout of "a run of ones, then a few bits".

The device (``backend.models.UintCode``, csrc/scl_uint_block.hip) codes uint32 values whose codewords fit 32 bits; the host
codes everything else: a block below ``UINT_BLOCK_MIN`` values (on decode: bits), a block the device answers with
``ST_SIZE``, and values of 2^32 and more.  Both write the reference's stream, so the choice never shows in the bits.

The choice is made by size alone, never by what hardware is there: from ``UINT_BLOCK_MIN`` on a block NEEDS the device, and
without one (or without memory on it) the call raises ``SclHipError`` like every other coder of this package -- there is no
quiet way back to the host.  That holds for the Elias-delta classes too, which were pure host code before they had this
route, and so for an LZ77 counts section of ``UINT_BLOCK_MIN`` bits and more (the LZ77 classes need the device anyway).

``UintBatchMixin`` adds ``encode_blocks`` / ``decode_blocks`` to the six classes: many blocks in batched launches, one lane per
block (csrc/scl_uint.hip), which carry every uint32 value; see the class.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..backend import lib as _lib
from ..backend.models import UintCode, compact
from ..core.data_block import DataBlock
from ..utils.bitarray_utils import BitArray
from ._stream_batch import MAX_BATCH_BYTES

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
    from .elias_delta_uint_coder import scatter_codewords  # (imported late: that module's classes build on this one)

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


# ---- many blocks at a time: one lane per block (csrc/scl_uint.hip) -----------------------------------------
def code_lengths(code: UintCode, x: np.ndarray) -> np.ndarray:
    """the codeword length of every value of the int64 array ``x`` (0 <= x < 2^32), in array arithmetic"""
    from .elias_delta_uint_coder import bit_length

    x = np.asarray(x, np.int64)
    if code.kind == _lib.UINT_GOLOMB:
        b = code.M.bit_length() - 1
        cutoff = (2 << b) - code.M
        q = x // code.M
        return q + 1 + b + ((x - q * code.M >= cutoff) & (cutoff != code.M))
    if code.kind == _lib.UINT_UNIVERSAL:
        return 2 * np.maximum(bit_length(x), 1)
    n = bit_length(x + 1) - 1
    return 2 * (bit_length(n + 1) - 1) + 1 + n


def _launches(sizes: Sequence[Tuple[int, int]]) -> List[List[int]]:
    """consecutive groups of the items whose (row bytes, slot bytes) are given, such that the rows of a group -- every one as
    wide as its widest -- and its slots each stay within ``MAX_BATCH_BYTES``"""
    groups, row, slot = [], 0, 0
    for i, (r, s) in enumerate(sizes):
        if groups and (len(groups[-1]) + 1) * max(row, r, s, slot) <= MAX_BATCH_BYTES:
            groups[-1].append(i)
            row, slot = max(row, r), max(slot, s)
        else:
            groups.append([i])
            row, slot = r, s
    return groups


class UintBatchMixin:
    """``encode_blocks`` / ``decode_blocks`` of the three encoders and decoders: the blocks that the device carries -- every
    integer in [0, 2^32) -- go through batched launches, one lane per block, every other block through ``encode_block`` /
    ``decode_block`` on its own, so ``result[i]`` is what a loop of those calls gives.  A batched launch NEEDS the device
    (``SclHipError`` without one), as a large block does.  Expects ``self._batch_code()`` -> the ``UintCode``, or None where the
    device has no such code (a Golomb M of 2^31 and more)."""

    def _batch_code(self) -> Optional[UintCode]:
        return self._uint_code()

    def encode_blocks(self, blocks: Sequence[DataBlock]) -> List[BitArray]:
        import torch

        code = self._batch_code()
        out: List[Optional[BitArray]] = [None] * len(blocks)
        rows = []  # (index, uint32 values, stream bits) of the blocks that travel in launches
        for i, block in enumerate(blocks):
            data = block.data_list
            values = np.asarray(data) if code is not None and len(data) else None
            if (values is None or values.dtype.kind not in "iu" or int(values.min()) < 0 or int(values.max()) >= (1 << 32)):
                out[i] = self.encode_block(block)  # in order: what a loop raises, and from which block, is raised here
                continue
            nbits = int(code_lengths(code, values).sum())
            # the writers store whole words; a block whose row or slot is a launch's worth of memory goes alone
            if max(4 * values.size, (nbits + 31) // 32 * 4) > MAX_BATCH_BYTES:
                out[i] = self.encode_block(block)
                continue
            rows.append((i, values.astype(np.uint32), nbits))
        if not rows:
            return out
        _lib.require_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        for group in _launches([((v.size + 3) // 4 * 16, (nbits + 127) // 128 * 16) for _, v, nbits in rows]):
            part = [rows[g] for g in group]
            width = (max(v.size for _, v, _ in part) + 3) // 4 * 4  # rows start on 16-byte boundaries
            stride = max((max(nbits for _, _, nbits in part) + 127) // 128 * 16, 16)
            val = np.zeros((len(part), width), np.uint32)
            for k, (_, v, _) in enumerate(part):
                val[k, :v.size] = v
            lens = torch.from_numpy(np.array([v.size for _, v, _ in part], np.int32)).to(dev)
            enc = code.encode_batch(torch.from_numpy(val.view(np.int32)).to(dev), lens=lens, out_stride=stride)
            dense, offs = compact(enc)
            status, got = enc.status.cpu().numpy(), enc.nbits.cpu().numpy().view(np.uint32)
            if status.any() or (got != np.array([nbits for _, _, nbits in part], np.uint32)).any():
                raise _lib.SclHipError(_lib.E_CHUNK, "scl_uint_encode_batch",
                                       f"chunk status {status[status != 0][:4]}, or a length the host did not expect")
            dense, offs = dense.cpu().numpy(), offs.cpu().numpy()
            for k, (i, _, nbits) in enumerate(part):
                out[i] = BitArray.from_packed(dense[offs[k]: offs[k] + (nbits + 7) // 8], nbits)
        return out

    def decode_blocks(self, bitarrays: Sequence[BitArray]) -> List[Tuple[DataBlock, int]]:
        import torch

        code = self._batch_code()
        name = type(self).__name__
        todo = []  # (index, packed bytes, bits) of the streams that travel in launches
        for i, bits in enumerate(bitarrays):
            n = len(bits)
            # (32-bit stream lengths as int32 tensors; an output row of n // min_len values within a launch's memory)
            if code is not None and 0 < n < (1 << 31) and 4 * (n // code.min_len) <= MAX_BATCH_BYTES:
                todo.append((i, bits.packed(), n))
        found = {}  # index -> (status, values, consumed)
        if todo:
            _lib.require_device()
            dev = torch.device("cuda", torch.cuda.current_device())
        for group in _launches([(4 * (n // code.min_len), (n + 127) // 128 * 16) for _, _, n in todo]):
            part = [todo[g] for g in group]
            starts = np.cumsum([0] + [(p.size + 15) // 16 * 16 for _, p, _ in part])
            buf = np.zeros(int(starts[-1]) + 16, np.uint8)
            for k, (_, p, _) in enumerate(part):
                buf[starts[k]: starts[k] + p.size] = p
            cap = max(max(n // code.min_len for _, _, n in part), 1)
            val, lens, used, status = code.decode_batch(
                torch.from_numpy(buf).to(dev), torch.from_numpy(8 * starts[:-1].astype(np.int64)).to(dev),
                torch.from_numpy(np.array([n for _, _, n in part], np.int32)).to(dev), cap)
            val, lens = val.cpu().numpy().view(np.uint32), lens.cpu().numpy()
            used, status = used.cpu().numpy(), status.cpu().numpy()
            for k, (i, _, _) in enumerate(part):
                found[i] = (int(status[k]), val[k, :lens[k]], int(used[k]))
        out = []
        for i, bits in enumerate(bitarrays):  # in order: what a loop raises, and from which block, is raised here
            status, values, used = found.get(i, (_lib.ST_SIZE, None, 0))
            if status & _lib.ST_SIZE:  # a value of 2^32 and more (or a stream that travelled in no launch): the host's
                out.append(self.decode_block(bits))
            elif status & _lib.ST_TRUNCATED:
                raise truncated(f"{name}.decode_blocks: block {i}")
            elif status:
                raise _lib.SclHipError(_lib.E_CHUNK, "scl_uint_decode_batch", f"block {i}: chunk status 0x{status:x}")
            else:
                out.append((DataBlock(values.tolist()), used))
        return out
