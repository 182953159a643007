"""Fixed-width coding with the reference's class API: every symbol of a block costs the same number of bits.

Drop-in for reference scl/compressors/fixed_bitwidth_compressor.py: ``get_alphabet_fixed_bitwidth``,
``FixedBitwidthEncoder`` / ``Decoder`` (alphabet as a pickle), ``TextAlphabetEncoder`` / ``Decoder`` and
``TextFixedBitwidthEncoder`` / ``Decoder`` (alphabet as one byte a character).

A block is ``alphabet_encoder.encode_block(list(data_block.get_alphabet()))``, the block's size in ``DATA_SIZE_BITS`` bits,
then the data section: the index of every symbol in that list, ``w`` bits each, most significant first.  The data section is
what csrc/scl_fixed.hip writes and reads; header and size stay on the host.

The choice between host numpy and the device is made by block size alone, as for the integer codes
(``_uint_block.UINT_BLOCK_MIN``): from ``FIXED_BLOCK_MIN`` symbols on a block NEEDS the device, and without one the call
raises ``SclHipError``.  Both write the same bits.  ``encode_blocks`` / ``decode_blocks`` code many blocks in batched
launches whatever their size.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from ..backend import lib as _lib
from ..backend.models import FixedWidthCode, compact
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..external_compressors.pickle_external import PickleDecoder, PickleEncoder
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray
from ._common import check_alphabet
from ._stream_batch import MAX_BATCH_BYTES
from ._uint_block import _launches, truncated

__all__ = ["get_alphabet_fixed_bitwidth", "FixedBitwidthEncoder", "FixedBitwidthDecoder", "TextAlphabetEncoder",
           "TextAlphabetDecoder", "TextFixedBitwidthEncoder", "TextFixedBitwidthDecoder", "FIXED_BLOCK_MIN"]

# A block of at least this many symbols goes to the device.  Measured, not chosen: encode_block / decode_block end to end,
# host path against device path, 256 symbols (8 bits each), 1 Ki to 1 Mi symbols in steps of 4x, wall clock, best of 3
# (tools/bench_fixed_width.py, profiles/fixed_width_bench.txt); the smallest swept size from which the device
# was never the slower one, on encode and on decode.  ms, host | device:
#      symbols   encode             decode
#        1 Ki     0.049 |  0.114     0.028 |  0.121
#        4 Ki     0.139 |  0.179     0.068 |  0.147
#       16 Ki     0.499 |  0.442     0.236 |  0.276
#       64 Ki     1.939 |  1.502     0.896 |  0.780
#      256 Ki     7.778 |  5.569     3.849 |  2.742
#        1 Mi    37.565 | 22.150    19.300 | 11.165
# Most of either path is the conversion between Python symbols and index arrays, which both pay; the device's share is the
# allocations and the copies of scl_fixed_*_host, not the kernel (a few microseconds at these sizes): at 16 Ki it still
# loses the decode.
FIXED_BLOCK_MIN = 1 << 16


def get_alphabet_fixed_bitwidth(alphabet_size) -> int:
    """bits an index into an alphabet of this size takes: ceil(log2(size)), and 1 for a single symbol (which the reference
    codes in one bit, not none).  An empty alphabet has no width: ``OverflowError``, which is what the reference's
    ``int(ceil(log2(0)))`` raises."""
    size = int(alphabet_size)
    if size <= 0:
        raise OverflowError("cannot convert float infinity to integer: an empty alphabet has no bit width")
    return max(1, (size - 1).bit_length())


# ---- the data section on the host ------------------------------------------------------------------------------------------
def _pack_host(idx: np.ndarray, width: int) -> np.ndarray:
    """indices -> their ``width`` low bits each, most significant first, as one uint8 0/1 array"""
    shifts = np.arange(width - 1, -1, -1, dtype=np.int64)
    return ((idx.astype(np.int64)[:, None] >> shifts) & 1).astype(np.uint8).reshape(-1)


def _unpack_host(bits: np.ndarray, n: int, width: int) -> np.ndarray:
    weights = np.int64(1) << np.arange(width - 1, -1, -1, dtype=np.int64)
    return bits[: n * width].reshape(n, width).astype(np.int64) @ weights


def _raise_status(what: str, status: int):
    if status & _lib.ST_TRUNCATED:
        raise truncated(what)
    if status & _lib.ST_SYMBOL:
        raise IndexError("list index out of range")  # the reference's alphabet[ind]
    if status:
        raise _lib.SclHipError(_lib.E_CHUNK, what, f"chunk status 0x{status:x}")


class FixedBitwidthEncoder(DataEncoder):
    def __init__(self):
        self.alphabet_encoder = PickleEncoder()
        self.DATA_SIZE_BITS = 32

    def _head(self, data_block: DataBlock):
        """-> (header bits, indices, width, alphabet size) of a block"""
        alphabet = list(data_block.get_alphabet())
        check_alphabet(alphabet)
        head = self.alphabet_encoder.encode_block(alphabet)
        assert data_block.size < (1 << self.DATA_SIZE_BITS)
        head = head + uint_to_bitarray(data_block.size, self.DATA_SIZE_BITS)
        width = get_alphabet_fixed_bitwidth(len(alphabet))
        index_of = {a: i for i, a in enumerate(alphabet)}
        data = data_block.data_list
        idx = np.fromiter(map(index_of.__getitem__, data), dtype=np.uint32, count=len(data))
        return head, idx, width, len(alphabet)

    def encode_block(self, data_block: DataBlock) -> BitArray:
        head, idx, width, K = self._head(data_block)
        if idx.size < FIXED_BLOCK_MIN:
            return head + BitArray._wrap(_pack_host(idx, width))
        packed, nbits, status = FixedWidthCode().encode_host(idx, width, K)
        _raise_status("scl_fixed_encode_host", status)
        return head + BitArray.from_packed(packed, nbits)

    def encode_blocks(self, blocks: Sequence[DataBlock]) -> List[BitArray]:
        """``[encode_block(b) for b in blocks]`` in batched launches, every block a stream of its own width; a batched launch
        NEEDS the device, whatever the blocks' sizes"""
        import torch

        heads = [self._head(b) for b in blocks]
        out: List[BitArray] = [None] * len(blocks)
        rows = []
        for i, (head, idx, width, K) in enumerate(heads):
            nbytes = (idx.size * width + 31) // 32 * 4
            if idx.size == 0:
                out[i] = head
            elif max(2 * idx.size, nbytes) > MAX_BATCH_BYTES:
                out[i] = self.encode_block(blocks[i])
            else:
                rows.append((i, idx, width, K))
        if not rows:
            return out
        _lib.require_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        code = FixedWidthCode()
        sizes = [((idx.size + 7) // 8 * 16, code.slot_bytes(idx.size, width)) for _, idx, width, _ in rows]
        for group in _launches(sizes):
            part = [rows[g] for g in group]
            cols = (max(idx.size for _, idx, _, _ in part) + 7) // 8 * 8  # uint16 rows start on 16-byte boundaries
            stride = max(sizes[g][1] for g in group)
            sym = np.zeros((len(part), cols), np.uint16)
            for k, (_, idx, _, _) in enumerate(part):
                sym[k, :idx.size] = idx
            lens = torch.from_numpy(np.array([idx.size for _, idx, _, _ in part], np.int32)).to(dev)
            enc = code.encode_batch(torch.from_numpy(sym.view(np.int16)).to(dev), lens, [w for _, _, w, _ in part],
                                    [K for _, _, _, K in part], out_stride=stride)
            dense, offs = compact(enc)
            status, got = enc.status.cpu().numpy(), enc.nbits.cpu().numpy().view(np.uint32)
            dense, offs = dense.cpu().numpy(), offs.cpu().numpy()
            for k, (i, idx, width, _) in enumerate(part):
                _raise_status("scl_fixed_encode_batch", int(status[k]))
                assert int(got[k]) == idx.size * width
                out[i] = heads[i][0] + BitArray.from_packed(dense[offs[k]: offs[k] + (int(got[k]) + 7) // 8], int(got[k]))
        return out


class FixedBitwidthDecoder(DataDecoder):
    def __init__(self):
        self.alphabet_decoder = PickleDecoder()
        self.DATA_SIZE_BITS = 32

    def _head(self, bitarray: BitArray, what: str):
        """-> (alphabet, block size, width, bits in front of the data section)"""
        alphabet, used = self.alphabet_decoder.decode_block(bitarray)
        if len(bitarray) < used + self.DATA_SIZE_BITS:
            raise truncated(what)
        size = bitarray_to_uint(bitarray[used: used + self.DATA_SIZE_BITS])
        used += self.DATA_SIZE_BITS
        # (a block of no symbols has no alphabet and no data section: nothing asks for a width)
        width = get_alphabet_fixed_bitwidth(len(alphabet)) if size else 1
        if len(bitarray) - used < size * width:
            raise truncated(what)
        return alphabet, size, width, used

    @staticmethod
    def _block(idx, alphabet) -> DataBlock:
        if idx.size and int(idx.max()) >= len(alphabet):
            raise IndexError("list index out of range")
        return DataBlock(list(map(alphabet.__getitem__, idx.tolist())))

    def decode_block(self, bitarray: BitArray) -> Tuple[DataBlock, int]:
        """-> (DataBlock, num_bits_consumed); bits behind the block are left alone"""
        what = f"{type(self).__name__}.decode_block"
        alphabet, size, width, used = self._head(bitarray, what)
        if size < FIXED_BLOCK_MIN:
            idx = _unpack_host(bitarray._b[used:], size, width)
        else:
            idx, consumed, status = FixedWidthCode().decode_host(bitarray.packed(), used, size * width, size, width,
                                                                 len(alphabet))
            _raise_status("scl_fixed_decode_host", status)
            assert consumed == size * width
        return self._block(idx, alphabet), used + size * width

    def decode_blocks(self, bitarrays: Sequence[BitArray]) -> List[Tuple[DataBlock, int]]:
        """``[decode_block(b) for b in bitarrays]`` in batched launches; what a loop raises, and from which block, is raised
        here"""
        import torch

        what = f"{type(self).__name__}.decode_blocks"
        heads, failed = [], None
        for i, bits in enumerate(bitarrays):
            try:
                heads.append(self._head(bits, f"{what}: block {i}"))
            except Exception as e:  # raised when its turn comes: the blocks in front are decoded first
                failed = e
                break
        todo = [(i, bitarrays[i].packed(), h) for i, h in enumerate(heads) if 0 < 2 * h[1] <= MAX_BATCH_BYTES]
        found = {}
        if todo:
            _lib.require_device()
            dev = torch.device("cuda", torch.cuda.current_device())
            code = FixedWidthCode()
        for group in _launches([((h[1] + 7) // 8 * 16, (p.size + 15) // 16 * 16) for _, p, h in todo]):
            part = [todo[g] for g in group]
            starts = np.cumsum([0] + [(p.size + 15) // 16 * 16 for _, p, _ in part])
            buf = np.zeros(int(starts[-1]) + 16, np.uint8)
            for k, (_, p, _) in enumerate(part):
                buf[starts[k]: starts[k] + p.size] = p
            cap = max(h[1] for _, _, h in part)
            offs = np.array([8 * int(starts[k]) + h[3] for k, (_, _, h) in enumerate(part)], np.int64)
            nbits = np.array([h[1] * h[2] for _, _, h in part], np.uint32).view(np.int32)
            lens = np.array([h[1] for _, _, h in part], np.int32)
            val, got, _, status = code.decode_batch(
                torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(nbits).to(dev),
                torch.from_numpy(lens).to(dev), [h[2] for _, _, h in part], [max(len(h[0]), 1) for _, _, h in part], cap,
                dtype=torch.int16)
            val, got, status = val.cpu().numpy().view(np.uint16), got.cpu().numpy(), status.cpu().numpy()
            for k, (i, _, _) in enumerate(part):
                found[i] = (int(status[k]), val[k, :got[k]])
        out = []
        for i, (alphabet, size, width, used) in enumerate(heads):
            if i not in found:
                out.append(self.decode_block(bitarrays[i]))
                continue
            status, idx = found[i]
            _raise_status(f"{what}: block {i}", status)
            out.append((self._block(idx, alphabet), used + size * width))
        if failed is not None:
            raise failed
        return out


class TextAlphabetEncoder(DataEncoder):
    """an alphabet of characters below U+0100: its size in 8 bits, then one byte a character"""

    def __init__(self):
        self.alphabet_size_bits = 8
        self.alphabet_bits = 8

    def encode_block(self, alphabet) -> BitArray:
        assert len(alphabet) < 2 ** self.alphabet_size_bits
        bits = uint_to_bitarray(len(alphabet), self.alphabet_size_bits)
        for ch in alphabet:
            bits += uint_to_bitarray(ord(ch), bit_width=self.alphabet_bits)
        return bits


class TextAlphabetDecoder(DataDecoder):
    def __init__(self):
        self.alphabet_size_bits = 8
        self.alphabet_bits = 8

    def decode_block(self, params_data_bitarray: BitArray):
        """-> (list of characters, bits consumed)"""
        assert len(params_data_bitarray) >= self.alphabet_size_bits
        count = bitarray_to_uint(params_data_bitarray[: self.alphabet_size_bits])
        used = self.alphabet_size_bits
        alphabet = []
        for _ in range(count):
            alphabet.append(chr(bitarray_to_uint(params_data_bitarray[used: used + self.alphabet_bits])))
            used += self.alphabet_bits
        return alphabet, used


class TextFixedBitwidthEncoder(FixedBitwidthEncoder):
    def __init__(self):
        super().__init__()
        self.alphabet_encoder = TextAlphabetEncoder()


class TextFixedBitwidthDecoder(FixedBitwidthDecoder):
    def __init__(self):
        super().__init__()
        self.alphabet_decoder = TextAlphabetDecoder()
