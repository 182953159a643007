"""LZ77 with the reference's class API; match finding, the greedy parse and sequence execution run on the gfx950 kernels.

Drop-in for reference scl/compressors/lz77.py: ``LZ77Sequence`` (:115-124), ``EmpiricalIntHuffmanEncoder`` / ``Decoder``
(:127-209), ``LogScaleBinnedIntegerEncoder`` / ``Decoder`` (:212-298), ``LZ77StreamsEncoder`` / ``Decoder`` (:301-428),
``LZ77Encoder`` (:431-623) and ``LZ77Decoder`` (:626-688).  The bits equal the reference's for every block.

* The LZ layer -- what the reference does with a dict of tuples and a byte-by-byte match loop -- is
  ``backend.lz77.parse_host`` / ``replay_host`` (csrc/scl_lz77.hip).  The coder objects keep their window
  across blocks on the host, as the reference does; every block hands the whole window to the device, which indexes it
  anew (the batch API in ``backend.lz77`` is the one to use for many streams).  From ``backend.lz77.wide_threshold()``
  bytes of block on, and with ``max_num_matches_considered`` in 1..64, the library parses and replays the stream across the
  whole GPU (csrc/scl_lz77_wide.hip) instead of on one wavefront: the same sequences, literals and bytes.
* The entropy stage is the reference's layout: each stream of integers is coded with a Huffman code of its own empirical
  counts (``HuffmanEncoder`` / ``HuffmanDecoder``, i.e. the prefix-code kernels), the counts travel Elias-delta coded, sizes
  as 32-bit headers.  Binning, residual bits and headers are array operations on the host.

``min_match_length`` above 8 raises ``NotImplementedError``: the device index carries an L-gram as one 64-bit key.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from ..backend import lz77 as _dev
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..core.data_stream import Uint8FileDataStream
from ..core.encoded_stream import EncodedBlockReader, EncodedBlockWriter
from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray, bitarray_to_uint, uint_to_bitarray
from .elias_delta_uint_coder import EliasDeltaUintDecoder, EliasDeltaUintEncoder, bit_length, scatter_codewords
from .huffman_coder import HuffmanDecoder, HuffmanEncoder

__all__ = ["LZ77Sequence", "EmpiricalIntHuffmanEncoder", "EmpiricalIntHuffmanDecoder", "LogScaleBinnedIntegerEncoder",
           "LogScaleBinnedIntegerDecoder", "LZ77StreamsEncoder", "LZ77StreamsDecoder", "LZ77Encoder", "LZ77Decoder",
           "ENCODED_BLOCK_SIZE_HEADER_BITS", "DEFAULT_MIN_MATCH_LEN", "DEFAULT_MAX_NUM_MATCHES_CONSIDERED"]

ENCODED_BLOCK_SIZE_HEADER_BITS = 32
DEFAULT_MIN_MATCH_LEN = 6
DEFAULT_MAX_NUM_MATCHES_CONSIDERED = 64


@dataclass
class LZ77Sequence:
    """copy ``literal_count`` literals to the output, then ``match_length`` bytes from ``match_offset`` back in it"""

    literal_count: int = 0
    match_length: int = 0
    match_offset: int = 0


def _int_list(values) -> list:
    return values.tolist() if isinstance(values, np.ndarray) else [int(v) for v in values]


class EmpiricalIntHuffmanEncoder(DataEncoder):
    """values in 0..alphabet_size-1 -> [32-bit size][Elias-delta counts of every value of the alphabet]
    [32-bit size][Huffman code of the values under those counts]; an empty block is one zero header"""

    def __init__(self, alphabet_size):
        self.alphabet_size = alphabet_size

    def encode_block(self, data_block: DataBlock) -> BitArray:
        vals = _int_list(data_block.data_list)
        if len(vals) == 0:
            return uint_to_bitarray(0, ENCODED_BLOCK_SIZE_HEADER_BITS)
        arr = np.asarray(vals, np.int64)
        assert arr.min() >= 0 and arr.max() < self.alphabet_size
        counts = np.bincount(arr, minlength=self.alphabet_size)
        # the tree is decided by the order of the distribution: values in ascending order, as the decoder rebuilds it
        total = int(counts.sum())
        dist = ProbabilityDist({int(v): int(counts[v]) / total for v in np.flatnonzero(counts)})
        values_bits = HuffmanEncoder(dist).encode_block(DataBlock(vals))
        counts_bits = EliasDeltaUintEncoder().encode_block(DataBlock(counts.tolist()))
        return (uint_to_bitarray(len(counts_bits), ENCODED_BLOCK_SIZE_HEADER_BITS) + counts_bits
                + uint_to_bitarray(len(values_bits), ENCODED_BLOCK_SIZE_HEADER_BITS) + values_bits)


class EmpiricalIntHuffmanDecoder(DataDecoder):
    def __init__(self, alphabet_size):
        self.alphabet_size = alphabet_size

    def decode_block(self, encoded_bitarray: BitArray) -> Tuple[DataBlock, int]:
        H = ENCODED_BLOCK_SIZE_HEADER_BITS
        counts_size = bitarray_to_uint(encoded_bitarray[:H])
        used = H
        if counts_size == 0:
            return DataBlock([]), used
        counts, counts_used = EliasDeltaUintDecoder().decode_block(encoded_bitarray[used: used + counts_size])
        assert counts_used == counts_size
        used += counts_size
        counts = counts.data_list
        dist = ProbabilityDist.normalize_prob_dict({i: counts[i] for i in range(self.alphabet_size) if counts[i] > 0})
        values_size = bitarray_to_uint(encoded_bitarray[used: used + H])
        used += H
        decoder = HuffmanDecoder(dist)
        decoder.max_block_size = self.max_block_size
        vals, vals_used = decoder.decode_block(encoded_bitarray[used: used + values_size])
        assert vals_used == values_size
        return vals, used + values_size


class LogScaleBinnedIntegerEncoder(DataEncoder):
    """non-negative integers: values below ``offset`` go to the Huffman coder as they are; v >= offset goes as the bin
    offset + floor(log2(v - offset + 1)), followed -- after all the bins -- by the bits of v - offset + 1 below its
    leading one (100 with offset 0: bin 6, residual 37 in 6 bits)"""

    def __init__(self, offset=0, max_num_bins=32):
        self.offset = offset
        self.max_num_bins = max_num_bins + self.offset
        self.empirical_huffman_encoder = EmpiricalIntHuffmanEncoder(alphabet_size=self.max_num_bins)

    def encode_block(self, data_block: DataBlock) -> BitArray:
        vals = np.asarray(_int_list(data_block.data_list), np.int64)
        assert vals.size == 0 or vals.min() >= 0
        binned = vals >= self.offset
        plus_1 = vals[binned] - self.offset + 1
        log = bit_length(plus_1) - 1
        if log.size and log.max() >= self.max_num_bins:
            big = int(plus_1[np.argmax(log)]) - 1
            raise ValueError(f"Value {big} is too large to be encoded with {self.max_num_bins} bins")
        bins = vals.copy()
        bins[binned] = log + self.offset
        bins_bits = self.empirical_huffman_encoder.encode_block(DataBlock(bins.tolist()))
        residual_bits = scatter_codewords(plus_1 - (np.int64(1) << log), log)
        return bins_bits + BitArray._wrap(residual_bits)


class LogScaleBinnedIntegerDecoder(DataDecoder):
    def __init__(self, offset=0, max_num_bins=32):
        self.offset = offset
        self.max_num_bins = max_num_bins + self.offset
        self.empirical_huffman_decoder = EmpiricalIntHuffmanDecoder(alphabet_size=self.max_num_bins)

    def decode_block(self, encoded_bitarray: BitArray) -> Tuple[DataBlock, int]:
        self.empirical_huffman_decoder.max_block_size = self.max_block_size
        bins, used = self.empirical_huffman_decoder.decode_block(encoded_bitarray)
        bins = np.asarray(bins.data_list, np.int64)
        binned = bins >= self.offset
        log = bins[binned] - self.offset
        ends = np.cumsum(log)
        n_residual = int(ends[-1]) if log.size else 0
        bits = encoded_bitarray._b[used: used + n_residual].astype(np.int64)
        if bits.size != n_residual:
            raise ValueError("the residual bits end before the last value")
        starts = ends - log
        residual = np.zeros(log.size, np.int64)
        for j in range(int(log.max(initial=0))):
            has = log > j
            residual[has] = (residual[has] << 1) | bits[starts[has] + j]
        out = bins.copy()
        out[binned] = self.offset + (np.int64(1) << log) + residual - 1
        return DataBlock(out.tolist()), used + n_residual


class LZ77StreamsEncoder(DataEncoder):
    """sequences and literals -> bits: literal counts, match lengths and match offsets each through a
    ``LogScaleBinnedIntegerEncoder``, then the literals through an ``EmpiricalIntHuffmanEncoder`` over the 256 bytes"""

    def __init__(self, log_scale_binned_coder_offset=16):
        self.log_scale_binned_coder_offset = log_scale_binned_coder_offset

    def encode_lz77_sequences(self, lz77_sequences: List[LZ77Sequence]) -> BitArray:
        coder = LogScaleBinnedIntegerEncoder(offset=self.log_scale_binned_coder_offset)
        out = BitArray()
        for field in ("literal_count", "match_length", "match_offset"):
            out += coder.encode_block(DataBlock([getattr(s, field) for s in lz77_sequences]))
        return out

    def encode_literals(self, literals: List) -> BitArray:
        return EmpiricalIntHuffmanEncoder(alphabet_size=256).encode_block(DataBlock(literals))

    def encode_block(self, lz77_sequences: List[LZ77Sequence], literals: List) -> BitArray:
        return self.encode_lz77_sequences(lz77_sequences) + self.encode_literals(literals)


class LZ77StreamsDecoder(DataDecoder):
    def __init__(self, log_scale_binned_coder_offset=16):
        self.log_scale_binned_coder_offset = log_scale_binned_coder_offset

    def decode_lz77_sequences(self, encoded_bitarray: BitArray):
        coder = LogScaleBinnedIntegerDecoder(offset=self.log_scale_binned_coder_offset)
        coder.max_block_size = self.max_block_size
        fields, used = [], 0
        for _ in range(3):
            block, n = coder.decode_block(encoded_bitarray[used:])
            fields.append(block.data_list)
            used += n
        return [LZ77Sequence(*t) for t in zip(*fields)], used

    def decode_literals(self, encoded_bitarray: BitArray):
        decoder = EmpiricalIntHuffmanDecoder(alphabet_size=256)
        decoder.max_block_size = self.max_block_size
        literals, used = decoder.decode_block(encoded_bitarray)
        return literals.data_list, used

    def decode_block(self, encoded_bitarray: BitArray):
        sequences, used_sequences = self.decode_lz77_sequences(encoded_bitarray)
        literals, used_literals = self.decode_literals(encoded_bitarray[used_sequences:])
        return (sequences, literals), used_sequences + used_literals


def _bytes_of(symbols, what: str) -> np.ndarray:
    arr = np.asarray(_int_list(symbols), np.int64)
    if arr.size and (arr.min() < 0 or arr.max() > 255):
        raise ValueError(f"{what}: LZ77 codes bytes (0..255)")
    return arr.astype(np.uint8)


class LZ77Encoder(DataEncoder):
    """Greedy LZ77: at every position take the longest match among the ``max_num_matches_considered`` most recent earlier
    occurrences of the next ``min_match_length`` bytes (0 = all of them; the most recent wins ties), else move on and
    keep the byte as a literal.  The window -- everything seen, ``initial_window`` first -- lives until ``reset()``."""

    def __init__(self, min_match_length: int = DEFAULT_MIN_MATCH_LEN,
                 max_num_matches_considered: int = DEFAULT_MAX_NUM_MATCHES_CONSIDERED, initial_window: List = None):
        if not 1 <= min_match_length <= _dev.MAX_MIN_MATCH_LENGTH:
            raise NotImplementedError(f"min_match_length {min_match_length}: the gfx950 match index keys a substring as one "
                                      f"64-bit word, 1 <= min_match_length <= {_dev.MAX_MIN_MATCH_LENGTH}")
        self.min_match_length = min_match_length
        self.max_num_matches_considered = max_num_matches_considered
        self._window = np.zeros(0, np.uint8)
        if initial_window is not None:
            self._window = _bytes_of(initial_window, "initial_window")
        self.streams_encoder = LZ77StreamsEncoder()

    @property
    def window(self) -> list:
        return self._window.tolist()

    def reset(self):
        self._window = np.zeros(0, np.uint8)

    def lz77_parse_and_generate_sequences(self, data_block: DataBlock):
        """-> (sequences, literals) of the block; the block joins the window"""
        start = int(self._window.size)
        window = np.concatenate([self._window, _bytes_of(data_block.data_list, "data_block")])
        if window.size >= 1 << 32:
            raise ValueError(f"a window of {window.size} bytes: positions inside a stream are 32-bit; call reset()")
        lc, ml, mo, literals = _dev.parse_host(window, start, self.min_match_length, self.max_num_matches_considered)
        self._window = window
        return [LZ77Sequence(*t) for t in zip(lc.tolist(), ml.tolist(), mo.tolist())], literals.tolist()

    def encode_block(self, data_block: DataBlock) -> BitArray:
        sequences, literals = self.lz77_parse_and_generate_sequences(data_block)
        return self.streams_encoder.encode_block(sequences, literals)

    def encode_file(self, input_file_path: str, encoded_file_path: str, block_size: int = 10000):
        """binary file -> framed block file"""
        with Uint8FileDataStream(input_file_path, "rb") as fds:
            with EncodedBlockWriter(encoded_file_path) as writer:
                self.encode(fds, block_size=block_size, encode_writer=writer)


class LZ77Decoder(DataDecoder):
    def __init__(self, initial_window: List = None):
        self._window = np.zeros(0, np.uint8)
        if initial_window is not None:
            self._window = _bytes_of(initial_window, "initial_window")
        self.streams_decoder = LZ77StreamsDecoder()

    @property
    def window(self) -> list:
        return self._window.tolist()

    def execute_lz77_sequences(self, literals: List, lz77_sequences: List[LZ77Sequence]) -> list:
        """-> the bytes the sequences and the literals stand for; they join the window"""
        fields = [[getattr(s, f) for s in lz77_sequences] for f in ("literal_count", "match_length", "match_offset")]
        if any(v < 0 or v >= 1 << 32 for f in fields for v in f):
            raise ValueError("sequence fields are unsigned 32-bit integers")
        new = _dev.replay_host(self._window, *fields, _bytes_of(literals, "literals"))
        self._window = np.concatenate([self._window, new])
        return new.tolist()

    def decode_block(self, encoded_bitarray: BitArray) -> Tuple[DataBlock, int]:
        self.streams_decoder.max_block_size = self.max_block_size
        (sequences, literals), used = self.streams_decoder.decode_block(encoded_bitarray)
        return DataBlock(self.execute_lz77_sequences(literals, sequences)), used

    def decode_file(self, encoded_file_path: str, output_file_path: str):
        """framed block file -> binary file"""
        with EncodedBlockReader(encoded_file_path) as reader:
            with Uint8FileDataStream(output_file_path, "wb") as fds:
                self.decode(reader, fds)
