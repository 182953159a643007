"""Sliding-window LZ77 with the reference's class API; with the hash-based match finder the parse and the sequence
execution run on the gfx950 kernels.

Drop-in for reference scl/compressors/lz77_sliding_window.py: ``LZ77Window``, ``MatchFinderBase``, ``HashBasedMatchFinder``,
``LZ77SlidingWindowEncoder`` and ``LZ77SlidingWindowDecoder``.  ``LZ77Sequence`` and the entropy stage
(``LZ77StreamsEncoder`` / ``LZ77StreamsDecoder``) are those of :mod:`.lz77`; the bits equal the reference's for every block.

* With a ``HashBasedMatchFinder`` exactly (not a subclass: a subclass may change any step), the encoder hands the last
  ``window_size`` bytes of its history plus the block to ``backend.lz77.sliding_parse_host`` (csrc/scl_lz77_sliding.hip,
  DESIGN.md 3.6.4), which indexes them anew and implements the finder's rule bit for bit: hash buckets, capped chains, the
  window test, right and left extension, lazy matching at the horizon of the first match.  Older bytes cannot change the
  outcome.  A block below ``backend.lz77.sliding_wide_threshold()`` bytes is parsed on ONE wavefront; from there on the
  host call spreads it over the whole GPU (csrc/scl_lz77_sliding_wide.hip), with the same sequences and
  literals.  ``backend.lz77.sliding_parse_batch`` is the call for many streams.
* Any other ``MatchFinderBase`` runs the reference's host loop over ``find_best_match``, so a user's own finder works; it
  is as slow as Python is.
* The decoder replays on the device with the window's rules: an offset beyond ``min(window_size, bytes so far)`` raises.
  A block of ``sliding_wide_threshold()`` bytes or more is replayed across the whole GPU, with the same bytes and errors.

Parameters the device refuses raise ``NotImplementedError``: ``hash_length`` outside 1..8, ``hash_table_size`` of 2^32 or
more, ``max_chain_length`` outside 1..64, and ``minimum_match_length`` 0, with which the reference loops forever.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from ..backend import lz77 as _dev
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..core.data_stream import Uint8FileDataStream
from ..core.encoded_stream import EncodedBlockReader, EncodedBlockWriter
from ..utils.bitarray_utils import BitArray
from .lz77 import LZ77Decoder, LZ77Sequence, LZ77StreamsDecoder, LZ77StreamsEncoder, _bytes_of

__all__ = ["LZ77Window", "MatchFinderBase", "HashBasedMatchFinder", "LZ77SlidingWindowEncoder", "LZ77SlidingWindowDecoder",
           "LZ77Decoder", "LZ77Sequence", "LZ77StreamsEncoder", "LZ77StreamsDecoder"]

DEFAULT_WINDOW_SIZE = 1000000


class LZ77Window:
    """The last ``size`` bytes of a stream, addressed by their absolute position in it: ``[start, end)`` is what is kept"""

    def __init__(self, size, initial_window=None):
        self.size = size
        self.start = 0
        self.end = 0
        self._kept = np.zeros(0, np.uint8)
        if initial_window is not None:
            self.extend(_bytes_of(initial_window, "initial_window"))

    def extend(self, data: np.ndarray):
        """``append`` for an array of bytes"""
        data = np.asarray(data, np.uint8)
        if self.size <= 0 and data.size:
            raise ZeroDivisionError("a window of size 0 holds no byte")
        self._kept = np.concatenate([self._kept, data])[-self.size:] if self.size > 0 else self._kept
        self.end += int(data.size)
        self.start = self.end - int(self._kept.size)

    def append(self, byte):
        self.extend(np.array([byte], np.uint8))

    def get_byte(self, position):
        if position < self.start or position >= self.end:
            raise IndexError("Position out of range")
        return int(self._kept[position - self.start])

    def get_byte_window_plus_lookahead(self, position, lookahead_buffer):
        """the byte at ``position``: from the window, or, beyond its end, from the lookahead buffer that follows it"""
        if position < self.end:
            return self.get_byte(position)
        return lookahead_buffer[position - self.end]

    def get_window_as_list(self):
        return self._kept.tolist()

    def as_array(self) -> np.ndarray:
        return self._kept


class MatchFinderBase:
    """Interface of a match finder: it is given the window and finds the best match for a lookahead buffer in it"""

    def reset(self):
        pass

    def set_window(self, window):
        self.window = window

    def extend_match(self, match_start_in_lookahead_buffer, match_pos, lookahead_buffer, left_extension=True):
        """Extends a candidate to the right, and to the left inside the lookahead buffer, while the bytes agree.
        -> (start in the lookahead buffer = the number of literals, position in the window, length)"""
        window, n = self.window, len(lookahead_buffer)
        match_length = 0
        while (match_start_in_lookahead_buffer + match_length < n
               and window.get_byte_window_plus_lookahead(match_pos + match_length, lookahead_buffer)
               == lookahead_buffer[match_start_in_lookahead_buffer + match_length]):
            match_length += 1
        if left_extension:
            while (match_pos > window.start and match_start_in_lookahead_buffer > 0
                   and lookahead_buffer[match_start_in_lookahead_buffer - 1]
                   == window.get_byte_window_plus_lookahead(match_pos - 1, lookahead_buffer)):
                match_pos -= 1
                match_length += 1
                match_start_in_lookahead_buffer -= 1
        return match_start_in_lookahead_buffer, match_pos, match_length

    def find_best_match(self, lookahead_buffer):
        """-> (number of literals, match position in the window, match length; 0: none)"""
        raise NotImplementedError


class HashBasedMatchFinder(MatchFinderBase):
    """The reference's hash-chain finder: positions are filed under ``hash(tuple(next hash_length bytes)) %
    hash_table_size``, a chain keeps its ``max_chain_length`` newest positions, a candidate is extended right and left, the
    longest wins (the newest on ties); a match counts from ``minimum_match_length`` bytes, and with ``lazy`` the positions
    behind the first match are tried while each is longer.  On an ``LZ77SlidingWindowEncoder`` the rule runs on the device;
    the object holds the parameters (and ``_hash``, the bucket function of the kernels)."""

    def __init__(self, hash_length=4, hash_table_size=1000000, max_chain_length=64, lazy=True, minimum_match_length=4):
        self.hash_length = hash_length
        self.hash_table_size = hash_table_size
        self.max_chain_length = max_chain_length
        self.lazy = lazy
        self.minimum_match_length = minimum_match_length
        if minimum_match_length < 1:
            raise NotImplementedError(f"minimum_match_length {minimum_match_length}: a match has at least one byte, "
                                      "1 <= minimum_match_length (with 0 the reference does not terminate)")
        if not 1 <= hash_length <= _dev.MAX_HASH_LENGTH:
            raise NotImplementedError(f"hash_length {hash_length}: the gfx950 kernels hash 1 <= hash_length <= "
                                      f"{_dev.MAX_HASH_LENGTH} bytes")
        if not 1 <= hash_table_size <= _dev.MAX_HASH_TABLE_SIZE:
            raise NotImplementedError(f"hash_table_size {hash_table_size}: a bucket number is 32-bit on the device, "
                                      f"1 <= hash_table_size <= {_dev.MAX_HASH_TABLE_SIZE}")
        if not 1 <= max_chain_length <= _dev.MAX_CHAIN_LENGTH:
            raise NotImplementedError(f"max_chain_length {max_chain_length}: the gfx950 parse scores one candidate per "
                                      f"lane of a wavefront, 1 <= max_chain_length <= {_dev.MAX_CHAIN_LENGTH}")

    def _hash(self, data):
        """bucket of the first ``hash_length`` bytes of ``data``"""
        return _dev.sliding_bucket(np.asarray(list(data[: self.hash_length]), np.uint8), self.hash_table_size)

    def params(self, window_size: int) -> "_dev.SlidingParams":
        return _dev.SlidingParams(self.hash_length, self.hash_table_size, self.max_chain_length, bool(self.lazy),
                                  self.minimum_match_length, window_size)

    def find_best_match(self, lookahead_buffer):
        """One sequence's worth of the rule, from the device parse of window + lookahead: the first sequence"""
        history = self.window.as_array()
        data = _bytes_of(lookahead_buffer, "lookahead_buffer")
        lc, ml, mo, _ = _dev.sliding_parse_host(np.concatenate([history, data]), history.size, self.params(self.window.size))
        if lc.size == 0:
            return (0, 0, 0)
        if ml[0] == 0:
            return (int(lc[0]), 0, 0)
        return (int(lc[0]), self.window.end + int(lc[0]) - int(mo[0]), int(ml[0]))


def _check_window_size(window_size):
    if not 1 <= window_size < 1 << 32:
        raise NotImplementedError(f"window_size {window_size}: positions inside a stream are 32-bit, 1 <= window_size < 2^32")


class LZ77SlidingWindowEncoder(DataEncoder):
    """LZ77 over the last ``window_size`` bytes; ``match_finder`` decides the matches.  ``initial_window``: bytes both sides
    know in advance (give the decoder the same)."""

    def __init__(self, match_finder, window_size=DEFAULT_WINDOW_SIZE, initial_window=None):
        _check_window_size(window_size)
        self.match_finder = match_finder
        self.window_size = window_size
        self.window = LZ77Window(window_size, initial_window=initial_window)
        self.match_finder.set_window(self.window)
        self.streams_encoder = LZ77StreamsEncoder()

    def reset(self):
        self.window = LZ77Window(self.window_size)
        self.match_finder.reset()
        self.match_finder.set_window(self.window)

    def lz77_parse_and_generate_sequences(self, data):
        """-> (sequences, literals) of the block ``data`` (bytes); the block joins the window"""
        block = _bytes_of(data.data_list if isinstance(data, DataBlock) else data, "data")
        if type(self.match_finder) is HashBasedMatchFinder:
            history = self.window.as_array()
            if history.size + block.size >= 1 << 32:
                raise ValueError(f"window and block of {history.size + block.size} bytes: positions are 32-bit")
            lc, ml, mo, literals = _dev.sliding_parse_host(np.concatenate([history, block]), history.size,
                                                           self.match_finder.params(self.window_size))
            self.window.extend(block)
            return [LZ77Sequence(*t) for t in zip(lc.tolist(), ml.tolist(), mo.tolist())], literals.tolist()
        return self._parse_on_host(block.tolist())

    def _parse_on_host(self, data: list):
        """the reference's loop over ``match_finder.find_best_match``, for finders the device does not know"""
        pos, sequences, literals = 0, [], []
        while pos < len(data):
            literals_count, match_pos, match_length = self.match_finder.find_best_match(data[pos:])
            offset = self.window.end + literals_count - match_pos if match_length > 0 else 0
            literals.extend(data[pos: pos + literals_count])
            sequences.append(LZ77Sequence(literals_count, match_length, offset))
            done = literals_count + match_length
            if done <= 0:
                raise ValueError("the match finder returned an empty sequence")
            self.window.extend(np.asarray(data[pos: pos + done], np.uint8))
            pos += done
        return sequences, literals

    def encode_block(self, data_block: DataBlock) -> BitArray:
        sequences, literals = self.lz77_parse_and_generate_sequences(data_block.data_list)
        return self.streams_encoder.encode_block(sequences, literals)

    def encode_file(self, input_file_path: str, encoded_file_path: str, block_size: int = 10000):
        """binary file -> framed block file"""
        with Uint8FileDataStream(input_file_path, "rb") as fds:
            with EncodedBlockWriter(encoded_file_path) as writer:
                self.encode(fds, block_size=block_size, encode_writer=writer)


class LZ77SlidingWindowDecoder(DataDecoder):
    """``window_size`` must be at least the encoder's; ``initial_window`` the same"""

    def __init__(self, window_size=DEFAULT_WINDOW_SIZE, initial_window=None):
        _check_window_size(window_size)
        self.window_size = window_size
        self.window = LZ77Window(window_size, initial_window=initial_window)
        self.streams_decoder = LZ77StreamsDecoder()

    def execute_lz77_sequences(self, literals: List, lz77_sequences: List[LZ77Sequence]) -> list:
        """-> the bytes the sequences and the literals stand for; they join the window.  An offset beyond the window or
        beyond the bytes so far raises ``SclHipError`` naming the status (the reference: ``IndexError``)."""
        fields = [[getattr(s, f) for s in lz77_sequences] for f in ("literal_count", "match_length", "match_offset")]
        if any(v < 0 or v >= 1 << 32 for f in fields for v in f):
            raise ValueError("sequence fields are unsigned 32-bit integers")
        new = _dev.sliding_replay_host(self.window.as_array(), *fields, _bytes_of(literals, "literals"), self.window_size)
        self.window.extend(new)
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
