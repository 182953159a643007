"""Shannon-Fano-Elias codes with the reference's class API, blocks coded by the gfx950 prefix-code kernels.

Drop-in for reference scl/compressors/shannon_fano_elias_coder.py.  The codeword of a symbol is the first
``ceil(-log2 p) + 1`` bits of the binary fraction of the midpoint of its interval, ``cumulative + p / 2`` in double, in the
distribution's own order (no sort).  ``encode_symbol`` computes it, ``decode_symbol`` keeps the reference's interval search
(halve [0, 1) bit by bit until the interval lies inside one symbol's), and the device table both classes code blocks with is
``{s: encode_symbol(s)}`` over the alphabet (``PrefixFreeEncoder.encode_block`` / ``PrefixFreeDecoder.decode_block``,
csrc/scl_prefix.hip).
"""
from __future__ import annotations

import math
from typing import Any, Tuple

import numpy as np

from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray
from .prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder
from .shannon_coder import fraction_codeword

__all__ = ["ShannonFanoEliasEncoder", "ShannonFanoEliasDecoder"]


def _codeword_length(prob_dist: ProbabilityDist, symbol) -> int:
    return math.ceil(prob_dist.neg_log_probability(symbol)) + 1


class ShannonFanoEliasEncoder(PrefixFreeEncoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.prob_dist = prob_dist
        self.cumulative_prob_dict = self.prob_dist.cumulative_prob_dict

    def encode_symbol(self, symbol) -> BitArray:
        midpoint = self.cumulative_prob_dict[symbol] + self.prob_dist.probability(symbol) / 2
        return fraction_codeword(symbol, midpoint, _codeword_length(self.prob_dist, symbol))

    def _code_table(self):
        return {s: self.encode_symbol(s) for s in self.prob_dist.alphabet}


class ShannonFanoEliasDecoder(PrefixFreeDecoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.prob_dist = prob_dist
        self.cumulative_prob_dict = self.prob_dist.cumulative_prob_dict

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        """-> (symbol, bits of its codeword): the symbol is known as soon as the dyadic interval the bits name lies inside
        its interval, which can be before the codeword ends; the codeword's own length is what is consumed"""
        starts = list(self.cumulative_prob_dict.values())
        lo, hi, used = 0.0, 1.0, 0
        while True:
            mid = (lo + hi) / 2
            if encoded_bitarray[used]:
                lo = mid
            else:
                hi = mid
            used += 1
            first = np.searchsorted(starts, lo, side="right")
            last = np.searchsorted(starts, hi, side="left")
            if first == last:
                symbol = self.prob_dist.alphabet[first - 1]
                return symbol, _codeword_length(self.prob_dist, symbol)

    def _code_table(self):
        return ShannonFanoEliasEncoder(self.prob_dist)._code_table()
