"""Shannon codes with the reference's class API, blocks coded by the gfx950 prefix-code kernels.

Drop-in for reference scl/compressors/shannon_coder.py.  The code table is built on the host by the reference's rule, float
arithmetic included: symbols sorted by decreasing probability (``ProbabilityDist.get_sorted_prob_dist``, a stable sort, so
ties keep their order), the codeword of a symbol = the first ``ceil(-log2 p)`` bits of the binary fraction of the cumulative
probability in front of it (``float_to_bitarrays``).  Blocks go through the inherited ``PrefixFreeEncoder.encode_block`` /
``PrefixFreeDecoder.decode_block`` (csrc/scl_prefix.hip).
"""
from __future__ import annotations

import math
from typing import Any, Tuple

from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray, float_to_bitarrays
from .prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder, PrefixFreeTree

__all__ = ["ShannonEncoder", "ShannonDecoder"]


def fraction_codeword(symbol, value: float, length: int) -> BitArray:
    """the first ``length`` bits of the binary fraction of ``value``; a code that gives ``symbol`` no bits at all (a symbol
    of probability 1) is no prefix code the kernels could carry: ``ValueError`` naming the symbol"""
    if length < 1:
        raise ValueError(f"symbol {symbol!r} would get a codeword of {length} bits: its probability leaves nothing to code")
    return float_to_bitarrays(value, length)[1]


class ShannonEncoder(PrefixFreeEncoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.prob_dist = prob_dist
        self.encoding_table = ShannonEncoder.generate_shannon_codebook(self.prob_dist)

    @classmethod
    def generate_shannon_codebook(cls, prob_dist: ProbabilityDist):
        """{symbol: codeword}, most probable symbol first"""
        by_prob = ProbabilityDist.get_sorted_prob_dist(prob_dist.prob_dict, descending=True)
        in_front = by_prob.cumulative_prob_dict
        return {s: fraction_codeword(s, in_front[s], math.ceil(by_prob.neg_log_probability(s))) for s in by_prob.prob_dict}

    def encode_symbol(self, s) -> BitArray:
        return self.encoding_table[s]


class ShannonDecoder(PrefixFreeDecoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.tree = PrefixFreeTree.build_prefix_free_tree_from_code(ShannonEncoder.generate_shannon_codebook(prob_dist))

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        return self.tree.decode_symbol(encoded_bitarray)
