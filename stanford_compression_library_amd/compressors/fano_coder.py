"""Fano codes with the reference's class API, blocks coded by the gfx950 prefix-code kernels.

Drop-in for reference scl/compressors/fano_coder.py.  The tree is built on the host by the reference's rule: the symbols
sorted by decreasing probability are cut in two where the cumulative probability in front of a symbol comes nearest to one
half -- the FIRST such symbol when several are equally near (``min`` with a key) -- the symbols in front of the cut hang
under the left edge (bit 0), the others under the right; each half is renormalised to sum to one and cut again until a
symbol stands alone.  The renormalisation is part of the rule: the cut of a half is taken on the rounded quotients, not on
the original probabilities.  Blocks go through the inherited ``PrefixFreeEncoder.encode_block`` /
``PrefixFreeDecoder.decode_block`` (csrc/scl_prefix.hip).
"""
from __future__ import annotations

from typing import Any, Tuple

from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray
from .prefix_free_compressors import BinaryNode, PrefixFreeDecoder, PrefixFreeEncoder, PrefixFreeTree

__all__ = ["FanoTree", "FanoEncoder", "FanoDecoder"]


class FanoTree(PrefixFreeTree):
    def __init__(self, prob_dist: ProbabilityDist):
        self.prob_dist = prob_dist
        self.sorted_prob_dist = ProbabilityDist.get_sorted_prob_dist(prob_dist.prob_dict, descending=True)
        self.root_node = BinaryNode(id=None)
        super().__init__(root_node=self.build_fano_tree(self.root_node, self.sorted_prob_dist))

    @staticmethod
    def _split_prob_dist_into_two(norm_sort_prob_dist: ProbabilityDist):
        """a sorted distribution that sums to one -> ({symbol: p} in front of the cut, {symbol: p} from the cut on)"""
        in_front = norm_sort_prob_dist.cumulative_prob_dict
        cut = min(in_front.items(), key=lambda item: abs(item[1] - 0.5))[0]
        symbols = list(in_front)
        at = symbols.index(cut)
        left = {s: norm_sort_prob_dist.probability(s) for s in symbols[:at]}
        right = {s: norm_sort_prob_dist.probability(s) for s in symbols[at:]}
        return left, right

    @staticmethod
    def build_fano_tree(root_node: BinaryNode, norm_sort_prob_dist: ProbabilityDist) -> BinaryNode:
        """hangs the code tree of the distribution under ``root_node`` and returns it"""
        halves = FanoTree._split_prob_dist_into_two(norm_sort_prob_dist)
        for side, half in zip(("left_child", "right_child"), halves):
            child = getattr(root_node, side)
            if child is None:
                child = BinaryNode(id=None)
                setattr(root_node, side, child)
            if len(half) == 1:
                child.id = next(iter(half))
            else:
                child.id = None
                FanoTree.build_fano_tree(child, ProbabilityDist.normalize_prob_dict(half))
        return root_node


class FanoEncoder(PrefixFreeEncoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.encoding_table = FanoTree(prob_dist).get_encoding_table()

    def encode_symbol(self, s) -> BitArray:
        return self.encoding_table[s]


class FanoDecoder(PrefixFreeDecoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.tree = FanoTree(prob_dist)

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        return self.tree.decode_symbol(encoded_bitarray)
