"""Huffman coding with the reference's class API; blocks are coded by the gfx950 prefix-code kernels.

Drop-in for reference scl/compressors/huffman_coder.py: ``HuffmanNode`` (:18-35), ``HuffmanTree`` (:38-93),
``HuffmanEncoder`` (:96-108), ``HuffmanDecoder`` (:111-123).  The tree is built on the host -- it decides the code, and
the reference's codes are tree-shaped, not canonical -- by the reference's rule: one leaf per symbol in alphabet order,
``heapq.heapify``, then pop two nodes (first = left child = bit 0, second = right child = bit 1) and push a node with
their float sum.  Ties are decided by the node order alone: ``a < b`` holds exactly when ``a.prob <= b.prob`` (the
reference defines ``__le__`` under ``total_ordering``), so no tie-break key may be added.
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass
from typing import Any, Tuple

from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray
from .prefix_free_compressors import BinaryNode, PrefixFreeDecoder, PrefixFreeEncoder, PrefixFreeTree

__all__ = ["HuffmanNode", "HuffmanTree", "HuffmanEncoder", "HuffmanDecoder"]


@dataclass(eq=False)
class HuffmanNode(BinaryNode):
    prob: float = None

    def __lt__(self, other):  # what heapq asks; total_ordering derives it from __le__ for distinct nodes
        return self.prob <= other.prob


class HuffmanTree(PrefixFreeTree):
    def __init__(self, prob_dist: ProbabilityDist):
        self.prob_dist = prob_dist
        super().__init__(root_node=self.build_huffman_tree())

    def build_huffman_tree(self) -> HuffmanNode:
        alphabet = self.prob_dist.alphabet
        if len(alphabet) == 1:  # the code "0": the root has a left child only
            return HuffmanNode(left_child=HuffmanNode(id=alphabet[0], prob=1.0), prob=1.0)
        heap = [HuffmanNode(id=a, prob=self.prob_dist.probability(a)) for a in alphabet]
        heapq.heapify(heap)
        while len(heap) > 1:
            first = heapq.heappop(heap)
            second = heapq.heappop(heap)
            heapq.heappush(heap, HuffmanNode(left_child=first, right_child=second, prob=first.prob + second.prob))
        return heap[0]


class HuffmanEncoder(PrefixFreeEncoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.encoding_table = HuffmanTree(prob_dist).get_encoding_table()

    def encode_symbol(self, s) -> BitArray:
        return self.encoding_table[s]


class HuffmanDecoder(PrefixFreeDecoder):
    def __init__(self, prob_dist: ProbabilityDist):
        self.tree = HuffmanTree(prob_dist)

    def decode_symbol(self, encoded_bitarray: BitArray) -> Tuple[Any, int]:
        return self.tree.decode_symbol(encoded_bitarray)
