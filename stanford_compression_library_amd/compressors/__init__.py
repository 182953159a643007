"""The drop-in coder classes, by the reference's module names; the prefix-free family is also exported here."""
from .huffman_coder import HuffmanDecoder, HuffmanEncoder, HuffmanNode, HuffmanTree
from .prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder, PrefixFreeTree

__all__ = ["HuffmanDecoder", "HuffmanEncoder", "HuffmanNode", "HuffmanTree", "PrefixFreeDecoder", "PrefixFreeEncoder",
           "PrefixFreeTree"]
