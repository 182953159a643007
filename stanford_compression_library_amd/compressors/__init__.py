"""The drop-in coder classes, by the reference's module names; the prefix-free family and the integer codes are also
exported here."""
from .golomb_coder import GolombCodeParams, GolombUintDecoder, GolombUintEncoder
from .huffman_coder import HuffmanDecoder, HuffmanEncoder, HuffmanNode, HuffmanTree
from .prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder, PrefixFreeTree
from .universal_uint_coder import UniversalUintDecoder, UniversalUintEncoder

__all__ = ["GolombCodeParams", "GolombUintDecoder", "GolombUintEncoder", "HuffmanDecoder", "HuffmanEncoder", "HuffmanNode",
           "HuffmanTree", "PrefixFreeDecoder", "PrefixFreeEncoder", "PrefixFreeTree", "UniversalUintDecoder",
           "UniversalUintEncoder"]
