"""Shared by the prefix-code tests: the Huffman goldens and a numpy restatement of the stream (the codewords of a block
back to back, prefix_free_compressors.py:31-50 of the reference) from a code table the goldens pin."""
import functools

import numpy as np

from conftest import load_golden


@functools.lru_cache(maxsize=None)
def goldens():
    cases = load_golden("huffman")
    return {"table": [c for c in cases if c.kind == "table"], "block": [c for c in cases if c.kind == "block"],
            "file": [c for c in cases if c.kind == "file"], "by_id": {c.id: c for c in cases}}


def table_case(group):
    return next(c for c in goldens()["table"] if c.group == group)


def make_dist(case):
    """the case's distribution over the alphabet 0..K-1 (``unvalidated``: without ProbabilityDist's checks, which
    refuse the probabilities a code of more than 32 bits needs)"""
    from stanford_compression_library_amd.core.prob_dist import ProbabilityDist

    prob_dict = {i: float(p) for i, p in enumerate(case.arr("probs"))}
    if not case.unvalidated:
        return ProbabilityDist(prob_dict)
    dist = ProbabilityDist.__new__(ProbabilityDist)
    dist.prob_dict = prob_dict
    return dist


def code_bits(case):
    """[K] list of uint8 bit arrays: the codeword of every symbol"""
    return [np.array([(int(c) >> (int(n) - 1 - j)) & 1 for j in range(int(n))], np.uint8)
            for c, n in zip(case.arr("code"), case.arr("len"))]


def encode_numpy(bits_of, sym):
    """-> (packed MSB-first bytes, nbits) of one block"""
    parts = [bits_of[int(s)] for s in sym]
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return np.packbits(bits), int(bits.size)


def stream_bits(data, bit_offset, nbits):
    """bits [bit_offset, bit_offset + nbits) of a byte buffer, packed left-aligned"""
    first, last = bit_offset >> 3, (bit_offset + nbits + 7) >> 3
    bits = np.unpackbits(data[first:last])[bit_offset - 8 * first:][:nbits]
    return np.packbits(bits)
