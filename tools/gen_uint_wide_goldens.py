"""Golden vectors of the three integer codes past 32 bits a codeword -- from the *imported reference* (data only).

Runs as tools/gen_uint_goldens.py does, whose cases and ``bitarray`` stand-in it shares:

    cd /tmp && PYTHONPATH=<reference checkout>:<repo> python -W ignore <repo>/tools/gen_uint_wide_goldens.py <repo>/tests/golden

Writes ``golden_uint_wide.npz`` (read by ``conftest.load_golden("uint_wide")``; the fields of a case are those of
``golden_uint_codes.npz``, ``device`` is False throughout: no codeword here fits the block kernels).  Groups, for Golomb M
in 1, 2, 3, 4, 10, 64, 1000, the universal and the Elias-delta code:
  wide       the smallest and the largest value of every codeword length from 33 to 64 bits (lengths the code has, values
             below 2^32)
  quotients  Golomb only: the quotients 31, 32, 33, 63, 64, 65, 1023, 1024, 1025 and 2100, each with the smallest and the
             largest remainder (the short and, where M has one, the long form)
  top        2^32 - 1 between two small values: universal, Elias-delta, and Golomb M = 1000 (a smaller M writes 2^32 / M ones)
No Golomb M just below a power of two: the reference takes b from a float logarithm, which rounds up for 2^31 - 1.
"""
import os
import sys

from gen_uint_goldens import GOLOMB_MS, add_case, coders
from gen_lz77_goldens import Collector

QUOTIENTS = (31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2100)
TOP = (1 << 32) - 1


def wide_values(kind, M):
    """the smallest and the largest value below 2^32 of every codeword length in 33..64, by the reference's own lengths"""
    enc = coders(kind, M)[0]
    length = lambda v: len(enc.encode_symbol(int(v)))  # noqa: E731
    if kind == "universal":
        ends = [((1 << (L - 1)), (1 << L) - 1) for L in range(17, 33)]
    elif kind == "elias_delta":
        ends = [((1 << n) - 1, min((1 << (n + 1)) - 2, TOP)) for n in range(24, 33)]
    else:
        b = M.bit_length() - 1
        cutoff = (2 << b) - M
        ends = []
        for want in range(33, 65):
            if cutoff == M:
                q = want - 1 - b
                ends.append((q * M, q * M + M - 1))
            else:
                ends.append(((want - 2 - b) * M + cutoff, (want - 1 - b) * M + cutoff - 1))
    out = []
    for lo, hi in ends:
        assert 33 <= length(lo) == length(hi) <= 64, (kind, M, lo, hi)
        assert lo == 0 or length(lo - 1) < length(lo), (kind, M, lo)
        assert hi == TOP or length(hi + 1) > length(hi), (kind, M, hi)
        out += [lo, hi]
    return out


def main(out_dir):
    col = Collector()
    for kind, M in [("golomb", M) for M in GOLOMB_MS] + [("universal", 0), ("elias_delta", 0)]:
        add_case(col, kind, M, "wide", wide_values(kind, M))
        if kind == "golomb":
            add_case(col, kind, M, "quotients", [q * M + r for q in QUOTIENTS for r in sorted({0, M - 1})])
        if kind != "golomb" or M == 1000:
            add_case(col, kind, M, "top", [3, TOP, 0])
    path = os.path.join(out_dir, "golden_uint_wide.npz")
    col.save(path)
    assert os.path.getsize(path) < (256 << 10), "the file is meant to stay small"


if __name__ == "__main__":
    main(sys.argv[1])
