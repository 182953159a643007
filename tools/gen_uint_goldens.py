"""Golden vectors of the three integer codes -- Golomb, universal, Elias-delta -- from the *imported reference* (data only).

Runs where the reference is checked out (as tools/gen_lz77_goldens.py, whose ``bitarray`` stand-in it shares):

    cd /tmp && PYTHONPATH=<reference checkout>:<repo> python -W ignore <repo>/tools/gen_uint_goldens.py <repo>/tests/golden

Writes ``golden_uint_codes.npz`` (manifest + ``c{id}_{name}`` arrays, read by ``conftest.load_golden("uint_codes")``).  Every
case: ``kind`` "golomb" (with ``M``) / "universal" / "elias_delta", ``group``, ``values`` (uint64), ``out`` = the packed bits
of the reference's ``encode_symbol`` of every value back to back, ``nbits``, ``lens`` = the length of every codeword, and
``device`` = every codeword fits 32 bits and every value 32 bits.  Groups, for Golomb M in 1, 2, 3, 4, 10, 64, 1000, the
universal and the Elias-delta code:
  reference   the data of the reference's own tests of the code (golomb_coder.py:148-184, universal_uint_coder.py:115-166,
              elias_delta_uint_coder.py:118-160), its expected bits asserted here
  range1000   list(range(1000))
  empty       the empty block
  boundaries  the smallest and the largest value of every codeword length up to 32 bits (Golomb: of every quotient's short
              and long remainders)
  past_limit  the one value behind the last of them: 33 bits and more, the host's path
  huge        2^32 + 5: no uint32

Golomb with M = 1 has b = 0, and the reference's ``uint_to_bitarray(r, bit_width=0)`` refuses a width of 0: its codeword is
the unary part alone, which this tool writes with the reference's own expression for that part (golomb_coder.py:81).
"""
import os
import sys

import numpy as np

import gen_lz77_goldens as base  # registers the bitarray stand-in where the package is missing  # noqa: F401
from gen_lz77_goldens import Collector, packed

from scl.compressors.elias_delta_uint_coder import EliasDeltaUintDecoder, EliasDeltaUintEncoder  # noqa: E402
from scl.compressors.golomb_coder import GolombCodeParams, GolombUintDecoder, GolombUintEncoder  # noqa: E402
from scl.compressors.universal_uint_coder import UniversalUintDecoder, UniversalUintEncoder  # noqa: E402
from scl.utils.bitarray_utils import BitArray  # noqa: E402

GOLOMB_MS = (1, 2, 3, 4, 10, 64, 1000)


class Unary:
    """Golomb M = 1"""

    def encode_symbol(self, x):
        return BitArray(x * "1" + "0")

    def decode_symbol(self, bits):
        used = 0
        while bits[used]:
            used += 1
        return used, used + 1


def coders(kind, M):
    if kind == "golomb":
        return (Unary(), Unary()) if M == 1 else (GolombUintEncoder(M), GolombUintDecoder(M))
    if kind == "universal":
        return UniversalUintEncoder(), UniversalUintDecoder()
    return EliasDeltaUintEncoder(), EliasDeltaUintDecoder()


def add_case(col, kind, M, group, values, expect=None):
    enc, dec = coders(kind, M)
    bits, lens = BitArray(""), []
    for v in values:
        word = enc.encode_symbol(int(v))
        assert dec.decode_symbol(word + BitArray("10")) == (int(v), len(word))
        bits += word
        lens.append(len(word))
    if expect is not None:
        assert bits == BitArray(expect), (kind, M, group)
    device = all(n <= 32 for n in lens) and all(int(v) < (1 << 32) for v in values)
    col.add(dict(kind=kind, M=M, group=group, n=len(values), nbits=len(bits), device=bool(device)),
            values=np.array(values, np.uint64), out=packed(bits), lens=np.array(lens, np.uint32))


def boundaries(kind, M):
    """(values at the ends of every codeword length up to 32 bits, the value behind the last of them)"""
    if kind == "universal":
        vals = sorted({v for L in range(1, 17) for v in ((1 << (L - 1)) if L > 1 else 0, (1 << L) - 1)})
        return vals, 1 << 16
    if kind == "elias_delta":
        vals = sorted({v for n in range(24) for v in ((1 << n) - 1, (1 << (n + 1)) - 2)})
        return vals, (1 << 24) - 1
    p = GolombCodeParams(M) if M > 1 else None
    b, cutoff = (p.b, p.cutoff) if p else (0, 1)
    vals = set()
    for q in range(32):
        for r in (0, cutoff - 1, cutoff, M - 1):
            long_form = M != cutoff and r >= cutoff
            if 0 <= r < M and q + 1 + b + long_form <= 32:
                vals.add(q * M + r)
    vals = sorted(vals)
    enc = coders(kind, M)[0]
    past = vals[-1] + 1  # the largest value of 32 bits and fewer is the last of its quotient's form
    while len(enc.encode_symbol(past)) <= 32:
        past += 1
    return vals, past


def main(out_dir):
    col = Collector()
    codes = [("golomb", M) for M in GOLOMB_MS] + [("universal", 0), ("elias_delta", 0)]
    reference = {
        ("golomb", 4): [([0, 1, 4, 102], "000" + "001" + "1000" + "1" * 25 + "0" + "10")],
        ("golomb", 10): [([2, 7, 26, 102], "0010" + "01101" + "1101100" + "11111111110010")],
        ("universal", 0): [([0, 0, 1, 3, 4, 100], None), ([0, 1, 3, 4, 100], "00" + "01" + "1011" + "110100" + "11111101100100")],
        ("elias_delta", 0): [([0, 0, 1, 3, 0, 0, 0, 2, 1, 4, 100], None),
                             ([0, 1, 3, 4, 5, 100], "1" + "0100" + "01100" + "01101" + "01110" + "00111100101")],
    }
    for kind, M in codes:
        for values, expect in reference.get((kind, M), []):
            add_case(col, kind, M, "reference", values, expect)
        add_case(col, kind, M, "range1000", list(range(1000)))
        add_case(col, kind, M, "empty", [])
        vals, past = boundaries(kind, M)
        add_case(col, kind, M, "boundaries", vals)
        add_case(col, kind, M, "past_limit", [3, past, 0])
        if kind != "golomb" or M == 1000:  # (a smaller M would write 2^32 / M ones)
            add_case(col, kind, M, "huge", [1, (1 << 32) + 5, 2])
    col.save(os.path.join(out_dir, "golden_uint_codes.npz"))


if __name__ == "__main__":
    main(sys.argv[1])
