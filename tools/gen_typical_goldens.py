"""Golden vectors of the typical-set coder, from the *imported reference* (data only).

Runs where the reference is checked out (as tools/gen_lz77_goldens.py, whose ``bitarray`` stand-in it shares):

    cd /tmp && PYTHONPATH=<reference checkout>:<repo> python -W ignore <repo>/tools/gen_typical_goldens.py <repo>/tests/golden

Run it with the interpreter and the numpy the package's tests run under, NOT with whatever interpreter the reference happens to
be installed for.  The reference takes -log2 p from numpy's log2, and numpy builds differ in its last bit: numpy 1.26.4 gives
-log2(0.3) = 0x3ffbca9c6f53897a, numpy 2.2.6 (and the C library) 0x3ffbca9c6f53897b.  The typical set follows: for {A: 0.6, B:
0.3, C: 0.1}, n = 10 the reference itself finds 161 / 2973 / 6184 typical tuples at eps = 0 / 0.1 / 0.2 under the former and
281 / 2989 / 6187 under the latter.  The fixtures record ``nlp`` and ``entropy`` as the run computed them, and every test but one
takes them from there; tests/test_typical_set_host.py also holds the package's ProbabilityDist against them bit for bit,
which only the same numpy can pass.  The committed file was written under Python 3.10.12, numpy 2.2.6.

Writes ``golden_typical_set.npz`` (manifest + ``c{id}_{name}`` arrays, read by ``conftest.load_golden``).  Every case is of kind
"typical": ``group`` names the distribution, ``K``, ``n``, ``eps`` the parameters; ``symbols`` is "str" (the symbols are "A",
"B", ... by position) or "int" (0..K-1).  Arrays: ``probs`` (float64, the ProbabilityDist's order), ``nlp`` (the reference's
``neg_log_probability`` per symbol) and ``entropy`` (its ``entropy``) as raw float64; ``bitmap`` = np.packbits of the flags
"tuple t is in index_typical" over t in itertools.product order; meta ``count``, ``bt`` (-1: the reference's None), ``bo`` =
the encoder's ``index_bitlen_*``; ``data`` = positions of the ``200 * n`` symbols of ``get_random_data_block(seed=0)``;
``out`` / ``nbits`` = ``encode_block``'s bits.  The decoder is run on the small cases only (it enumerates once more).
"""
import itertools
import os
import sys

import numpy as np

import gen_lz77_goldens as base  # registers the bitarray stand-in where the package is missing  # noqa: F401
from gen_lz77_goldens import Collector, packed

from scl.compressors.typical_set_coder import TypicalSetCoderParams, TypicalSetDecoder, TypicalSetEncoder  # noqa: E402
from scl.core.prob_dist import ProbabilityDist  # noqa: E402
from scl.utils.test_utils import get_random_data_block  # noqa: E402

REFERENCE_DISTS = [("abc631", {"A": 0.6, "B": 0.3, "C": 0.1}), ("ab64", {"A": 0.6, "B": 0.4}), ("ab99", {"A": 0.99, "B": 0.01}),
                   ("a1", {"A": 1})]
REFERENCE_EPS = (0.0, 0.01, 0.1, 0.2, 2.0)
REFERENCE_N = (1, 3, 6, 10)


def normalised(w):
    w = np.asarray(w, dtype=np.float64)
    return {i: float(x) for i, x in enumerate(w / w.sum())}


def cases():
    for name, d in REFERENCE_DISTS:
        for eps in REFERENCE_EPS:
            for n in REFERENCE_N:
                yield name, d, eps, n
    for n in REFERENCE_N:
        yield "dyadic", {"A": 0.5, "B": 0.25, "C": 0.25}, 0.0, n
    rng = np.random.default_rng(17)
    yield "k4", normalised([0.4, 0.3, 0.2, 0.1]), 0.1, 8
    yield "k2", normalised([0.7, 0.3]), 0.05, 16  # N = 2^16 exactly
    yield "k7", normalised(rng.random(7) + 0.05), 0.1, 5
    yield "k256", normalised(rng.random(256) + 0.01), 0.1, 2
    wide = normalised(rng.random(300) + 0.01)
    yield "k300", wide, 0.1, 1
    yield "k300", wide, 0.1, 2


def add(col, name, prob_dict, eps, n):
    dist = ProbabilityDist(prob_dict)
    symbols = list(prob_dict)
    position = {s: i for i, s in enumerate(symbols)}
    params = TypicalSetCoderParams(n, eps, dist)
    enc = TypicalSetEncoder(params)
    flags = np.fromiter((chunk in enc.index_typical for chunk in itertools.product(symbols, repeat=n)), dtype=bool,
                        count=len(symbols) ** n)
    assert int(flags.sum()) == len(enc.index_typical)
    data = get_random_data_block(dist, 200 * n, seed=0)
    bits = enc.encode_block(data)
    if len(symbols) ** n <= 4096:
        back, used = TypicalSetDecoder(params).decode_block(bits)
        assert back.data_list == data.data_list and used == len(bits)
    bt = enc.index_bitlen_typical
    col.add(dict(kind="typical", group=name, symbols="str" if isinstance(symbols[0], str) else "int", K=len(symbols), n=n,
                 eps=eps, count=int(flags.sum()), bt=-1 if bt is None else int(bt), bo=int(enc.index_bitlen_overall),
                 nbits=len(bits)),
            probs=np.array(list(prob_dict.values()), np.float64),
            nlp=np.array([dist.neg_log_probability(s) for s in symbols], np.float64),
            entropy=np.array([dist.entropy], np.float64), bitmap=np.packbits(flags),
            data=np.array([position[s] for s in data.data_list], np.uint16), out=packed(bits))


if __name__ == "__main__":
    col = Collector()
    for case in cases():
        add(col, *case)
    col.save(os.path.join(sys.argv[1], "golden_typical_set.npz"))
