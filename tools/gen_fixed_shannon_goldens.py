"""Golden vectors of the fixed-width coder and of the Shannon, Fano and Shannon-Fano-Elias codes, from the *imported
reference* (data only).

Runs where the reference is checked out (as tools/gen_lz77_goldens.py, whose ``bitarray`` stand-in it shares):

    cd /tmp && PYTHONPATH=<reference checkout>:<repo> python -W ignore <repo>/tools/gen_fixed_shannon_goldens.py <repo>/tests/golden

Writes two files (manifest + ``c{id}_{name}`` arrays, read by ``conftest.load_golden``):

``golden_fixed_bitwidth.npz``
  kind "block": ``coder`` "pickle" (FixedBitwidthEncoder) or "text" (TextFixedBitwidthEncoder); ``data`` = the block (int64
                symbols, or code points of one-character str symbols when ``symbols`` is "str"); ``order`` = the alphabet in
                header order, ``list(data_block.get_alphabet())`` as this run got it -- set order: fixed for small
                non-negative ints, a matter of the hash seed for str; ``out`` / ``nbits`` = ``encode_block``'s bits;
                ``head_bits`` = the bits of the alphabet in front of the 32-bit size (a pickle: the interpreter's);
                ``garbage_lens`` / ``garbage{g}`` / ``consumed`` = ``num_bits_consumed`` with g random bits behind the block.
                ``raises``: the block is refused with this exception (the empty block: no alphabet, no width).
  kind "file" : ``text`` (bytes), ``block_size`` and the bytes ``TextFixedBitwidthEncoder.encode_file`` wrote.

``golden_shannon_family.npz``
  kind "table": ``coder`` "shannon" / "fano" / "sfe", the distribution (``symbols``: int64, or code points for str symbols;
                ``probs``: exact float64, in the ProbabilityDist's order) and the reference's code: ``order`` = positions in
                ``symbols`` in the table's key order, ``code`` / ``len`` per entry of ``order``.  ``raises``: the reference
                refuses the distribution with this exception (no table).
  kind "block": ``table`` = id of its table; ``data`` = positions in ``symbols`` of the 2000 symbols of
                ``get_random_data_block(seed=0)``; ``out`` / ``nbits`` / ``consumed`` from ``encode_block`` / ``decode_block``.
"""
import os
import sys
import tempfile

import numpy as np

import gen_lz77_goldens as base  # registers the bitarray stand-in where the package is missing  # noqa: F401
from gen_lz77_goldens import Collector, packed

from scl.compressors.fano_coder import FanoDecoder, FanoEncoder  # noqa: E402
from scl.compressors.fixed_bitwidth_compressor import (FixedBitwidthDecoder, FixedBitwidthEncoder,  # noqa: E402
                                                       TextFixedBitwidthDecoder, TextFixedBitwidthEncoder)
from scl.compressors.shannon_coder import ShannonDecoder, ShannonEncoder  # noqa: E402
from scl.compressors.shannon_fano_elias_coder import ShannonFanoEliasDecoder, ShannonFanoEliasEncoder  # noqa: E402
from scl.core.data_block import DataBlock  # noqa: E402
from scl.core.prob_dist import ProbabilityDist  # noqa: E402
from scl.utils.bitarray_utils import BitArray  # noqa: E402
from scl.utils.test_utils import get_random_data_block  # noqa: E402

GARBAGE_LENS = (0, 5, 64)
SMALL_K = (1, 2, 3, 4, 5, 16, 17)
BIG_K = (255, 256, 257, 1000, 65536)
BLOCK_SIZES = (0, 1, 7, 100)


def bits_of(a):
    return BitArray("".join(map(str, np.asarray(a).tolist())))


# ---- fixed width -----------------------------------------------------------------------------------------------------------
def add_fixed(col, coder, group, data, symbols, rng):
    enc, dec = ((FixedBitwidthEncoder(), FixedBitwidthDecoder()) if coder == "pickle" else
                (TextFixedBitwidthEncoder(), TextFixedBitwidthDecoder()))
    block = DataBlock(list(data))
    as_int = (lambda s: ord(s)) if symbols == "str" else int
    meta = dict(kind="block", coder=coder, group=group, symbols=symbols, n=len(data))
    values = np.array([as_int(s) for s in data], np.int64)
    try:
        bits = enc.encode_block(block)
    except OverflowError as e:
        col.add(dict(meta, raises=type(e).__name__), data=values)
        return
    order = list(block.get_alphabet())
    head_bits = len(enc.alphabet_encoder.encode_block(order))
    assert bits[:head_bits] == enc.alphabet_encoder.encode_block(order)
    junk = {f"garbage{g}": rng.integers(0, 2, g).astype(np.uint8) for g in GARBAGE_LENS}
    consumed = []
    for g in GARBAGE_LENS:
        back, used = dec.decode_block(bits + bits_of(junk[f"garbage{g}"]))
        assert back.data_list == list(data) and used == len(bits)
        consumed.append(used)
    col.add(dict(meta, nbits=len(bits), head_bits=head_bits, garbage_lens=list(GARBAGE_LENS), consumed=consumed),
            data=values, order=np.array([as_int(s) for s in order], np.int64), out=packed(bits), **junk)


def fixed_cases(col):
    rng = np.random.default_rng(11)
    for K in SMALL_K:
        for n in BLOCK_SIZES:
            data = rng.integers(0, K, n)
            if n >= K:
                data[:K] = rng.permutation(K)  # every symbol is there: the alphabet has K symbols
            add_fixed(col, "pickle", f"k{K}", data.tolist(), "int", rng)
    for K in BIG_K:
        data = np.concatenate([rng.permutation(K), rng.integers(0, K, 37)])
        add_fixed(col, "pickle", f"k{K}", data.tolist(), "int", rng)
    # the reference's own test vectors (fixed_bitwidth_compressor.py:184-215)
    add_fixed(col, "text", "reference", ["A", "B", "C", "C", "A", "C", "D"], "str", rng)
    add_fixed(col, "pickle", "reference", ["A", "B", "C", "C", "A", "C", "D"], "str", rng)
    uniform4 = ProbabilityDist({"A": 0.25, "B": 0.25, "C": 0.25, "D": 0.25})
    add_fixed(col, "pickle", "reference100k", get_random_data_block(uniform4, 100000, seed=0).data_list, "str", rng)
    # a 2000-byte file through encode_file (:218-241, seeded here)
    text = "".join(get_random_data_block(ProbabilityDist({"A": 0.5, "B": 0.25, "C": 0.25}), 2000, seed=3).data_list)
    with tempfile.TemporaryDirectory() as tmp:
        src, coded, back = (os.path.join(tmp, f) for f in ("in.txt", "coded.bin", "back.txt"))
        with open(src, "w") as f:
            f.write(text)
        TextFixedBitwidthEncoder().encode_file(src, coded, block_size=1000)
        TextFixedBitwidthDecoder().decode_file(coded, back)
        assert open(back).read() == text
        col.add(dict(kind="file", coder="text", group="file2000", block_size=1000, n=len(text)),
                text=np.frombuffer(text.encode("ascii"), np.uint8), file=np.frombuffer(open(coded, "rb").read(), np.uint8))


# ---- Shannon, Fano, Shannon-Fano-Elias ---------------------------------------------------------------------------------------
CODERS = {"shannon": (ShannonEncoder, ShannonDecoder), "fano": (FanoEncoder, FanoDecoder),
          "sfe": (ShannonFanoEliasEncoder, ShannonFanoEliasDecoder)}
# the reference's own expectations (shannon_coder.py:96-107, fano_coder.py:134-145)
REFERENCE_DISTS = [{"A": 0.5, "B": 0.5}, {"A": 0.3, "B": 0.3, "C": 0.4}, {"A": 0.5, "B": 0.25, "C": 0.12, "D": 0.13},
                   {"A": 0.9, "B": 0.1}]
EXPECTED = {
    "shannon": [{"A": "0", "B": "1"}, {"A": "01", "B": "10", "C": "00"}, {"A": "0", "B": "10", "C": "1110", "D": "110"},
                {"A": "0", "B": "1110"}],
    "fano": [{"A": "0", "B": "1"}, {"A": "10", "B": "11", "C": "0"}, {"A": "0", "B": "10", "C": "111", "D": "110"},
             {"A": "0", "B": "1"}],
}


def normalised(w):
    w = np.asarray(w, dtype=np.float64)
    return w / w.sum()


def distributions():
    rng = np.random.default_rng(5)
    for i, d in enumerate(REFERENCE_DISTS):
        yield f"reference{i}", d
    as_dict = lambda p: {i: float(x) for i, x in enumerate(p)}  # noqa: E731
    yield "dyadic4", as_dict([0.5, 0.25, 0.125, 0.125])
    yield "dyadic_ladder", as_dict([2.0 ** -(i + 1) for i in range(15)] + [2.0 ** -15])
    yield "uniform64", as_dict(np.full(64, 1 / 64))
    yield "unsorted5", as_dict([0.1, 0.35, 0.05, 0.3, 0.2])
    for k in (17, 64):
        yield f"random{k}", as_dict(normalised(rng.random(k) + 0.01))
    yield "ties16", as_dict(normalised(rng.integers(1, 4, 16)))
    yield "ties_uniform5", as_dict(np.full(5, 0.2))
    yield "twenty_bits", as_dict([0.7, 0.3 - 1.2e-6, 1.2e-6])  # -log2(1.2e-6) = 19.67: a 20-bit Shannon codeword


def shannon_cases(col):
    for name, prob_dict in distributions():
        dist = ProbabilityDist(prob_dict)
        symbols = list(prob_dict)
        is_str = isinstance(symbols[0], str)
        sym_arr = np.array([ord(s) if is_str else s for s in symbols], np.int64)
        data = get_random_data_block(dist, 2000, seed=0)
        positions = {s: i for i, s in enumerate(symbols)}
        for coder, (Enc, Dec) in CODERS.items():
            meta = dict(kind="table", coder=coder, group=name, symbols="str" if is_str else "int", n=len(symbols))
            try:
                enc, dec = Enc(dist), Dec(dist)
                table = {s: enc.encode_symbol(s) for s in (symbols if coder == "sfe" else enc.encoding_table)}
            except Exception as e:
                col.add(dict(meta, raises=type(e).__name__), symbols=sym_arr, probs=np.array(list(prob_dict.values())))
                continue
            if name.startswith("reference") and coder in EXPECTED:
                want = EXPECTED[coder][int(name[-1])]
                assert {s: c.to01() for s, c in table.items()} == want, (coder, name)
            tid = col.add(meta, symbols=sym_arr, probs=np.array(list(prob_dict.values()), np.float64),
                          order=np.array([positions[s] for s in table], np.int64),
                          code=np.array([int(c.to01(), 2) for c in table.values()], np.uint64),
                          len=np.array([len(c) for c in table.values()], np.int64))
            bits = enc.encode_block(data)
            back, used = dec.decode_block(bits)
            assert back.data_list == data.data_list and used == len(bits)
            col.add(dict(kind="block", coder=coder, group=name, table=tid, n=data.size, nbits=len(bits), consumed=used),
                    data=np.array([positions[s] for s in data.data_list], np.int64), out=packed(bits))


if __name__ == "__main__":
    out_dir = sys.argv[1]
    col = Collector()
    fixed_cases(col)
    col.save(os.path.join(out_dir, "golden_fixed_bitwidth.npz"))
    col = Collector()
    shannon_cases(col)
    col.save(os.path.join(out_dir, "golden_shannon_family.npz"))
