"""Golden vectors of the prefix-free / Huffman coders, from the *imported reference* (data only).

Runs where the reference is checked out, with an interpreter that has the ``bitarray`` module (as oracle/gen_goldens.py):

    cd /tmp && PYTHONPATH=<reference checkout> python -W ignore <repo>/tools/gen_prefix_goldens.py <repo>/tests/golden

Writes ``golden_huffman.npz`` (manifest + ``c{id}_{name}`` arrays, read by ``conftest.load_golden("huffman")``):
  kind "table": a distribution (``probs``: exact float64, alphabet = 0..K-1 in this order; ``unvalidated``: made without
                ProbabilityDist's checks, which refuse what a code of more than 32 bits needs) and the reference's code table:
                ``order`` = the symbols in ``get_encoding_table()`` key order, ``code`` / ``len`` per symbol;
  kind "block": symbol indices coded with table ``table`` by ``HuffmanEncoder.encode_block``: packed bits, ``nbits``,
                and ``consumed`` = ``num_bits_consumed`` of ``HuffmanDecoder.decode_block``;
  kind "file" : a text, its character distribution and the bytes ``HuffmanEncoder.encode_file`` wrote for it.
"""
import json
import os
import sys
import tempfile

import numpy as np

from scl.compressors.huffman_coder import HuffmanDecoder, HuffmanEncoder, HuffmanTree
from scl.core.data_block import DataBlock
from scl.core.prob_dist import ProbabilityDist

BLOCK_LENS = (0, 1, 2, 1000)


class Collector:
    def __init__(self):
        self.cases, self.arrays = [], {}

    def add(self, meta, **arrays):
        meta = dict(meta, id=len(self.cases))
        self.cases.append(meta)
        for k, v in arrays.items():
            self.arrays[f"c{meta['id']}_{k}"] = np.asarray(v)
        return meta["id"]

    def save(self, path):
        np.savez_compressed(path, manifest=np.array(json.dumps(self.cases)), **self.arrays)
        print(f"{path}: {len(self.cases)} cases, {os.path.getsize(path)} bytes")


def normalised(w):
    w = np.asarray(w, dtype=np.float64)
    return w / w.sum()


def distributions():
    rng = np.random.default_rng(7)
    yield "dyadic2", np.array([0.5, 0.5])
    yield "dyadic3", np.array([0.5, 0.25, 0.25])
    yield "dyadic4", np.array([0.5, 0.25, 0.125, 0.125])
    yield "one_symbol", np.array([1.0])
    yield "k2", np.array([0.3, 0.7])
    for k in (3, 5, 256):
        yield f"uniform{k}", np.full(k, 1.0 / k)
    for k in (16, 200):
        yield f"ties{k}", normalised(rng.integers(1, 5, k))
    for k in (17, 256):
        yield f"random{k}", normalised(rng.random(k) + 1e-3)
    yield "random300", normalised(rng.random(300) + 1e-3)
    # ProbabilityDist refuses p < 1e-6, and no Huffman code of such a distribution is longer than 28 bits; Fibonacci weights
    # give the deepest tree: 28 symbols, longest code 27 bits, smallest probability 1.2e-6
    fib = [1, 1]
    while len(fib) < 28:
        fib.append(fib[-1] + fib[-2])
    yield "skewed28", normalised(fib)
    # a code longer than 32 bits needs a distribution ProbabilityDist would refuse: the object is made without its
    # validation (HuffmanTree reads .alphabet and .probability only)
    yield "skewed40", normalised(2.0 ** -np.arange(1, 41))


def make_dist(probs):
    prob_dict = {i: float(p) for i, p in enumerate(probs)}
    if min(prob_dict.values()) >= 1e-6:
        return ProbabilityDist(prob_dict), False
    dist = ProbabilityDist.__new__(ProbabilityDist)
    dist.prob_dict = prob_dict
    return dist, True


def main(out_dir):
    col = Collector()
    rng = np.random.default_rng(11)
    for name, probs in distributions():
        dist, unvalidated = make_dist(probs)
        table = HuffmanTree(dist).get_encoding_table()
        k = len(probs)
        code, length = np.zeros(k, np.uint64), np.zeros(k, np.uint8)
        for s, bits in table.items():
            code[s], length[s] = int(bits.to01(), 2), len(bits)
        tid = col.add(dict(kind="table", group=name, K=k, max_len=int(length.max()), unvalidated=unvalidated), probs=probs,
                      order=np.array(list(table), np.uint32), code=code, len=length)
        if length.max() > 32:
            continue
        enc, dec = HuffmanEncoder(dist), HuffmanDecoder(dist)
        for n in BLOCK_LENS:
            sym = rng.choice(k, size=n, p=probs)
            bits = enc.encode_block(DataBlock(sym.tolist()))
            block, used = dec.decode_block(bits)
            assert block.data_list == sym.tolist() and used == len(bits)
            col.add(dict(kind="block", group=name, table=tid, n=n, nbits=len(bits), consumed=int(used)),
                    sym=sym.astype(np.uint16), out=np.frombuffer(bits.tobytes(), np.uint8))
    # the reference's block loop and framing: a text of two blocks through encode_file
    chars = "abcdefgh \n"
    probs = normalised([8, 1, 3, 4, 13, 2, 2, 6, 7, 1])
    text = "".join(rng.choice(list(chars), size=1200, p=probs))
    dist = ProbabilityDist({c: float(p) for c, p in zip(chars, probs)})
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.bin")
        with open(src, "w", newline="") as f:
            f.write(text)
        HuffmanEncoder(dist).encode_file(src, dst, block_size=700)
        encoded = np.fromfile(dst, np.uint8)
        back = os.path.join(tmp, "back.txt")
        HuffmanDecoder(dist).decode_file(dst, back)
        assert open(back, newline="").read() == text
    col.add(dict(kind="file", group="encode_file", block_size=700, chars=chars), probs=probs,
            text=np.frombuffer(text.encode("ascii"), np.uint8), encoded=encoded)
    col.save(os.path.join(out_dir, "golden_huffman.npz"))


if __name__ == "__main__":
    main(sys.argv[1])
