"""Golden vectors of the sliding-window LZ77 coder, from the *imported reference* (data only).

Runs where the reference is checked out (as tools/gen_lz77_goldens.py, with the same ``bitarray`` stand-in):

    cd /tmp && PYTHONPATH=<reference checkout>:<repo> python -W ignore <repo>/tools/gen_lz77_sliding_goldens.py <repo>/tests/golden

Writes ``golden_lz77_sliding.npz`` (manifest + ``c{id}_{name}`` arrays, read by ``conftest.load_golden("lz77_sliding")``):
  kind "sliding": an ``LZ77SlidingWindowEncoder(HashBasedMatchFinder(hl, m, C, lazy, mml), W, init)`` fed ``n_blocks``
                  blocks; ``reset_before[b]`` = ``reset()`` was called in front of block b.  Per block b: ``b{b}_data``,
                  ``b{b}_seq`` ([k, 3]: literal_count, match_length, match_offset), ``b{b}_lit``, ``b{b}_out`` (packed bits
                  of ``encode_block``), meta ``nbits[b]`` and ``consumed[b][i]`` = ``num_bits_consumed`` of an
                  ``LZ77SlidingWindowDecoder`` in the matching state fed the bits + ``garbage{g}``, g = ``garbage_lens[i]``;
  kind "file"   : ``data`` through ``encode_file(block_size)`` of such an encoder: the ``encoded`` bytes.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

try:
    import bitarray  # noqa: F401
except ImportError:
    from stanford_compression_library_amd.utils import bitarray_utils as _own

    _mod, _util = types.ModuleType("bitarray"), types.ModuleType("bitarray.util")
    _mod.bitarray = _own.BitArray
    _util.ba2int = _own.bitarray_to_uint
    _util.int2ba = lambda x, length=None: _own.uint_to_bitarray(x, length)
    _util.urandom = _own.get_random_bitarray
    _mod.util = _util
    sys.modules["bitarray"], sys.modules["bitarray.util"] = _mod, _util

from scl.compressors.lz77_sliding_window import (HashBasedMatchFinder, LZ77SlidingWindowDecoder,  # noqa: E402
                                                 LZ77SlidingWindowEncoder)
from scl.utils.bitarray_utils import BitArray  # noqa: E402

GARBAGE_LENS = (0, 3, 61)
DEFAULTS = dict(hl=4, m=1000000, C=64, lazy=True, mml=4, W=1000000)


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


def packed(bits):
    return np.frombuffer(bits.tobytes(), np.uint8)


def make_encoder(p, init):
    finder = HashBasedMatchFinder(hash_length=p["hl"], hash_table_size=p["m"], max_chain_length=p["C"], lazy=p["lazy"],
                                  minimum_match_length=p["mml"])
    return LZ77SlidingWindowEncoder(finder, window_size=p["W"], initial_window=init)


def sliding_case(col, rng, group, init, blocks, reset_before=None, **overrides):
    p = dict(DEFAULTS, **overrides)
    reset_before = reset_before or [False] * len(blocks)
    enc = make_encoder(p, init)
    junk = {f"garbage{g}": rng.integers(0, 2, g).astype(np.uint8) for g in GARBAGE_LENS}
    arrays, nbits, consumed = dict(init=np.array(init or [], np.uint8), **junk), [], []
    first = None
    for b, (data, reset) in enumerate(zip(blocks, reset_before)):
        if reset:
            enc.reset()
        before = enc.window.get_window_as_list()
        seqs, lits = enc.lz77_parse_and_generate_sequences(list(data))
        bits = enc.streams_encoder.encode_block(seqs, lits)
        used_by = []
        for g in GARBAGE_LENS:
            dec = LZ77SlidingWindowDecoder(window_size=p["W"], initial_window=before)
            block, used = dec.decode_block(bits + BitArray("".join(map(str, junk[f"garbage{g}"].tolist()))))
            assert list(block.data_list) == list(data) and used == len(bits)
            used_by.append(int(used))
        arrays[f"b{b}_data"] = np.array(data, np.uint8)
        arrays[f"b{b}_seq"] = np.array([[s.literal_count, s.match_length, s.match_offset] for s in seqs],
                                       np.uint32).reshape(-1, 3)
        arrays[f"b{b}_lit"] = np.array(lits, np.uint8)
        arrays[f"b{b}_out"] = packed(bits)
        nbits.append(len(bits))
        consumed.append(used_by)
        first = first or (seqs[0] if seqs else None)
    col.add(dict(kind="sliding", group=group, hl=p["hl"], m=p["m"], C=p["C"], lazy=bool(p["lazy"]), mml=p["mml"], W=p["W"],
                 n_blocks=len(blocks), reset_before=[bool(r) for r in reset_before],
                 n=int(sum(len(b) for b in blocks)), nbits=nbits, consumed=consumed, garbage_lens=list(GARBAGE_LENS)),
            **arrays)
    return first


def main(out_dir):
    col = Collector()
    rng = np.random.default_rng(4077)

    three = rng.integers(0, 3, 640).tolist()
    for W in (16, 100, 100000):
        for m in (1, 3, 1000000):
            for C in (2, 64):
                for hl in (2, 4):
                    for lazy in ((True, False) if m == 1000000 else (True,)):
                        sliding_case(col, rng, "grid", three[:40], [three[40:]], W=W, m=m, C=C, hl=hl, lazy=lazy)

    words = [rng.integers(97, 101, int(rng.integers(2, 8))).tolist() for _ in range(12)]
    text = [c for k in rng.integers(0, 12, 300).tolist() for c in words[k]]
    sliding_case(col, rng, "word_text", None, [text[:700], text[700:]])
    sliding_case(col, rng, "word_text", None, [text[:700], text[700:]], lazy=False, hl=3, W=200)

    sliding_case(col, rng, "long_run", None, [[7] * 1000], W=16)
    for hl in (2, 4):
        for n in (0, 1, hl - 1, hl):
            sliding_case(col, rng, "short_block", None, [[9] * n], hl=hl)
            sliding_case(col, rng, "short_block_with_window", [9] * 8, [[9] * n], hl=hl)
    long_init = rng.integers(0, 4, 300).tolist()
    sliding_case(col, rng, "long_initial_window", long_init, [rng.integers(0, 4, 400).tolist()], W=64)
    blocks = [rng.integers(0, 3, 150).tolist() for _ in range(3)]
    sliding_case(col, rng, "blocks_then_reset", three[:10], blocks, [False, False, True], W=100)
    four = rng.integers(0, 4, 500).tolist()
    for hl, mml in ((4, 1), (3, 1), (2, 6), (8, 6)):
        sliding_case(col, rng, "mml", four[:20], [four[20:]], hl=hl, mml=mml)

    block = rng.integers(0, 200, 172).tolist()
    history = [b for j in range(80) for b in [250] + block[j: j + 4 + j] + [251]]
    first = sliding_case(col, rng, "ladder", history, [block])
    assert (first.literal_count, first.match_length) == (79, 83), first
    first = sliding_case(col, rng, "ladder", history, [block], lazy=False)
    assert (first.literal_count, first.match_length) == (0, 4), first

    init = [44, 45, 46] * 5
    data = rng.choice([44, 45, 46, 255], size=500, p=[0.5, 0.25, 0.2, 0.05]).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, back = (os.path.join(tmp, f) for f in ("in.bin", "out.bin", "back.bin"))
        data.tofile(src)
        make_encoder(dict(DEFAULTS, W=100), init).encode_file(src, dst, block_size=200)
        LZ77SlidingWindowDecoder(window_size=100, initial_window=init).decode_file(dst, back)
        assert np.array_equal(np.fromfile(back, np.uint8), data)
        encoded = np.fromfile(dst, np.uint8)
    col.add(dict(kind="file", group="encode_file", block_size=200, n=500, W=100), init=np.array(init, np.uint8), data=data,
            encoded=encoded)
    col.save(os.path.join(out_dir, "golden_lz77_sliding.npz"))


if __name__ == "__main__":
    main(sys.argv[1])
