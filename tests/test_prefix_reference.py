"""CPU: the yardsticks of tests/test_gpu_prefix_limits.py (prefix_helpers.py), pinned before any kernel is compared with
them: decode_reference and encode_vectorised on the reference's Huffman goldens, decode_reference's statuses on cases whose
answer is written out here, and the table builders' geometry."""
from fractions import Fraction

import numpy as np
import pytest

from prefix_helpers import (DEEP_LONG_FIRST, ST_CAPACITY, ST_STATE, ST_TRUNCATED, bits_of_table, code_bits, comb,
                            count_deep_nodes, decode_reference, deep_chains, encode_numpy, encode_vectorised, goldens,
                            table_case)

BLOCKS = goldens()["block"]
BUILDERS = {"comb11": lambda: comb(11), "comb12": lambda: comb(12), "comb32": lambda: comb(32),
            "deep512": lambda: deep_chains(512), "deep513": lambda: deep_chains(513)}


def kraft(length):
    return sum(Fraction(1, 1 << int(n)) for n in length)


def is_prefix_free(code, length):
    words = sorted("".join(map(str, b)) for b in bits_of_table(code, length))
    return all(not b.startswith(a) for a, b in zip(words, words[1:]))  # a prefix sorts right in front of an extension


# ---- the goldens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BLOCKS, ids=repr)
def test_decode_reference_on_the_golden_blocks(case):
    table = table_case(case.group)
    sym, consumed, status = decode_reference(table.arr("code"), table.arr("len"), case.arr("out"), 0, case.nbits,
                                             len(case.arr("sym")))
    assert (consumed, status) == (case.nbits, 0)
    assert np.array_equal(sym, case.arr("sym"))


@pytest.mark.parametrize("case", BLOCKS, ids=repr)
def test_encode_vectorised_on_the_golden_blocks(case):
    table = table_case(case.group)
    packed, nbits = encode_vectorised(table.arr("code"), table.arr("len"), case.arr("sym"))
    assert nbits == case.nbits and np.array_equal(packed, case.arr("out"))
    mine, mine_bits = encode_numpy(code_bits(table), case.arr("sym"))
    assert mine_bits == nbits and np.array_equal(mine, packed)


@pytest.mark.parametrize("name", BUILDERS)
def test_encode_vectorised_on_the_builders_tables(name):
    code, length = BUILDERS[name]()
    sym = np.random.default_rng(len(code)).integers(0, len(code), 10_000)
    want, want_bits = encode_numpy(bits_of_table(code, length), sym)
    packed, nbits = encode_vectorised(code, length, sym)
    assert nbits == want_bits == int(length[sym].sum()) and np.array_equal(packed, want)
    back, consumed, status = decode_reference(code, length, packed, 0, nbits, len(sym))
    assert (consumed, status) == (nbits, 0) and np.array_equal(back, sym)
    assert encode_vectorised(code, length, sym[:0])[1] == 0


# ---- the builders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [11, 12, 32])
def test_comb_tables(L):
    code, length = comb(L)
    assert sorted(length.tolist()) == list(range(1, L + 1)) + [L]
    assert is_prefix_free(code, length) and kraft(length) == 1
    assert count_deep_nodes(code, length) == max(L - 11, 0)
    ones = {int(n): int(c) for c, n in zip(code, length) if c & 1}
    assert ones == {L: (1 << L) - 1}  # every other codeword ends in its zero
    assert sorted(code[length == L].tolist()) == [(1 << L) - 2, (1 << L) - 1]
    assert length.tolist() != sorted(length.tolist())  # the length does not grow with the index
    if L == 32:
        assert {0xFFFFFFFF, 0xFFFFFFFE} <= set(code.tolist())


@pytest.mark.parametrize("n_deep", [512, 513])
def test_deep_chains_tables(n_deep):
    code, length = deep_chains(n_deep)
    assert len(code) == 256 and int(length.max()) == 32 and int(length.min()) == 2
    assert is_prefix_free(code, length)
    assert count_deep_nodes(code, length) == n_deep
    long_lens = sorted(length[length > 11].tolist())
    assert long_lens == sorted([32] * 24 + [19] + ([12] if n_deep == 513 else []))
    assert sum(n - 11 for n in long_lens) == n_deep
    assert length[255] == 32
    prefixes = [int(c) >> (int(n) - 11) for c, n in zip(code, length) if n > 11]
    assert sorted(prefixes) == list(range(DEEP_LONG_FIRST, DEEP_LONG_FIRST + len(long_lens)))  # one each
    assert (code[length == 32] >= 1 << 31).all()  # the top bit of the 32-bit word is used
    n11 = int((length == 11).sum())
    assert n11 == 256 - 4 - len(long_lens)
    assert kraft(length) == Fraction(15, 32) + sum(Fraction(1, 1 << n) for n in long_lens) + Fraction(n11, 2048) < 1


def test_count_deep_nodes_on_a_tree_drawn_by_hand():
    # 13-bit "1111111111110" and 12-bit "000000000001": inner nodes at depth 11 (two of them) and 12 (one)
    assert count_deep_nodes([0b1111111111110, 0b000000000001], [13, 12]) == 3
    # max_len 3: the table is 3 bits wide and there is no node at depth 3
    assert count_deep_nodes([0b0, 0b10, 0b110, 0b111], [1, 2, 3, 3]) == 0


# ---- decode_reference's statuses, each answer derived here ----------------------------------------------------------------
def test_decode_reference_cut_inside_the_last_codeword():
    code, length = comb(32)
    rng = np.random.default_rng(1)
    sym = rng.integers(0, 33, 50)
    sym[-1] = int(np.nonzero(code == 0xFFFFFFFE)[0][0])
    packed, nbits = encode_vectorised(code, length, sym)
    start = nbits - 32
    for left in (1, 10, 11, 12, 31):  # bits of the last codeword that remain
        got, consumed, status = decode_reference(code, length, packed, 0, start + left, 50)
        assert (len(got), consumed, status) == (49, start, ST_TRUNCATED) and np.array_equal(got, sym[:49])
    # the same stream at a bit offset, between other bits
    bits = np.concatenate([np.ones(13, np.uint8), np.unpackbits(packed)[:nbits], np.ones(40, np.uint8)])
    got, consumed, status = decode_reference(code, length, np.packbits(bits), 13, start + 5, 50)
    assert (len(got), consumed, status) == (49, start, ST_TRUNCATED) and np.array_equal(got, sym[:49])


def test_decode_reference_missing_child():
    code, length = deep_chains(512)
    s32 = 255
    short = int(np.nonzero(length == 2)[0][0])
    head, head_bits = encode_vectorised(code, length, [short, s32, short])
    assert head_bits == 36
    good = np.unpackbits(head)[:36]
    # "01111": the four short codes leave that branch empty; the walk stops at its fifth bit
    bits = np.concatenate([good, [0, 1, 1, 1, 1, 0, 0, 0]]).astype(np.uint8)
    got, consumed, status = decode_reference(code, length, np.packbits(bits), 0, 44, 10)
    assert (got.tolist(), consumed, status) == ([short, s32, short], 36, ST_STATE)
    # ... and with only four of those bits in the stream it is a cut codeword, not a missing child
    got, consumed, status = decode_reference(code, length, np.packbits(bits), 0, 40, 10)
    assert (got.tolist(), consumed, status) == ([short, s32, short], 36, ST_TRUNCATED)
    # below the lookup table: symbol 255's chain has one child per node, so its last bit flipped leads nowhere
    bits = np.concatenate([good, good[2:34]]).astype(np.uint8)
    bits[-1] ^= 1
    got, consumed, status = decode_reference(code, length, np.packbits(bits), 0, 68, 10)
    assert (got.tolist(), consumed, status) == ([short, s32, short], 36, ST_STATE)
    bits[-1] ^= 1
    got, consumed, status = decode_reference(code, length, np.packbits(bits), 0, 68, 10)
    assert (got.tolist(), consumed, status) == ([short, s32, short, s32], 68, 0)


def test_decode_reference_capacity():
    table = table_case("random17")
    code, length = table.arr("code"), table.arr("len")
    sym = np.random.default_rng(2).integers(0, 17, 40)
    packed, nbits = encode_vectorised(code, length, sym)
    ends = np.cumsum(length[sym])
    for cap in (0, 1, 39):  # below the count: the bits of the first `cap` codewords, and bits are left
        got, consumed, status = decode_reference(code, length, packed, 0, nbits, cap)
        assert (consumed, status) == (int(ends[cap - 1]) if cap else 0, ST_CAPACITY) and np.array_equal(got, sym[:cap])
    got, consumed, status = decode_reference(code, length, packed, 0, nbits, 40)  # out_cap == n: no bit is left
    assert (consumed, status) == (nbits, 0) and np.array_equal(got, sym)
    more = np.concatenate([np.unpackbits(packed)[:nbits], [1]]).astype(np.uint8)  # out_cap == n, one bit left over
    got, consumed, status = decode_reference(code, length, np.packbits(more), 0, nbits + 1, 40)
    assert (consumed, status) == (nbits, ST_CAPACITY) and np.array_equal(got, sym)
    assert decode_reference(code, length, packed, 0, 0, 0)[1:] == (0, 0)  # an empty stream is complete
