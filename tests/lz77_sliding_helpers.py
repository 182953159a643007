"""Shared by the sliding-window LZ77 tests: the goldens and an independent restatement of the parse rule and of the
windowed replay, with the named wrong variants the goldens must tell apart.

The rule.  w[0..n) is the history followed by the block, the block starts at s; params = (hl, m, C, lazy, mml, W) =
(hash_length, hash_table_size, max_chain_length, lazy, minimum_match_length, window_size; W = 0: no bound).
bucket(p) = H(w[p..p+hl)) mod m with H = CPython's tuple hash.  The candidates of p at horizon T <= p are the C newest
q < T with bucket(q) == bucket(p); those with p - q > W are skipped but counted.  A candidate is extended right (longest l
with w[q+k] == w[p+k], p + l <= n), then left while p > E, q > max(0, E - W) and w[p-1] == w[q-1]; candidates are scored
newest first and a strictly longer one replaces the best.  From E (= s at first): with num = n - E - hl + 1 <= 0 the
sequence is (n - E, 0, 0); else the first i < num whose best(E+i) at T = E+i has at least mml bytes is taken, and if lazy
the positions E+j, j > i, are tried at the SAME horizon T = E+i while each is strictly longer; without such an i the
sequence is (num, 0, 0).
"""
import bisect
import functools

import numpy as np

from conftest import load_golden
from lz77_helpers import ST_CAPACITY, ST_STATE, ST_TRUNCATED, _common_prefix

MASK = (1 << 64) - 1
VARIANTS = ("horizon", "exact", "noleft", "tie", "lazyge")
DEFAULTS = (4, 1000000, 64, 1, 4, 1000000)  # (hl, m, C, lazy, mml, W)


def bucket(gram, m):
    """hash(tuple(gram)) % m of a 64-bit CPython, from the definition"""
    acc = 0x27D4EB2F165667C5
    for b in gram:
        acc = (acc + int(b) * 0xC2B2AE3D27D4EB4F) & MASK
        acc = ((acc << 31) | (acc >> 33)) & MASK
        acc = (acc * 0x9E3779B185EBCA87) & MASK
    acc = (acc + (len(gram) ^ (0x27D4EB2F165667C5 ^ 3527539))) & MASK
    if acc == MASK:
        acc = 1546275796
    if acc >= 1 << 63:
        acc -= 1 << 64
    return acc % m


@functools.lru_cache(maxsize=None)
def goldens():
    return load_golden("lz77_sliding")


def case_params(case):
    return (case.hl, case.m, case.C, int(case.lazy), case.mml, case.W)


def golden_blocks(case):
    """[(the coder's window before the block: its last W bytes, block data, sequences [k, 3], literals, packed bits, nbits,
    consumed per garbage length)] of a case, in order"""
    W = case.W
    window, out = case.arr("init")[-W:], []
    for b in range(case.n_blocks):
        if case.reset_before[b]:
            window = np.zeros(0, np.uint8)
        data = case.arr(f"b{b}_data")
        out.append((window, data, case.arr(f"b{b}_seq").astype(np.int64).reshape(-1, 3), case.arr(f"b{b}_lit"),
                    case.arr(f"b{b}_out"), case.nbits[b], case.consumed[b]))
        window = np.concatenate([window, data])[-W:]
    return out


def parse_restated(window, start, params, variant=None, walks=None):
    """-> (sequences as an int64 array [k, 3], literals as a uint8 array).  ``variant``: None = the rule, or one of VARIANTS,
    each a plausible misreading.  ``walks``: a list that receives the number of lazy steps taken per match."""
    assert variant is None or variant in VARIANTS
    hl, m, C, lazy, mml, W = params
    W = W if W else float("inf")
    w = bytes(np.asarray(window, np.uint8))
    n = len(w)
    if variant == "exact":
        key = [w[p:p + hl] for p in range(n - hl + 1)]
    else:
        key = [bucket(w[p:p + hl], m) for p in range(n - hl + 1)]
    chains = {}
    for p, k in enumerate(key):
        chains.setdefault(k, []).append(p)

    def best(p, T, E):
        """-> (literals, q, length) after both extensions; length 0: nothing"""
        chain = chains[key[p]]
        upto = bisect.bisect_left(chain, T)
        found = (0, 0, 0)
        for q in chain[max(0, upto - C):upto][::-1]:
            if p - q > W:
                continue
            length, pp = _common_prefix(w, q, p, n - p), p
            if variant != "noleft":
                first = max(0, E - W)
                while pp > E and q > first and w[pp - 1] == w[q - 1]:
                    pp, q, length = pp - 1, q - 1, length + 1
            if length > found[2] or (variant == "tie" and length == found[2]):
                found = (pp - E, q, length)
        return found

    seqs, lits, E = [], bytearray(), start
    while E < n:
        num = n - E - hl + 1
        if num <= 0:
            seq = (n - E, 0, 0)
        else:
            seq = (num, 0, 0)
            for i in range(num):
                found = best(E + i, E + i, E)
                if found[2] < mml:
                    continue
                steps = 0
                if lazy:
                    for j in range(i + 1, num):
                        other = best(E + j, E + j if variant == "horizon" else E + i, E)
                        if other[2] > found[2] or (variant == "lazyge" and other[2] == found[2]):
                            found, steps = other, steps + 1
                        else:
                            break
                if walks is not None:
                    walks.append(steps)
                seq = (found[0], found[2], E + found[0] - found[1])
                break
        seqs.append(seq)
        lits += w[E:E + seq[0]]
        E += seq[0] + seq[1]
    return np.array(seqs, np.int64).reshape(-1, 3), np.frombuffer(bytes(lits), np.uint8)


def replay_restated(history, seqs, literals, window_size=0, cap=None):
    """-> (new bytes: uint8 array, status).  As lz77_helpers.replay_restated, except that a sequence with match length 0
    copies nothing and its offset is not looked at, and that an offset above min(window_size, bytes so far) is ST_STATE
    (window_size 0: no bound)."""
    out = bytearray(bytes(np.asarray(history, np.uint8)))
    have, lit, at = len(out), bytes(np.asarray(literals, np.uint8)), 0
    cap = float("inf") if cap is None else cap

    def done(status):
        return np.frombuffer(bytes(out[have:]), np.uint8), status

    for run, length, off in np.asarray(seqs, np.int64).reshape(-1, 3).tolist():
        if run > len(lit) - at:
            return done(ST_TRUNCATED)
        if len(out) + run > cap:
            return done(ST_CAPACITY)
        out += lit[at:at + run]
        at += run
        if length == 0:
            continue
        if off == 0 or off > len(out) or (window_size and off > window_size):
            return done(ST_STATE)
        if len(out) + length > cap:
            return done(ST_CAPACITY)
        for _ in range(length):
            out.append(out[-off])
    if len(out) + len(lit) - at > cap:
        return done(ST_CAPACITY)
    out += lit[at:]
    return done(0)


@functools.lru_cache(maxsize=None)
def ragged_reference(params):
    """parse_restated of every stream of lz77_helpers.ragged_batch(): [(sequences, literals)]"""
    from lz77_helpers import ragged_batch

    b = ragged_batch()
    return [parse_restated(w, int(s), params) for w, s in zip(b["windows"], b["start"])]
