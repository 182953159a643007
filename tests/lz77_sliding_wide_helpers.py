"""Shared by the tests of the wide sliding-window LZ77 path: a pure-Python restatement of the scheme --
speculate / walk / emit, with the segment S and the cap CAP as arguments -- and the fixtures, each a few segments long and
sitting on an edge of the scheme.

The scheme.  f(E) = the sequence (literals, length, offset) the rule produces from E (lz77_sliding_helpers has the rule);
it depends on E and the window only, so the parse is the orbit of f from `start`.  speculate: per segment of S positions
the orbit from the segment's first block position is followed up to the first sequence start at or past the segment's end
(the segment's exit), every sequence stored in a table by its E as DONE; right extensions are capped at CAP bytes and the
search for a first match stops at the end of the next segment, and a sequence with a scored candidate at the cap or a
search at its bound is OPEN: nothing is stored and the orbit ends.  walk: from e = start; DONE: e = the segment's exit;
stored by the walk: followed; else f(e) in full, stored, followed.  emit: per segment the chain is followed from the
segment's entry; counts, exclusive scans over the segments, then every segment writes its rows and the literal bytes that
lie inside it: literal j has number j - start - (bytes matched before j).
"""
import bisect
import functools
from types import SimpleNamespace

import numpy as np

from lz77_helpers import _common_prefix
from lz77_sliding_helpers import DEFAULTS, buckets_restated, case_params, golden_blocks, goldens, parse_restated

DONE, OPEN, WALK = "done", "open", "walk"
NONLAZY = (4, 1000000, 64, 0, 4, 1000000)
SMALL = (2, 3, 2, 1, 2, 100)            # three buckets, two candidates, a window of 100 bytes
ONE_BUCKET = (1, 1, 64, 1, 1, 40)       # every position in one bucket, a window of 40 bytes
LONG_GRAM = (8, 65537, 3, 1, 6, 1000)   # mml below hl: the gram decides
PARAM_SETS = (DEFAULTS, NONLAZY, SMALL, ONE_BUCKET, LONG_GRAM)
PLANT = (4, (1 << 32) - 1, 64, 1, 4, 0)   # the planted cases: no window bound, (nearly) a bucket per gram
PLANT_C1 = (4, (1 << 32) - 1, 1, 1, 6, 0)  # one candidate and mml 6: a repeat of 4 bytes hides an older, longer one
PLANT_C2 = (4, (1 << 32) - 1, 2, 1, 6, 0)


class Rule:
    """f(E), with and without the speculation's cap and bound"""

    def __init__(self, window, params):
        self.hl, self.m, self.C, self.lazy, self.mml, W = params
        self.W = W if W else float("inf")
        self.w = bytes(np.asarray(window, np.uint8))
        self.n = len(self.w)
        self.key = buckets_restated(window, self.hl, self.m).tolist()
        self.chains = {}
        for p, k in enumerate(self.key):
            self.chains.setdefault(k, []).append(p)

    def best(self, p, T, E, cap):
        """-> ((literals, q, length), a scored candidate reached the cap)"""
        w, n, W = self.w, self.n, self.W
        chain = self.chains[self.key[p]]
        upto = bisect.bisect_left(chain, T)
        found, capped = (0, 0, 0), False
        room = n - p
        limit = room if cap is None or cap >= room else cap
        for q in chain[max(0, upto - self.C):upto][::-1]:
            if p - q > W:
                continue
            length, pp = _common_prefix(w, q, p, limit), p
            capped = capped or (limit < room and length >= limit)
            first = max(0, E - W)
            while pp > E and q > first and w[pp - 1] == w[q - 1]:
                pp, q, length = pp - 1, q - 1, length + 1
            if length > found[2]:
                found = (pp - E, q, length)
        return found, capped

    def sequence(self, E, cap=None, bound=None):
        """-> (literals, length, offset), or None for OPEN (only with a cap or a bound)"""
        n, hl = self.n, self.hl
        num = n - E - hl + 1
        if num <= 0:
            return (n - E, 0, 0)
        stop = E + num
        search_end = stop if bound is None or bound >= stop else bound
        for p in range(E, search_end):
            found, capped = self.best(p, p, E, cap)
            if capped:
                return None
            if found[2] < self.mml:
                continue
            if self.lazy:
                for pj in range(p + 1, stop):
                    other, capped = self.best(pj, p, E, cap)
                    if capped:
                        return None
                    if other[2] <= found[2]:
                        break
                    found = other
            return (found[0], found[2], E + found[0] - found[1])
        return None if search_end < stop else (num, 0, 0)


def scheme_restated(window, start, params, S, CAP):
    """-> (sequences int64 [k, 3], literals uint8, info): info.state[E] in (DONE, OPEN, WALK), info.table[E], info.exit[seg],
    info.entry[seg] (segments never entered are missing), info.computed = the positions the walk computed itself"""
    rule = Rule(window, params)
    w, n = rule.w, rule.n
    n_seg = -(-n // S)
    table, state, exits = {}, {}, []
    for seg in range(n_seg):
        seg_end, bound = min((seg + 1) * S, n), min((seg + 2) * S, n)
        e = max(seg * S, start)
        while e < seg_end:
            r = rule.sequence(e, CAP, bound)
            if r is None:
                state[e] = OPEN
                break
            table[e], state[e] = r, DONE
            e += r[0] + r[1]
        exits.append(e)
    entry, computed, e, in_seg = {}, [], start, None
    while e < n:
        seg = e // S
        if seg != in_seg:
            entry[seg], in_seg = e, seg
        if state.get(e) == DONE:
            nxt = exits[seg]
        elif state.get(e) == WALK:
            nxt = e + table[e][0] + table[e][1]
        else:
            computed.append(e)
            table[e], state[e] = rule.sequence(e), WALK
            nxt = e + table[e][0] + table[e][1]
        assert nxt > e
        e = nxt
    # emit: the counting pass, the scans, the writing pass
    cnt, msum, last = [0] * (n_seg + 1), [0] * (n_seg + 1), [0] * (n_seg + 1)
    for seg, e in entry.items():
        seg_end = min((seg + 1) * S, n)
        while e < seg_end:
            lits, length, _ = table[e]
            cnt[seg], msum[seg], last[seg] = cnt[seg] + 1, msum[seg] + length, e + 1
            e += lits + length
    cnt_x = np.concatenate([[0], np.cumsum(cnt)])[:-1].tolist()
    msum_x = np.concatenate([[0], np.cumsum(msum)])[:-1].tolist()
    last_x = np.concatenate([[0], np.maximum.accumulate(last)])[:-1].tolist()
    total = cnt_x[n_seg]
    rows = np.zeros((total, 3), np.int64)
    lit = np.full(n - start - msum_x[n_seg], -1, np.int64)
    for seg in range(n_seg):
        seg_end = min((seg + 1) * S, n)
        front, front_end = max(seg * S, start), entry.get(seg, seg_end)
        if front < front_end:  # the tail of the sequence that covers the segment's front
            E = last_x[seg] - 1
            before = msum_x[seg] - table[E][1]
            for j in range(front, min(E + table[E][0], front_end)):
                lit[j - start - before] = w[j]
        if seg in entry:
            e, k, before = entry[seg], cnt_x[seg], msum_x[seg]
            while e < seg_end:
                lits, length, off = table[e]
                rows[k] = (lits, length, off)
                for j in range(e, min(e + lits, seg_end)):
                    lit[j - start - before] = w[j]
                e, k, before = e + lits + length, k + 1, before + length
    assert (lit >= 0).all(), "a literal that no segment wrote"
    info = SimpleNamespace(state=state, table=table, exit=exits, entry=entry, computed=computed, n_seg=n_seg, cap=CAP)
    return rows, lit.astype(np.uint8), info


# ---- sources -----------------------------------------------------------------------------------------------------------------
def markov16(n, seed=1):
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 16, (16, 3))  # every symbol has three likely successors
    out, s = np.empty(n, np.uint8), 0
    pick, jump = rng.integers(0, 3, n), rng.random(n) < 0.08
    rnd = rng.integers(0, 16, n)
    for i in range(n):
        s = rnd[i] if jump[i] else table[s, pick[i]]
        out[i] = 97 + s
    return out


def word_text(n, seed=2):
    rng = np.random.default_rng(seed)
    words = [rng.integers(97, 123, int(k)).astype(np.uint8) for k in rng.integers(2, 9, 120)]
    parts, size = [], 0
    while size < n:
        parts += [words[int(rng.integers(0, 120))], np.array([32], np.uint8)]
        size += len(parts[-2]) + 1
    return np.concatenate(parts)[:n]


def random_bytes(n, symbols, seed=3):
    return np.random.default_rng(seed).integers(0, symbols, n).astype(np.uint8)


def no_repeat(n, seed=4):
    """random bytes over 256 symbols in which no gram of 4 bytes occurs twice"""
    w = random_bytes(n, 256, seed)
    rng = np.random.default_rng(seed + 100)
    while True:
        grams = np.lib.stride_tricks.sliding_window_view(w, 4)
        keys = grams[:, 0].astype(np.int64) << 24 | grams[:, 1].astype(np.int64) << 16 | grams[:, 2].astype(np.int64) << 8 | grams[:, 3]
        _, first, counts = np.unique(keys, return_index=True, return_counts=True)
        if (counts == 1).all():
            return w
        dup = np.setdiff1d(np.arange(len(keys)), first)
        w[dup] = rng.integers(0, 256, len(dup))


SOURCES = {"markov": markov16, "text": word_text, "random4": lambda n: random_bytes(n, 4), "equal": lambda n: np.full(n, 7, np.uint8),
           "period3": lambda n: np.resize(np.array([1, 2, 3], np.uint8), n), "period7": lambda n: np.resize(np.arange(7, dtype=np.uint8), n),
           "nomatch": no_repeat}


def _copy(w, dst, src, k):
    """w[dst : dst + k] becomes a repeat of w[src : src + k] that is exactly k bytes long on both sides"""
    w[dst: dst + k] = w[src: src + k]
    if dst + k < len(w) and w[dst + k] == w[src + k]:
        w[dst + k] ^= 0x55
    if src > 0 and w[dst - 1] == w[src - 1]:
        w[dst - 1] ^= 0x55


def _case(name, window, start, params, **expect):
    window = np.ascontiguousarray(window, np.uint8)
    window.setflags(write=False)
    return dict(name=name, window=window, start=int(start), params=tuple(params), expect=expect)


@functools.lru_cache(maxsize=None)
def all_cases(S, CAP):
    """every fixture at segment S and cap CAP: [dict(name, window, start, params, expect)].  expect names what
    check_edges() asserts of the restated scheme's parse."""
    n = 3 * S + 57
    cases = []
    for name, make in SOURCES.items():
        cases.append(_case(f"{name}-defaults", make(n), 0, DEFAULTS))
    for params, tag in zip(PARAM_SETS[1:], ("nonlazy", "small", "onebucket", "longgram")):
        for name in ("markov", "text"):
            cases.append(_case(f"{name}-{tag}", SOURCES[name](n), 0, params))
    cases.append(_case("random4-small", SOURCES["random4"](n), 0, SMALL))
    cases.append(_case("period7-onebucket", SOURCES["period7"](n), 0, ONE_BUCKET))
    # placement: where the block starts, how long it is
    for start in (1, S - 1, S, S + 1):
        cases.append(_case(f"markov-start{start}", markov16(n), start, DEFAULTS))
    cases.append(_case("markov-history-beyond-W", markov16(n), 700, SMALL))
    cases.append(_case("text-history-beyond-W", word_text(n + 1500), 1500, LONG_GRAM))
    for size, tag in ((0, "0"), (3, "hl-1"), (4, "hl"), (S - 1, "S-1"), (S, "S"), (S + 1, "S+1")):
        cases.append(_case(f"text-block{tag}", word_text(50 + size), 50, DEFAULTS))
    # planted matches in bytes without a repeat
    for k in (CAP - 1, CAP, CAP + 1):
        w = no_repeat(n)
        _copy(w, S + 100, 50, k)
        cases.append(_case(f"ext{k - CAP:+d}", w, 0, PLANT, first_seq=(S + 100, k, S + 50), open_at=0 if k >= CAP else None,
                           done_at=0 if k < CAP else None))
        cases.append(_loser_case(f"loser{k - CAP:+d}", n, S, k, CAP))
    w = no_repeat(n)
    _copy(w, n - 30, 200, 30)
    cases.append(_case("match-to-last-byte", w, 0, PLANT, last_seq=(None, 30, n - 230)))
    for d in (-1, 0, 1):
        w = no_repeat(n)
        _copy(w, 2 * S + d - 40, 300, 40)
        cases.append(_case(f"match-ends-segment{d:+d}", w, 0, PLANT, chain_has=2 * S + d))
    w = no_repeat(n)
    _copy(w, 2 * S - 50, 100, S + 49)   # ends at 3S - 1: the chain enters segment 2 at its last position
    cases.append(_case("enters-at-last-position", w, 0, PLANT, entry={2: 3 * S - 1}))
    w = no_repeat(5 * S + 57)
    _copy(w, 2 * S + 100, 20, 2 * S + 30)  # from segment 2 into segment 4: segment 3 is never entered
    cases.append(_case("segment-never-entered", w, 0, PLANT, not_entered=(3,), entry={4: 4 * S + 130}))
    cases.append(_left_case("left-to-E", n, S, to_E=True))
    cases.append(_left_case("left-to-window-start", n, S, to_E=False))
    ladder = [c for c in goldens() if c.kind == "sliding" and c.group == "ladder" and c.lazy][0]
    window, data = golden_blocks(ladder)[0][:2]
    cases.append(_case("ladder", np.concatenate([window, data]), len(window), case_params(ladder)))
    return tuple(cases)


def _hide(w, at, room):
    """makes the one candidate (C = 1) of position `at` a repeat of just its gram: the 4 bytes at `at` are copied to `room`,
    which lies in front of `at` and behind the older occurrence; the byte behind the copy differs"""
    w[room: room + 4] = w[at: at + 4]
    if w[room + 4] == w[at + 4]:
        w[room + 4] ^= 0x55


def _left_case(name, n, S, to_E):
    """A match found at p whose left extension covers p - 1 and p - 2, which were passed over because their one candidate
    (C = 1) is a repeat of 4 bytes, below mml = 6.  to_E: the extension ends at E, the end of the match in front, although
    the bytes go on being equal; else it ends at the first byte of the window (max(0, E - W) = 0) with E further back."""
    w = no_repeat(n)
    if to_E:
        _copy(w, S + 200, 40, 30)       # a match that ends at E = S + 230
        E, q = S + 230, 120              # p = E + 2; the source q with q - 3 .. q - 1 equal to the bytes in front of p
        p = E + 2
        w[p: p + 20] = w[q: q + 20]
        w[q - 3: q] = w[p - 3: p]        # equal back to p - 3 = E - 1, one byte past E
        w[p + 20] = w[q + 20] ^ 0x55
        _hide(w, p - 1, 150)
        _hide(w, p - 2, 170)
        return _case(name, w, 0, PLANT_C1, has_seq=(E, (0, 22, p - q)))
    p, q = S + 300, 2                    # the source starts two bytes into the window
    w[p - 2: p + 5] = w[0: 7]            # five bytes to the right, below mml: the left extension makes the match
    w[p + 5] = w[7] ^ 0x55
    _hide(w, p - 1, 150)
    _hide(w, p - 2, 170)
    return _case(name, w, 0, PLANT_C1, first_seq=(p - 2, 7, p - q))


def _loser_case(name, n, S, k, CAP):
    """Position p has two candidates (C = 2): the older one extends k bytes to the right and nothing to the left, the newer
    one CAP - 1 bytes to the right and two to the left, CAP + 1 in all, and wins for k <= CAP; for k = CAP + 1 the lengths
    tie and the newer one wins.  p - 1 and p - 2 were passed over: both their candidates are repeats of 4 bytes."""
    w = no_repeat(n)
    p, q1, q2 = S + 400, 100, 100 + CAP + 200
    w[q2: q2 + CAP - 1] = w[q1: q1 + CAP - 1]
    w[q2 + CAP - 1] = w[q1 + CAP - 1] ^ 0x55
    w[p - 2: p + CAP - 1] = w[q2 - 2: q2 + CAP - 1]     # equal to the newer one from p - 2 on
    w[p + CAP - 1: p + k] = w[q1 + CAP - 1: q1 + k]     # and to the older one up to k bytes
    w[p + k] = w[q1 + k] ^ 0x33
    if w[q1 - 1] == w[p - 1]:
        w[q1 - 1] ^= 0x55
    w[p - 3] = w[q2 - 3] ^ 0x55
    at = q2 + CAP + 100
    for pos in (p - 1, p - 2):
        for _ in range(2):
            _hide(w, pos, at)
            at += 20
    E = q2 + CAP - 1  # the newer candidate is itself a repeat of the older one: the sequence in front ends here
    return _case(name, w, 0, PLANT_C2, first_seq=(q2, CAP - 1, q2 - q1), has_seq=(E, (p - 2 - E, CAP + 1, p - q2)),
                 open_at=E if k >= CAP else None, done_at=E if k < CAP else None)


@functools.lru_cache(maxsize=None)
def reference(S, CAP):
    """parse_restated of every case of all_cases(S, CAP): {name: (sequences, literals)}, computed once"""
    return {c["name"]: parse_restated(c["window"], c["start"], c["params"]) for c in all_cases(S, CAP)}


def check_edges(case, seqs, info, S):
    """asserts that the case has the edge it is named for, in the rule's parse (seqs) and in the scheme's tables (info)"""
    ex, start = case["expect"], case["start"]
    starts = start + np.concatenate([[0], np.cumsum(seqs[:, 0] + seqs[:, 1])])
    if ex.get("first_seq"):
        assert tuple(seqs[0]) == ex["first_seq"], (case["name"], seqs[0])
    if ex.get("last_seq"):
        assert tuple(seqs[-1][1:]) == ex["last_seq"][1:] and starts[-1] == len(case["window"]), (case["name"], seqs[-1])
    if ex.get("has_seq"):
        E, seq = ex["has_seq"]
        at = np.flatnonzero(starts[:-1] == E)
        assert at.size == 1 and tuple(seqs[at[0]]) == seq, (case["name"], E, seqs[at[0]] if at.size else None)
    if ex.get("chain_has") is not None:
        assert ex["chain_has"] in starts, case["name"]
    if ex.get("open_at") is not None:
        assert info.state.get(ex["open_at"]) == WALK and ex["open_at"] in info.computed, case["name"]
        bound = min((ex["open_at"] // S + 2) * S, len(case["window"]))
        assert Rule(case["window"], case["params"]).sequence(ex["open_at"], info.cap, bound) is None
    if ex.get("done_at") is not None:
        assert info.state.get(ex["done_at"]) == DONE, case["name"]
    for seg, e in ex.get("entry", {}).items():
        assert info.entry.get(seg) == e, (case["name"], info.entry)
    for seg in ex.get("not_entered", ()):
        assert seg not in info.entry, (case["name"], info.entry)
