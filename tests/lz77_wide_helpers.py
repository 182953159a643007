"""Shared by the tests of the wide LZ77 path (csrc/scl_lz77_wide.hip): the streams they parse and replay, each with the edge
it is there for, and a pure-Python restatement of the scheme -- scores capped at C, tile exits, the walk, the per-tile emit
behind scans, and the replay by prefix sums, validation and pointer doubling.  The restatement documents the algorithm and
guards the fixtures: tests/test_lz77_wide_host.py holds it against lz77_helpers.parse_restated / replay_restated.

Every builder takes the kernels' shape (T = positions per tile, C = the cap of a scored extension) as arguments, so the
edges move with the constants.
"""
import bisect
import functools

import numpy as np

from lz77_helpers import ST_CAPACITY, ST_STATE, ST_TRUNCATED, _common_prefix, markov1_stream, parse_restated

LONG, NONE = -1, -1
LM = ((6, 64), (1, 1), (8, 3), (4, 64), (6, 63))


# ---- the streams -----------------------------------------------------------------------------------------------------------
def _case(name, window, start=0, L=6, M=64, expect=()):
    """expect: [(position, match length)] that the parse must contain -- what the case is there for"""
    return dict(name=name, window=np.ascontiguousarray(window, np.uint8), start=int(start), L=L, M=M, expect=list(expect))


def _noise(rng, n):
    """bytes without repeats worth a match: 256 symbols, a few thousand bytes, grams of 6"""
    return rng.integers(0, 256, n).astype(np.uint8)


def _differs(b):
    return np.uint8((int(b) + 1) & 255)


def _planted(rng, m, p2, tail=40):
    """X (m bytes) at 0, noise up to p2, X again at p2, then a byte that ends the match, then noise: the parse has the
    sequence (p2, m) -- position p2, match length m, offset p2"""
    assert p2 > m + 1
    x = _noise(rng, m)
    w = np.concatenate([x, _noise(rng, p2 - m), x, _noise(rng, tail)])
    w[p2 + m] = _differs(w[m])
    return w


def source_cases(T, C):
    """five sources x five (L, M), block = the whole window of 3 tiles and a bit"""
    n = 3 * T + 37
    rng = np.random.default_rng(41)
    sources = (("markov", markov1_stream(n, 3)), ("equal", np.full(n, 7, np.uint8)),
               ("period3", np.resize(np.array([5, 1, 9], np.uint8), n)),
               ("period7", np.resize(np.arange(7, dtype=np.uint8), n)), ("rand4", rng.integers(0, 4, n).astype(np.uint8)))
    return [_case(f"{name}-L{L}-M{M}", w, 0, L, M) for name, w in sources for L, M in LM]


def start_cases(T, C):
    w = markov1_stream(5 * T, 8)
    out = [_case(f"start{s}", w[: 3 * T + 11], s) for s in (0, 1, T - 1, T, T + 1)]
    out.append(_case("history-longer-than-block", w, 3 * T + 5))
    return out


def length_cases(T, C, L=6):
    """blocks of 0, L - 1, L, T - 1, T, T + 1 bytes behind a history of T + 3 bytes they repeat"""
    hist = markov1_stream(T + 3, 9)
    block = np.resize(hist[5:], T + 1)
    return [_case(f"block{k}", np.concatenate([hist, block[:k]]), len(hist), L) for k in (0, L - 1, L, T - 1, T, T + 1)]


def cap_cases(T, C):
    rng = np.random.default_rng(42)
    out = []
    for m in (C - 1, C, C + 1):
        p2 = m + T + 13
        out.append(_case(f"match{m}", _planted(rng, m, p2), expect=[(p2, m)]))
        # the same match as the OLDER of two candidates: the newer one stops after 20 bytes
        x = _noise(rng, m)
        w = np.concatenate([x, _noise(rng, 30), x[:20], _noise(rng, 30), x, _noise(rng, 40)])
        w[m + 30 + 20] = _differs(x[20])
        p3 = m + 30 + 20 + 30
        w[p3 + m] = _differs(w[m])
        out.append(_case(f"older{m}", w, expect=[(m + 30, 20), (p3, m)]))
    x = _noise(rng, 2 * C)
    out.append(_case("long-to-the-last-byte", np.concatenate([x, _noise(rng, 50), x]), expect=[(2 * C + 50, 2 * C)]))
    x = _noise(rng, C + 50)
    out.append(_case("short-of-the-cap-at-the-window-end", np.concatenate([x, _noise(rng, 50), x[: C - 10]]),
                     expect=[(C + 100, C - 10)]))
    return out


def tile_cases(T, C):
    rng = np.random.default_rng(43)
    out = []
    for d in (-1, 0, 1):  # a match that ends at tile_end - 1, tile_end, tile_end + 1
        p2 = 2 * T - 40 + d
        out.append(_case(f"ends-at-tile-end{d:+d}", _planted(rng, 40, p2, tail=T), expect=[(p2, 40)]))
    p2, m = 2 * T - 5, T + 4  # ... at the last position of the tile after the next
    out.append(_case("enters-at-a-last-position", _planted(rng, m, p2, tail=T), expect=[(p2, m)]))
    m = 2 * T + 2 * C + 100  # tiles covered whole by one match: never entered
    p2 = m + 33
    out.append(_case("tiles-without-entry", _planted(rng, m, p2, tail=T + 5), expect=[(p2, m)]))
    p2 = 4 * T + 17  # literals from 40 to p2: the run in front of the second sequence spans three whole tiles
    out.append(_case("literal-run-over-three-tiles", _planted(rng, 40, p2, tail=60), expect=[(p2, 40)]))
    # a tile whose entry is a LONG position: X Y ... X Y, the match of X ends where Y's begins, in the next tile
    x, y = _noise(rng, 40), _noise(rng, C + 30)
    p2 = 2 * T - 20
    w = np.concatenate([x, _noise(rng, 1), y, _noise(rng, p2 - 41 - len(y)), x, y, _noise(rng, 50)])
    w[40] = _differs(y[0])
    w[p2 + 40 + len(y)] = _differs(w[41 + len(y)])
    out.append(_case("entry-is-long", w, expect=[(p2, 40), (p2 + 40, len(y))]))
    return out


@functools.lru_cache(maxsize=None)
def all_cases(T, C):
    return tuple(source_cases(T, C) + start_cases(T, C) + length_cases(T, C) + cap_cases(T, C) + tile_cases(T, C))


@functools.lru_cache(maxsize=None)
def reference(T, C):
    """name -> parse_restated of the case: (sequences [k, 3], literals), computed once"""
    return {c["name"]: parse_restated(c["window"], c["start"], c["L"], c["M"]) for c in all_cases(T, C)}


def sequence_positions(seqs, start):
    """[(position, match length)] of a parse"""
    out, pos = [], start
    for run, length, _ in np.asarray(seqs, np.int64).reshape(-1, 3).tolist():
        out.append((pos + run, length))
        pos += run + length
    return out


def damage_cases(seqs, literals, have):
    """Sequences of a good parse with ONE fault each -> [(name, sequences, cap or None)]: offset 0, offset one past the
    bytes so far, literal count one more than the literals left -- in the first, a middle and the last sequence -- and a
    slot one byte too small at a literal run, at a match (first, middle, last) and at the literals left over."""
    seqs = np.asarray(seqs, np.int64).reshape(-1, 3)
    k_all, n_lit = len(seqs), len(literals)
    d = have + np.concatenate([[0], np.cumsum(seqs[:, 0] + seqs[:, 1])])
    lp = np.concatenate([[0], np.cumsum(seqs[:, 0])])
    assert k_all >= 3 and n_lit > lp[-1], "needs sequences and literals left over"
    out = []
    for where, k in (("first", 0), ("middle", k_all // 2), ("last", k_all - 1)):
        for name, col, value in (("offset0", 2, 0), ("offset-past", 2, d[k] + seqs[k, 0] + 1),
                                 ("literals-short", 0, n_lit - lp[k] + 1)):
            bad = seqs.copy()
            bad[k, col] = value
            out.append((f"{name}-{where}", bad, None))
        with_run = next(j for j in list(range(k, k_all)) + list(range(k)) if seqs[j, 0] >= 1)
        out.append((f"slot-short-at-literals-{where}", seqs, int(d[with_run] + seqs[with_run, 0] - 1)))
        out.append((f"slot-short-at-match-{where}", seqs, int(d[k + 1] - 1)))
    out.append(("slot-short-at-leftover", seqs, int(d[-1] + n_lit - lp[-1] - 1)))
    return out


# ---- the scheme, restated ----------------------------------------------------------------------------------------------------
def parse_wide_restated(window, start, L, M, T, C, seq_cap=None):
    """The wide parse step by step -> (sequences [n_seq, 3], literals [n_lit], status, info); info: steps of the walk,
    LONG positions it resolved, tiles never entered."""
    assert 1 <= M <= 64 and T <= C
    w = bytes(np.asarray(window, np.uint8))
    n = len(w)
    where = {}
    for q in range(n - L + 1):
        where.setdefault(w[q:q + L], []).append(q)

    def score(p, limit):
        """(longest length, its q) among the newest M candidates q <= p - L, newest on ties; extensions stop at limit"""
        occ = where[w[p:p + L]]
        cand = occ[:bisect.bisect_right(occ, p - L)][::-1][:M]
        best = (0, 0)
        for q in cand:
            length = _common_prefix(w, q, p, limit)
            if length > best[0]:
                best = (length, q)
        return best

    # score: every position of the block that has a candidate; at the cap the position is LONG and nothing else is kept
    slen, sq = [0] * n, [0] * n
    for p in range(start, n - L + 1):
        length, q = score(p, min(C, n - p))
        slen[p], sq[p] = (LONG, 0) if length >= C else (length, q)
    if seq_cap is None:
        seq_cap = max((n - start) // L, 1)
    if start == n:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.uint8), 0, dict(steps=0, resolved=[], skipped=0)
    n_tiles = (n + T - 1) // T
    # tile exits, by a backward sweep: the first chain position >= tile end, or the LONG position the chain stops at
    exit_ = [0] * n
    for tile in range(n_tiles):
        for p in range(min((tile + 1) * T, n) - 1, max(tile * T, start) - 1, -1):
            if slen[p] == LONG:
                exit_[p] = p
            else:
                to = p + max(slen[p], 1)
                exit_[p] = to if to >= (tile + 1) * T or to >= n else exit_[to]
    # the walk
    entry, e, steps, resolved = [NONE] * n_tiles, start, 0, []
    while e < n:
        tile = e // T
        assert entry[tile] == NONE, "a tile is entered once"
        entry[tile], x, steps = e, exit_[e], steps + 1
        if x < n and x // T == tile:
            slen[x], sq[x] = score(x, n - x)
            assert slen[x] >= C >= T
            resolved.append(x)
            e = x + slen[x]
        else:
            assert x > e
            e = x
    # emit: count per tile, scan over the tiles, write

    def chain(tile):
        """[(literal segment begin, end, sequence position or None)] of the tile's part of the chain"""
        pos, tile_end, out = entry[tile], min((tile + 1) * T, n), []
        while pos < tile_end:
            p = next((g for g in range(pos, tile_end) if slen[g]), tile_end)
            out.append((pos, p, p if p < tile_end else None))
            if p >= tile_end:
                break
            pos = p + slen[p]
        return out

    cnt, msum, lend = [0] * n_tiles, [0] * n_tiles, [0] * n_tiles
    for tile in range(n_tiles):
        if entry[tile] != NONE:
            ps = [p for _, _, p in chain(tile) if p is not None]
            cnt[tile], msum[tile] = len(ps), sum(slen[p] for p in ps)
            lend[tile] = ps[-1] + slen[ps[-1]] if ps else 0
    seq_off, m_off, prev_end = [0] * (n_tiles + 1), [0] * (n_tiles + 1), [0] * (n_tiles + 1)
    for tile in range(n_tiles):
        seq_off[tile + 1], m_off[tile + 1] = seq_off[tile] + cnt[tile], m_off[tile] + msum[tile]
        prev_end[tile + 1] = max(prev_end[tile], lend[tile])
    total = seq_off[n_tiles]
    rows, lits = {}, {}
    n_lit = n - start - m_off[n_tiles] if total <= seq_cap else None
    for tile in range(n_tiles):
        if entry[tile] == NONE:
            continue
        k, before, prev = seq_off[tile], m_off[tile], max(prev_end[tile], start)
        for a, b, p in chain(tile):
            if k < seq_cap or (k == total and total <= seq_cap):
                for j in range(a, b):
                    assert j - start - before not in lits
                    lits[j - start - before] = w[j]
            if p is None:
                break
            if k < seq_cap:
                rows[k] = (p - prev, slen[p], p - sq[p])
            elif k == seq_cap:
                n_lit = prev - start - before
            prev = p + slen[p]
            before += slen[p]
            k += 1
    n_seq = min(total, seq_cap)
    assert sorted(rows) == list(range(n_seq)) and sorted(lits) == list(range(n_lit)), "rows and literals without gaps"
    info = dict(steps=steps, resolved=resolved, skipped=sum(1 for t in range(start // T, n_tiles) if entry[t] == NONE))
    return (np.array([rows[k] for k in range(n_seq)], np.int64).reshape(-1, 3),
            np.array([lits[i] for i in range(n_lit)], np.uint8), ST_CAPACITY if total > seq_cap else 0, info)


def replay_wide_restated(history, seqs, literals, cap=None):
    """The wide replay step by step -> (new bytes, status, rounds that moved a root)"""
    hist = np.asarray(history, np.uint8)
    seqs = np.asarray(seqs, np.int64).reshape(-1, 3)
    lit = np.asarray(literals, np.uint8)
    have, n_seq, n_lit = len(hist), len(seqs), len(lit)
    cap = have + n_lit + int(seqs[:, 1].sum()) + int(seqs[:, 0].sum()) if cap is None else cap
    d = have + np.concatenate([[0], np.cumsum(seqs[:, 0] + seqs[:, 1])])  # the output position in front of sequence k
    lp = np.concatenate([[0], np.cumsum(seqs[:, 0])])                     # the literal position in front of it

    def check(k):
        run, length, off = seqs[k].tolist()
        if lp[k] > n_lit or run > n_lit - lp[k]:
            return ST_TRUNCATED, False
        if d[k] > cap or run > cap - d[k]:
            return ST_CAPACITY, False
        if off == 0 or off > d[k] + run:
            return ST_STATE, True
        if length > cap - d[k] - run:
            return ST_CAPACITY, True
        return 0, True

    first = min((k for k in range(n_seq) if check(k)[0]), default=n_seq)
    if first < n_seq:
        status, with_literals = check(first)
        end = d[first] + (seqs[first, 0] if with_literals else 0)
    else:
        rest = n_lit - lp[n_seq]
        status, end = (ST_CAPACITY, d[n_seq]) if rest > cap - d[n_seq] else (0, d[n_seq] + rest)
    end = int(end)
    out = np.concatenate([hist, np.zeros(end - have, np.uint8)])
    root, places = np.arange(end, dtype=np.int64), d.tolist()
    for i in range(have, end):
        k = bisect.bisect_right(places, i, 0, n_seq + 1) - 1
        run = seqs[k, 0] if k < n_seq else end
        if i - d[k] < run:
            out[i] = lit[lp[k] + i - d[k]]
        else:
            m, off = d[k] + run, seqs[k, 2]
            root[i] = m - off + (i - m) % off
    rounds = 0
    bound = int(np.ceil(np.log2(n_seq + 1))) + 1
    while True:
        hop = root[root]
        if np.array_equal(hop, root):
            break
        root, rounds = hop, rounds + 1
    assert rounds <= bound, (rounds, bound)
    out[have:] = out[root[have:]]
    return out[have:], int(status), rounds
