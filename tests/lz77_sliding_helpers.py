"""Shared by the sliding-window LZ77 tests: the goldens and an independent restatement of the parse rule and of the
windowed replay, with the named wrong variants the goldens must tell apart; the bucket index restated
from its definition (keys, sort, inverse, bitmap) with the scratch layout it is read at, and the inputs of
test_gpu_lz77_sliding_limits.py: the cases of the white-box index test, one long stream and one block for the classes.

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
from lz77_helpers import ST_CAPACITY, ST_STATE, ST_TRUNCATED, _common_prefix, _round_up, index_shape

MASK = (1 << 64) - 1
NO_KEY = 0xFFFFFFFF  # key[] of a position without a whole gram inside its stream
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


# ---- the bucket index, restated ("The index") ---------------------------------------------------------------
def key_passes(m):
    """sort passes over the key: the bytes of the largest bucket number m - 1, at least one, at most four"""
    passes = 1
    while passes < 4 and (m - 1) >> (8 * passes):
        passes += 1
    return passes


def stream_passes(n_streams):
    """sort passes over the stream number: the bytes of n_streams (the number of the bytes outside every stream); none for
    a batch of one stream"""
    passes = 0
    while n_streams >> (8 * passes):
        passes += 1
    return passes if n_streams > 1 else 0


def sort_passes(m, n_streams):
    return key_passes(m) + stream_passes(n_streams)


def buckets_restated(buf, hl, m):
    """bucket() at every position of `buf` that has hl bytes, in wrap-around uint64 arithmetic on whole arrays: the hash is
    read as a signed number and reduced to the non-negative remainder.  -> int64 [max(len(buf) - hl + 1, 0)]"""
    buf = np.asarray(buf, np.uint8)
    n = len(buf) - hl + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    with np.errstate(over="ignore"):
        acc = np.full(n, 0x27D4EB2F165667C5, np.uint64)
        for j in range(hl):
            acc = acc + buf[j: j + n].astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
            acc = (acc << np.uint64(31)) | (acc >> np.uint64(33))
            acc = acc * np.uint64(0x9E3779B185EBCA87)
        acc = acc + np.uint64(hl ^ (0x27D4EB2F165667C5 ^ 3527539))
    acc[acc == np.uint64(MASK)] = np.uint64(1546275796)
    return np.mod(acc.view(np.int64), np.int64(m))  # numpy's mod has the sign of the divisor, as Python's %


def sliding_index_shape(N):
    """The scratch of one sliding-window parse call over N bytes, restated from sliding_scratch_layout: the greedy index's
    parts (lz77_helpers.index_shape) and behind them key[], 4 N bytes rounded up to 256, an empty one taking 256.
    -> index_shape's namespace with key and total replaced"""
    sh = index_shape(N)
    sh.key = sh.total
    sh.total = sh.key + _round_up(max(4 * N, 1), 256)
    return sh


def sliding_index_restated(buf, win_off, hl, m, W):
    """The definition of the bucket index of a batch -> (key [N], order [N], rank [N]: int64; bitmap: uint64 words).
    key[g] is the bucket of the hl-gram at g where g lies in a stream s and g + hl <= min(win_off[s + 1], N), else NO_KEY.
    order is the STABLE sort of all positions by (stream digit, key digit): the stream digit is the stream of g, n_streams
    outside every stream, and nothing at all for a batch of one stream; the key digit is the low key_passes(m) bytes of the
    key (so with fewer than four passes NO_KEY sorts as its low bytes).  rank is the inverse.  Bit g of the bitmap, with
    c = order[rank[g] - 1]: key[g] != NO_KEY, rank[g] > 0, win_off[s] <= c < g, g - c <= W (W = 0: no bound) and the
    whole key[c] == key[g]."""
    buf, win_off = np.asarray(buf, np.uint8), np.asarray(win_off, np.int64)
    N, n_streams = len(buf), len(win_off) - 1
    v = np.arange(N, dtype=np.int64)
    stream = np.searchsorted(win_off, v, side="right") - 1  # the last s with win_off[s] <= v, of all n_streams + 1 entries
    stream[(stream < 0) | (stream >= n_streams)] = n_streams
    end = np.minimum(np.append(win_off[1:], 0)[stream], N)
    base = np.append(win_off[:-1], 0)[stream]
    key = np.full(N, NO_KEY, np.int64)
    whole = (stream < n_streams) & (v + hl <= end)
    key[whole] = buckets_restated(buf, hl, m)[v[whole]]
    stream_digit = stream & (256 ** stream_passes(n_streams) - 1)
    key_digit = key & (256 ** key_passes(m) - 1)
    order = np.lexsort((key_digit, stream_digit)).astype(np.int64)
    rank = np.empty(N, np.int64)
    rank[order] = v
    c = order[np.maximum(rank - 1, 0)] if N else order
    bit = np.zeros(_round_up(N, 64), bool)
    bit[:N] = (key != NO_KEY) & (rank > 0) & (base <= c) & (c < v) & (v - c <= (W if W else 1 << 62)) & (key[c] == key)
    return key, order, rank, np.packbits(bit, bitorder="little").view(np.uint64)


def assert_index_equal(got, want, N, what=""):
    """(key, order, rank, bitmap words) of the device against the definition's, stage by stage: the message names the first
    stage that is wrong -- keys, sort, inverse or bitmap.  Only bitmap bits below N count."""
    (key, order, rank, bitmap), (want_key, want_order, want_rank, want_bitmap) = got, want
    bad = np.flatnonzero(np.asarray(key, np.int64) != want_key)
    assert bad.size == 0, f"{what}: key[] differs at position {bad[0]} ({bad.size} positions): keys (lz77_sliding_keys)"
    bad = np.flatnonzero(np.asarray(order, np.int64) != want_order)
    assert bad.size == 0, f"{what}: order[] differs from entry {bad[0]} on ({bad.size} entries) with key[] right: sort"
    bad = np.flatnonzero(np.asarray(rank, np.int64) != want_rank)
    assert bad.size == 0, f"{what}: rank[] differs at position {bad[0]} with order[] right: inverse (the last scatter pass)"
    bitmap = np.array(bitmap, np.uint64)
    if N % 64:
        bitmap[-1] &= np.uint64((1 << (N % 64)) - 1)
    bad = np.flatnonzero(bitmap != want_bitmap)
    assert bad.size == 0, f"{what}: bitmap word {bad[0]} differs with key[], order[] and rank[] right: bitmap (lz77_sliding_bitmap)"


def bits_of(bitmap, N):
    """the bitmap words as N booleans"""
    return np.unpackbits(np.asarray(bitmap, np.uint64).view(np.uint8), bitorder="little")[:N].astype(bool)


# The one-stream batch at m = 256: NO_KEY sorts as 0xFF there, next to bucket 255.  Of all grams of 1..8 bytes over the two
# symbols of edge_batch(1) only (0, 1, 1, 1, 0, 0) falls into bucket 255, so these cases hash 6 bytes, and the seed is one
# whose stream holds that gram (test_lz77_sliding_host.py asserts it).
ONE_STREAM_SEED, ONE_STREAM_HL = 1, 6


INDEX_CASES = (  # (batch, hl, m, W, sort passes = key passes + stream-number passes) of the white-box index test
    ("ragged", 4, 1, 16, 1 + 1), ("ragged", 4, 256, 50, 1 + 1), ("ragged", 4, 257, 1000, 2 + 1),
    ("ragged", 4, 65536, 1000, 2 + 1), ("ragged", 4, (1 << 24) + 1, 0, 4 + 1), ("ragged", 4, (1 << 32) - 1, 1000000, 4 + 1),
    ("ragged", 1, 256, 50, 1 + 1), ("ragged", 8, 256, 50, 1 + 1),
    ("one", ONE_STREAM_HL, 256, 60, 1 + 0), ("one", ONE_STREAM_HL, (1 << 32) - 1, 60, 4 + 0),
    ("edge257", 3, 65537, 60, 3 + 2), ("edge257", 3, 1 << 24, 60, 3 + 2), ("edge257", 3, (1 << 24) + 1, 60, 4 + 2),
    ("tiled", 4, (1 << 24) + 1, 1000000, 4 + 3), ("tiled", 3, 1, 40, 1 + 3))


def index_batch(name):
    from lz77_helpers import edge_batch, ragged_batch, tiled_batch

    return {"ragged": ragged_batch, "one": lambda: edge_batch(1, ONE_STREAM_SEED), "edge257": lambda: edge_batch(257),
            "tiled": tiled_batch}[name]()


# ---- one long stream -------------------------------------------------------------------------------------------------------------
LONG_N = 40170
LONG_STEP = 4096       # positions lz_next_bit covers per iteration: 64 words of 64 bits
LONG_LEAD = 90         # bytes of the short stream in front of the long one in long_batch(True)
# (where, from where, bytes) of the planted repeats, in the order they are copied
LONG_PLANTS = ((500, 100, 30),         # 400 back
               (1700, 700, 12),        # exactly 1000 back: the farthest W = 1000 takes
               (3000, 1999, 12),       # 1001 back: the nearest W = 1000 refuses
               (15391, 40, 30),        # far: behind 12 379 bytes without a repeat
               (15430, 15000, 20),     # 430 back
               (27801, 200, 40),       # far: behind 12 351 bytes without a repeat
               (27850, 27400, 16),     # 450 back
               (LONG_N - 4, 300, 4))   # far: the last position that has a gram of 4, behind 12 300 bytes without a repeat
LONG_PARAMS = ((4, (1 << 32) - 1, 64, 0, 1, 4),   # (hl, m, C, W, lazy, mml): no window, a bucket per gram
               (4, (1 << 32) - 1, 64, 1000, 1, 4),  # the far repeats and the one 1001 back lie outside the window
               (4, 65536, 64, 5000, 1, 4))          # bucket collisions: bitmap bits that lead to no match


@functools.lru_cache(maxsize=None)
def long_stream():
    """LONG_N random bytes over 256 symbols with LONG_PLANTS copied in: three stretches of at least 3 * 4096 bytes without a
    repeat, each ended by a copy of bytes from the start of the stream; repeats 400, 430 and 450 back, one exactly 1000
    back and one 1001 back."""
    w = np.random.default_rng(42).integers(0, 256, LONG_N).astype(np.uint8)
    for at, src, k in LONG_PLANTS:
        w[at: at + k] = w[src: src + k]
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def long_batch(between):
    """long_stream() alone behind pack_windows' one filler byte (base 1), or as the middle stream of three between short
    ones of LONG_LEAD and 75 bytes (base 1 + LONG_LEAD): both bases are odd"""
    from lz77_helpers import pack_windows

    rng = np.random.default_rng(43)
    if not between:
        return pack_windows([long_stream()], [0])
    return pack_windows([rng.integers(0, 3, LONG_LEAD).astype(np.uint8), long_stream(), rng.integers(0, 3, 75).astype(np.uint8)],
                        [0, 0, 7])


@functools.lru_cache(maxsize=None)
def long_reference(p):
    """parse_restated of long_stream() for p = (hl, m, C, W, lazy, mml)"""
    hl, m, C, W, lazy, mml = p
    return parse_restated(long_stream(), 0, (hl, m, C, lazy, mml, W))


def long_gaps(seqs):
    """the literal runs of at least 3 * LONG_STEP bytes that end in a match: [(first position, bytes)] within the stream"""
    seqs = np.asarray(seqs, np.int64).reshape(-1, 3)
    at = np.concatenate([[0], np.cumsum(seqs[:, 0] + seqs[:, 1])])[:-1]
    return [(int(a), int(run)) for a, (run, length, _) in zip(at, seqs) if run >= 3 * LONG_STEP and length > 0]


# ---- one block through the classes -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_block():
    """-> (history of 1500 bytes, block of 100 000 bytes): words of 5..12 random bytes drawn from a vocabulary of 800, so
    that a word's last occurrence lies inside a window of 1000 bytes for some and outside for most"""
    rng = np.random.default_rng(47)
    vocabulary = [rng.integers(0, 256, int(k)).astype(np.uint8) for k in rng.integers(5, 13, 800)]
    text = np.concatenate([vocabulary[i] for i in rng.integers(0, 800, 13000)])
    assert text.size >= 101500
    return text[:1500].copy(), text[1500:101500].copy()
