"""Shared by the LZ77 tests: the goldens, an independent restatement of the parse rule and of sequence replay, a host
stand-in for the prefix-code device calls (so that the host code above them can be checked without a GPU), and the byte
sources the GPU tests draw their streams from.

The parse rule.  w[0..n) is the window, the block starts at s, L = min_match_length, M =
max_num_matches_considered.  A candidate for p (p + L <= n) is a q <= p - L with w[q..q+L) == w[p..p+L); candidates are
taken newest first, at most M of them (M = 0: all); a candidate's score is the longest l with w[q+i] == w[p+i] for i < l and
p + l <= n; the longest wins, the newest on ties.  From pos = s: the first p >= pos with a candidate gives the sequence
(p - pos, best length, p - best q), and pos = p + best length; without one the rest of the window is literals.
"""
import bisect
import functools
import types

import numpy as np

from conftest import load_golden

ST_CAPACITY, ST_TRUNCATED, ST_STATE, ST_SIZE = 0x1, 0x4, 0x8, 0x20


@functools.lru_cache(maxsize=None)
def goldens():
    cases = load_golden("lz77")
    return {k: [c for c in cases if c.kind == k] for k in ("lz77", "elias", "logbin", "empirical", "file")}


def golden_blocks(case):
    """[(window before the block: uint8 array, block data, sequences [k, 3], literals, packed bits, nbits, consumed per
    garbage length)] of a kind "lz77" case, in order"""
    window, out = case.arr("init"), []
    for b in range(case.n_blocks):
        if case.reset_before[b]:
            window = np.zeros(0, np.uint8)
        data = case.arr(f"b{b}_data")
        out.append((window, data, case.arr(f"b{b}_seq").astype(np.int64), case.arr(f"b{b}_lit"), case.arr(f"b{b}_out"),
                    case.nbits[b], case.consumed[b]))
        window = np.concatenate([window, data])
    return out


def with_garbage(case, packed, nbits):
    """[(0/1 bit array of the code followed by each stored garbage, index into ``consumed``)]"""
    base = np.unpackbits(np.asarray(packed, np.uint8))[:nbits]
    return [(np.concatenate([base, case.arr(f"garbage{g}")]) if g else base, i) for i, g in enumerate(case.garbage_lens)]


# ---- the parse rule --------------------------------------------------------------------------------------------------------
def _common_prefix(w: bytes, q: int, p: int, limit: int) -> int:
    """largest l <= limit with w[q:q+l] == w[p:p+l]"""
    if w[q:q + limit] == w[p:p + limit]:
        return limit
    lo, hi = 0, limit  # equal for lo, different for hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if w[q + lo:q + mid] == w[p + lo:p + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def parse_restated(window, start, L, M):
    """-> (sequences as an int64 array [k, 3], literals as a uint8 array)"""
    w = bytes(np.asarray(window, np.uint8))
    n = len(w)
    where = {}
    for q in range(n - L + 1):
        where.setdefault(w[q:q + L], []).append(q)
    seqs, lits, pos, p = [], bytearray(), start, start
    while p + L <= n:
        occurrences = where[w[p:p + L]]
        n_cand = bisect.bisect_right(occurrences, p - L)
        if n_cand == 0:
            p += 1
            continue
        newest_first = occurrences[:n_cand][::-1]
        if M:
            newest_first = newest_first[:M]
        best_len, best_q = 0, -1
        for q in newest_first:
            length = _common_prefix(w, q, p, n - p)
            if length > best_len:
                best_len, best_q = length, q
        seqs.append((p - pos, best_len, p - best_q))
        lits += w[pos:p]
        pos = p = p + best_len
    lits += w[pos:]
    return np.array(seqs, np.int64).reshape(-1, 3), np.frombuffer(bytes(lits), np.uint8)


# ---- replay ----------------------------------------------------------------------------------------------------------------
def replay_restated(history, seqs, literals, cap=None):
    """-> (new bytes: uint8 array, status).  A window of at most ``cap`` bytes (None: no limit); per sequence the literals
    are checked (ST_TRUNCATED: more asked than left; ST_CAPACITY), then the match (ST_STATE: offset 0 or beyond the bytes
    so far; ST_CAPACITY); the stream stops at its first fault and keeps what came before."""
    out = bytearray(bytes(np.asarray(history, np.uint8)))
    have, lit, at = len(out), bytes(np.asarray(literals, np.uint8)), 0
    cap = float("inf") if cap is None else cap
    for run, length, off in np.asarray(seqs, np.int64).reshape(-1, 3).tolist():
        if run > len(lit) - at:
            return np.frombuffer(bytes(out[have:]), np.uint8), ST_TRUNCATED
        if len(out) + run > cap:
            return np.frombuffer(bytes(out[have:]), np.uint8), ST_CAPACITY
        out += lit[at:at + run]
        at += run
        if off == 0 or off > len(out):
            return np.frombuffer(bytes(out[have:]), np.uint8), ST_STATE
        if len(out) + length > cap:
            return np.frombuffer(bytes(out[have:]), np.uint8), ST_CAPACITY
        for _ in range(length):
            out.append(out[-off])
    if len(out) + len(lit) - at > cap:
        return np.frombuffer(bytes(out[have:]), np.uint8), ST_CAPACITY
    out += lit[at:]
    return np.frombuffer(bytes(out[have:]), np.uint8), 0


# ---- the prefix-code device calls, on the host -----------------------------------------------------------------------------
def use_host_prefix_coder(monkeypatch):
    """HuffmanEncoder.encode_block / HuffmanDecoder.decode_block normally run on the GPU; for the CPU tests of the host code
    ABOVE them (headers, counts, binning) they are replaced by the stream's definition: the codewords back to back, and a
    walk down the tree until the bits are used up."""
    from stanford_compression_library_amd.compressors.prefix_free_compressors import PrefixFreeDecoder, PrefixFreeEncoder
    from stanford_compression_library_amd.core.data_block import DataBlock
    from stanford_compression_library_amd.utils.bitarray_utils import BitArray

    def encode_block(self, data_block):
        table = self._code_table()
        parts = [table[s]._b for s in data_block.data_list]
        return BitArray._wrap(np.concatenate(parts) if parts else np.zeros(0, np.uint8))

    def decode_block(self, bitarray):
        bits, out, used = bitarray.tolist(), [], 0
        while used < len(bits):
            node = self.tree.root_node
            while not node.is_leaf_node:
                node = node.right_child if bits[used] else node.left_child
                used += 1
            out.append(node.id)
        return DataBlock(out), used

    monkeypatch.setattr(PrefixFreeEncoder, "encode_block", encode_block)
    monkeypatch.setattr(PrefixFreeDecoder, "decode_block", decode_block)


# ---- byte sources ----------------------------------------------------------------------------------------------------------
def markov1_stream(n, seed):
    """n bytes of the benchmark suite's first-order Markov source over 16 symbols (bench_data.markov1_host)"""
    from stanford_compression_library_amd import bench_data

    return bench_data.markov1_host(16, n, seed=seed)


def markov1_long_stream(n, seed):
    """markov1_stream(n, seed) byte for byte, in a tenth of the time, for streams of a MiB: all 16 possible successors of every
    step come from one vectorised comparison (what searchsorted(row, u, side="right") counts: the entries <= u), and only
    the walk through them is a loop.  tests/test_lz77_wide_host.py holds it against markov1_stream."""
    K, piece = 16, 1 << 16
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(rng.dirichlet(0.3 * np.ones(K), size=K), axis=1)
    u = rng.random(n)
    out, prev = bytearray(n), 0
    for a in range(0, n, piece):
        nxt = np.minimum((cdf[None, :, :] <= u[a: a + piece, None, None]).sum(axis=2), K - 1).astype(np.uint8).tobytes()
        for t in range(len(nxt) // K):
            out[a + t] = prev = nxt[K * t + prev]
    return np.frombuffer(out, np.uint8).copy()


@functools.lru_cache(maxsize=None)
def ragged_batch(n_streams=130, seed=5):
    """130 streams of 0..3000 bytes over alphabets of 2, 4 and 256 symbols, histories of 0, 3 and 1000 bytes, packed back to
    back from an odd offset on.  Every 13th stream is a short pattern repeated with a few bytes changed (long matches, and
    more than 64 candidates that all run far).  Two-symbol streams stay below 700 bytes and four-symbol ones below 1200:
    with M = 0 their candidate lists grow with the stream, and the restatement is a Python loop.
    -> dict(buf, win_off [n + 1], start [n], windows = [uint8 arrays])"""
    rng = np.random.default_rng(seed)
    windows, start = [], []
    for s in range(n_streams):
        k = (2, 4, 256)[s % 3]
        hist = (0, 3, 1000)[(s // 3) % 3]
        top = {2: 700, 4: 1200, 256: 3000}[k]
        n = (0, 1, top)[s] if s < 3 else int(rng.integers(0, top + 1))
        w = rng.integers(0, k, n).astype(np.uint8)
        if s % 13 == 5 and n:
            w = np.resize(w[: int(rng.integers(1, 41))], n)
            flips = rng.integers(0, n, n // 200)
            w[flips] = rng.integers(0, k, flips.size)
        windows.append(w)
        start.append(min(hist, n))
    return pack_windows(windows, start)


def pack_windows(windows, start, lead=None, tail=None):
    """the windows back to back behind ONE filler byte, so that the first offset is odd and, with ragged lengths, so are
    many of the others: window s = buf[win_off[s]:win_off[s + 1]].  `lead` replaces the filler byte by bytes of the
    caller's, `tail` adds bytes behind the last window: both belong to no stream."""
    lead = np.full(1, 0xA5, np.uint8) if lead is None else np.asarray(lead, np.uint8)
    tail = np.zeros(0, np.uint8) if tail is None else np.asarray(tail, np.uint8)
    lens = np.array([len(w) for w in windows], np.int64)
    win_off = len(lead) + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf = np.concatenate([lead] + [np.asarray(w, np.uint8) for w in windows] + [tail])
    return dict(buf=buf, win_off=win_off, start=np.array(start, np.int32), windows=[np.asarray(w, np.uint8) for w in windows])


@functools.lru_cache(maxsize=None)
def ragged_reference(L, M):
    """parse_restated of every stream of ragged_batch(): [(sequences, literals)]"""
    b = ragged_batch()
    return [parse_restated(w, int(s), L, M) for w, s in zip(b["windows"], b["start"])]


# ---- the batch past every limit of the index ---------------------------------------------------------------------------------
TILED_STREAMS, TILED_TEMPLATES = 70000, 61


@functools.lru_cache(maxsize=None)
def tiled_batch(n_streams=TILED_STREAMS, seed=11):
    """n_streams short streams drawn from K = 61 templates of 97..160 bytes over alphabets of 2, 4 and 256 symbols; every
    fifth template is a period of 3..6 bytes repeated (all candidates tie at "runs to the end": the newest wins only if
    the sort is stable).  Stream s is template ids[s]; every block starts at 0.  ids = s % K, except that every third
    group of four streams is one template four times: different AND identical neighbours.  With 70 000 streams the batch
    has more than 65 536 streams (three stream-number passes of the sort) and more than 8 388 608 bytes (more than 256 scan
    blocks).  The restatement is needed for the K templates only: tiled_reference().
    -> pack_windows' dict + templates = [uint8 arrays], ids [n_streams]"""
    rng = np.random.default_rng(seed)
    K = TILED_TEMPLATES
    templates = []
    for t in range(K):
        n, k = int(rng.integers(97, 161)), (2, 4, 256)[t % 3]
        w = rng.integers(0, k, n).astype(np.uint8)
        if t % 5 == 4:
            w = np.resize(w[: int(rng.integers(3, 7))], n)
        templates.append(w)
    s = np.arange(n_streams)
    ids = np.where((s // 4) % 3 == 0, (s // 4) % K, s % K)
    batch = pack_windows([templates[t] for t in ids.tolist()], np.zeros(n_streams, np.int32))
    return dict(batch, templates=templates, ids=ids)


@functools.lru_cache(maxsize=None)
def tiled_reference(L, M):
    """parse_restated of the K templates of tiled_batch(): [(sequences, literals)]; stream s has entry ids[s]"""
    return [parse_restated(w, 0, L, M) for w in tiled_batch()["templates"]]


# ---- the index, restated ---------------------------------------------------------------------------------------------------------
def _round_up(x, to):
    return (x + to - 1) // to * to


def index_shape(N):
    """The scratch of one parse call over N bytes, restated from csrc/scl_lz77_internal.h: a sort tile is 4096 positions, the
    tile histograms are 256 x tiles counts, a scan block is 2048 of them, the bitmap has a 64-bit word per 64 positions;
    the parts order_a, order_b, rank (4 N bytes each), bitmap, hist, block_sums follow each other, each rounded up to 256
    bytes, an empty one taking 256.
    -> namespace(n_tiles, n_hist, n_scan_blocks, n_words, order_a, order_b, rank, bitmap, hist, block_sums, total)"""
    sh = types.SimpleNamespace(n_tiles=(N + 4095) // 4096)
    sh.n_hist = 256 * sh.n_tiles
    sh.n_scan_blocks = (sh.n_hist + 2047) // 2048
    sh.n_words = (N + 63) // 64
    at = 0
    for name, size in (("order_a", 4 * N), ("order_b", 4 * N), ("rank", 4 * N), ("bitmap", 8 * sh.n_words),
                       ("hist", 4 * sh.n_hist), ("block_sums", 4 * sh.n_scan_blocks)):
        setattr(sh, name, at)
        at += _round_up(max(size, 1), 256)
    sh.total = at
    return sh


def index_restated(buf, win_off, L):
    """The definition of the match index of a batch -> (order [N] int64, rank [N] int64, bitmap: uint64
    words).  order is the STABLE sort of all N positions by (stream of v, L-gram at v): the gram is the L bytes from v on
    as a little-endian number, read as they lie -- into the next stream, and as 0 past the buffer; the stream of a position
    outside every stream is n_streams.  A batch of one stream is sorted by the gram alone (there is no stream-number pass
    for it).  rank is the inverse of order.  Bit g of the bitmap: g + L <= end of g's stream (the end clamped to N), and
    the oldest equal gram of that stream lies at q <= g - L."""
    buf, win_off = np.asarray(buf, np.uint8), np.asarray(win_off, np.int64)
    N, n_streams = len(buf), len(win_off) - 1
    v = np.arange(N, dtype=np.int64)
    stream = np.searchsorted(win_off, v, side="right") - 1  # the last s with win_off[s] <= v, of all n_streams + 1 entries
    stream[(stream < 0) | (stream >= n_streams)] = n_streams
    padded = np.concatenate([buf, np.zeros(L, np.uint8)]).astype(np.uint64)
    gram = np.zeros(N, np.uint64)
    for j in range(L):
        gram |= padded[j: j + N] << np.uint64(8 * j)
    order = np.lexsort((gram, stream)) if n_streams > 1 else np.argsort(gram, kind="stable")
    order = order.astype(np.int64)
    rank = np.empty(N, np.int64)
    rank[order] = v
    # the groups of equal (stream, gram) along order[]: the first entry of a group is its oldest position
    ss, gg = stream[order], gram[order]
    first = np.ones(N, bool)
    first[1:] = (ss[1:] != ss[:-1]) | (gg[1:] != gg[:-1])
    oldest = order[np.maximum.accumulate(np.where(first, v, 0))] if N else order
    end = np.minimum(np.append(win_off[1:], 0)[ss], N)
    bit = np.zeros(_round_up(N, 64), bool)
    bit[order] = (ss < n_streams) & (order + L <= end) & (oldest + L <= order)
    return order, rank, np.packbits(bit, bitorder="little").view(np.uint64)


@functools.lru_cache(maxsize=None)
def edge_batch(n_streams, seed=23):
    """n_streams streams of 40..90 bytes over 2 to 4 symbols between bytes that belong to no stream but look like stream
    content: a lead of 40 bytes that copies the start of stream 0 and a tail of 40 bytes that copies the start of the last
    stream that has bytes.  Every third stream is an identical copy of the one in front of it; from 8 streams on, three
    streams in the middle and the last three are empty.  Histories of 0 and 7 bytes.
    -> pack_windows' dict; the buffer is 40 bytes longer than win_off[-1]"""
    rng = np.random.default_rng(seed + n_streams)
    empty = set()
    if n_streams >= 8:
        mid = n_streams // 2
        empty = {mid, mid + 1, mid + 2, n_streams - 3, n_streams - 2, n_streams - 1}
    windows = []
    for s in range(n_streams):
        if s in empty:
            windows.append(np.zeros(0, np.uint8))
        elif s % 3 == 2 and len(windows[-1]):
            windows.append(windows[-1].copy())
        else:
            windows.append(rng.integers(0, 2 + s % 3, int(rng.integers(40, 91))).astype(np.uint8))
    start = [min((0, 7)[s % 2], len(w)) for s, w in enumerate(windows)]
    last = [w for w in windows if len(w)][-1]
    return pack_windows(windows, start, lead=windows[0][:40], tail=last[:40])


@functools.lru_cache(maxsize=None)
def edge_reference(n_streams, L, M):
    b = edge_batch(n_streams)
    return [parse_restated(w, int(s), L, M) for w, s in zip(b["windows"], b["start"])]


def parse_with_order(buf, win_off, start, s, L, M, order):
    """What the device parse makes of stream s given ANY permutation `order` of the positions as its index (rank = the
    inverse, the bitmap by the kernel's own looks at the L entries in front of rank[g]).  It takes the entries in front of
    rank[p] newest first, re-checks stream and gram of each, scores them in groups of 64 and keeps the longest, the first
    on ties: with the true index that is the rule; with a wrong one it is still a valid parse -- of other matches.
    -> (sequences [k, 3], literals), as parse_restated"""
    w, order = bytes(np.asarray(buf, np.uint8)), np.asarray(order).tolist()
    rank = {v: i for i, v in enumerate(order)}
    base, end = int(win_off[s]), int(win_off[s + 1])

    def ok(c, g):
        return base <= c and c + L <= g and w[c:c + L] == w[g:g + L]

    def has_candidate(g):
        for k in range(1, min(L, rank[g]) + 1):
            c = order[rank[g] - k]
            if c < base or c >= g or w[c:c + L] != w[g:g + L]:
                return False
            if c + L <= g:
                return True
        return False

    seqs, lits, pos = [], bytearray(), base + int(start[s])
    while True:
        p = next((g for g in range(pos, end - L + 1) if has_candidate(g)), None)
        if p is None:
            break
        i = rank[p]
        skip = sum(1 for j in range(min(L - 1, i)) if base <= order[i - 1 - j] < p < order[i - 1 - j] + L
                   and w[order[i - 1 - j]:order[i - 1 - j] + L] == w[p:p + L])
        best_len, best_q, group = 0, -1, 0
        while True:
            lanes = [order[i - 1 - skip - nth] for nth in range(group, group + 64) if skip + nth < i and (M == 0 or nth < M)]
            valid = [ok(c, p) for c in lanes]
            if not valid or not valid[0]:
                break
            for c in (c for c, v in zip(lanes, valid) if v):
                length = _common_prefix(w, c, p, end - p)
                if length > best_len:
                    best_len, best_q = length, c
            if len(lanes) < 64 or not all(valid) or (M and group + 64 >= M):
                break
            group += 64
        assert best_len, "the bitmap promised a candidate"
        seqs.append((p - pos, best_len, p - best_q))
        lits += w[pos:p]
        pos = p + best_len
    lits += w[pos:end]
    return np.array(seqs, np.int64).reshape(-1, 3), np.frombuffer(bytes(lits), np.uint8)
