// scl_lz77_internal.h -- shapes, scratch layout and shared device code of the LZ77 kernels (scl_lz77.hip: batches, one
// wavefront per stream; scl_lz77_wide.hip: one stream across the whole GPU; scl_lz77_sliding.hip: the sliding-window coder,
// one wavefront per stream; scl_lz77_sliding_wide.hip: that coder's one stream across the whole GPU).  Internal to csrc/.
//
// Written once for the greedy and the sliding-window coder, which differ in their match rule and in two replay rules:
//   device  lz_replay_frame<WINDOWED> (all of a replay kernel), the index sort, lz_score / lz_extend,
//           lz_replay_stream<WINDOWED>.  NOT what stands around the match rule of the two parse kernels (prologue, emit
//           step, epilogue): a frame around them left lz77_sliding_parse its registers but measured slower
//           (profiles/lz77_frame_codegen.txt, profiles/lz77_frame_timing.txt), so both kernels keep their own lines
//           lz_sliding_sequence / lz_sliding_best: the sliding-window coder's match rule, one sequence from E, for its
//           one-wave parse and its wide kernels alike (as lz_score serves both greedy parses)
//   entry   lz77_parse_check, lz77_scratch_carve, lz77_replay_launch, sliding_scratch_layout, sliding_check_params
//   host    LzMeta, LzHostFrame (parse_open / parse_close, replay_open / replay_close)
#pragma once

#include "scl_common.h"
#include "scl_scan.h"

// ---- the index sort: a stable LSD radix sort of the POSITIONS, 8-bit digits ------------------------------------------
// Nothing but the permutation moves: the digit of position v in pass d comes from a digit source (LzGramDigit below: in
// gram pass d the byte win[v + d], 0 past the buffer, in stream pass k byte k of v's stream number).  A tile is 4 waves x
// 16 rounds x 64 positions; a wave owns 1024 consecutive entries, so tile order, wave order, round order and lane order
// together are the input order (stability).
#define LZ_SORT_THREADS 256
#define LZ_SORT_ROUNDS 16
#define LZ_SORT_WAVES (LZ_SORT_THREADS / SCL_WAVE)
#define LZ_SORT_TILE (LZ_SORT_THREADS * LZ_SORT_ROUNDS)
#define LZ_SCAN_THREADS 256
#define LZ_SCAN_PER_THREAD 8
#define LZ_SCAN_BLOCK (LZ_SCAN_THREADS * LZ_SCAN_PER_THREAD)

// parse / replay: one wavefront per stream, four streams per workgroup
#define LZ_STREAM_THREADS 256
#define LZ_STREAMS_PER_BLOCK (LZ_STREAM_THREADS / SCL_WAVE)

// Device scratch of one parse call over N = total_bytes positions; every part starts on a 256-byte boundary.
struct Lz77Scratch {
    u64 order_a, order_b, rank, bitmap, hist, block_sums, total;  // byte offsets; total = bytes needed
    u64 n_tiles, n_hist, n_scan_blocks, n_words;
};

static inline Lz77Scratch lz77_scratch_layout(u64 N) {
    Lz77Scratch s;
    s.n_tiles = (N + LZ_SORT_TILE - 1) / LZ_SORT_TILE;
    s.n_hist = 256 * s.n_tiles;
    s.n_scan_blocks = (s.n_hist + LZ_SCAN_BLOCK - 1) / LZ_SCAN_BLOCK;
    s.n_words = (N + 63) / 64;
    SclCarver c;
    s.order_a = c.take(N * 4);
    s.order_b = c.take(N * 4);
    s.rank = c.take(N * 4);
    s.bitmap = c.take(s.n_words * 8);
    s.hist = c.take(s.n_hist * 4);
    s.block_sums = c.take(s.n_scan_blocks * 4);
    s.total = c.at;
    return s;
}

// Exclusive scan of data[0..n) in place, three kernels on `st` (scl_lz77.hip, over the workgroup scans of scl_scan.h);
// block_sums: ceil(n / LZ_SCAN_BLOCK) values.  V: u32 or u64.
template <class V>
void lz77_scan_exclusive(V *data, u64 n, V *block_sums, hipStream_t st);

// ---- the entry points' shared parts ------------------------------------------------------------------------------------
// the index part of a scratch buffer as pointers (the sliding-window coder adds its keys behind it)
struct Lz77ScratchPtrs {
    u32 *order_a, *order_b, *rank;
    u64 *bitmap;
    u32 *hist, *sums;
};

static inline Lz77ScratchPtrs lz77_scratch_carve(void *d_scratch, const Lz77Scratch &lay) {
    u8 *scr = (u8 *)d_scratch;
    return {(u32 *)(scr + lay.order_a), (u32 *)(scr + lay.order_b), (u32 *)(scr + lay.rank),
            (u64 *)(scr + lay.bitmap),  (u32 *)(scr + lay.hist),    (u32 *)(scr + lay.block_sums)};
}

// What scl_lz77_parse_batch and scl_lz77_sliding_parse_batch refuse alike, in one order: null pointers, the coder's own
// parameters (`params`: int() -> SCL_OK or the error), sizes, phases, the scratch buffer against `scratch_fn`.
template <class A, class Params>
static inline int lz77_parse_check(const char *what, const A *a, Params params,
                                   uint64_t (*scratch_fn)(uint64_t, uint64_t), const char *scratch_name) {
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_win_off && a->d_start && a->d_n_seq && a->d_n_lit && a->d_status && a->d_scratch &&
                    (a->total_bytes == 0 || (a->d_win && a->d_literals)) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    if (int rc = params()) return rc;
    SCL_REQUIRE(a->total_bytes < (1ull << 32) && a->n_streams < (1ull << 32),
                "%s: a batch holds less than 2^32 bytes and 2^32 streams", what);
    SCL_REQUIRE(a->phases <= 3, "%s: phases is a mask of SCL_LZ77_INDEX | SCL_LZ77_PARSE", what);
    const u64 need = scratch_fn(a->total_bytes, a->n_streams);
    SCL_REQUIRE(((uintptr_t)a->d_scratch & 255) == 0 && a->scratch_bytes >= need,
                "%s: d_scratch must be 256-byte aligned and hold %s = %llu bytes", what, scratch_name,
                (unsigned long long)need);
    return SCL_OK;
}

// ---- the sliding-window coder's scratch and parameters (scl_lz77_sliding.hip, scl_lz77_sliding_wide.hip) ------------------
#define LZ_NO_KEY 0xFFFFFFFFu  // m < 2^32, so no bucket has this number

struct SlidingScratch {
    Lz77Scratch index;  // order_a, order_b, rank, bitmap, hist, block_sums as in the greedy index
    u64 key, total;
};

static inline SlidingScratch sliding_scratch_layout(u64 N) {
    SlidingScratch s;
    s.index = lz77_scratch_layout(N);
    s.key = s.index.total;
    s.total = s.key + scl_round_up(N * 4 ? N * 4 : 1, 256);
    return s;
}

static inline int sliding_check_params(const char *what, u32 hl, u64 m, u32 C, u32 mml) {
    SCL_REQUIRE(hl >= 1 && hl <= 8, "%s: hash_length %u: 1 <= hash_length <= 8", what, hl);
    SCL_REQUIRE(m >= 1 && m < (1ull << 32), "%s: hash_table_size %llu: a bucket number is 32-bit, 1 <= hash_table_size < 2^32",
                what, (unsigned long long)m);
    SCL_REQUIRE(C >= 1 && C <= 64, "%s: max_chain_length %u: one candidate per lane, 1 <= max_chain_length <= 64", what, C);
    SCL_REQUIRE(mml >= 1, "%s: min_match_length 0: a match has at least one byte", what);
    return SCL_OK;
}

// ---- one stream in host memory: a batch of one around any of the parse / replay calls ------------------------------------
struct LzMeta {  // the small per-stream words of a batch of one, in one allocation
    u64 win_off[2];
    u64 lit_off;
    u32 start, n_seq, n_lit, status, have, out_len;
};

// Owns the device buffers of one host call.  *_open allocates, uploads and fills the fields every argument struct of its
// kind has (A: scl_lz77_parse_args / scl_lz77_sliding_parse_args, or the two replay structs); the caller adds its own
// fields, makes the call, and *_close synchronises, reads the meta words back and downloads.
struct LzHostFrame {
    ScratchDev d_win, d_lit, d_seq, d_meta, d_scr;
    LzMeta meta = {};
    u32 *d_lc = nullptr, *d_ml = nullptr, *d_mo = nullptr;  // the three rows in d_seq

    int alloc(u64 win_bytes, u64 lit_bytes, u64 seq_cap, u64 scratch_bytes) {
        int rc;
        if ((rc = d_win.alloc(win_bytes)) || (rc = d_lit.alloc(lit_bytes)) || (rc = d_seq.alloc(3 * seq_cap * 4)) ||
            (rc = d_meta.alloc(sizeof(LzMeta))) || (rc = d_scr.alloc(scratch_bytes)))
            return rc;
        d_lc = (u32 *)d_seq.p;
        d_ml = d_lc + seq_cap;
        d_mo = d_ml + seq_cap;
        return SCL_OK;
    }

    template <class A>
    int parse_open(A &a, const u8 *h_window, u64 n, u64 start, u64 seq_cap, u64 scratch_bytes) {
        if (int rc = alloc(n, n, seq_cap, scratch_bytes)) return rc;
        meta.win_off[1] = n;
        meta.start = (u32)start;
        if (n) SCL_HIP_TRY(hipMemcpy(d_win.p, h_window, n, hipMemcpyHostToDevice));
        SCL_HIP_TRY(hipMemcpy(d_meta.p, &meta, sizeof(meta), hipMemcpyHostToDevice));
        LzMeta *dm = (LzMeta *)d_meta.p;
        a.d_win = (const u8 *)d_win.p;
        a.d_win_off = dm->win_off;
        a.d_start = &dm->start;
        a.n_streams = 1;
        a.total_bytes = n;
        a.seq_cap = (u32)seq_cap;
        a.d_lit_count = d_lc;
        a.d_match_len = d_ml;
        a.d_match_off = d_mo;
        a.d_literals = (u8 *)d_lit.p;
        a.d_n_seq = &dm->n_seq;
        a.d_n_lit = &dm->n_lit;
        a.d_status = &dm->status;
        a.d_scratch = d_scr.p;
        a.scratch_bytes = scratch_bytes;
        return SCL_OK;
    }

    // a stream the parse gave up on reports its status and downloads nothing
    int parse_close(const char *what, u64 start, u32 *h_lit_count, u32 *h_match_len, u32 *h_match_off, u64 *n_seq,
                    u8 *h_literals, u64 *n_lit) {
        SCL_HIP_TRY(hipDeviceSynchronize());
        SCL_HIP_TRY(hipMemcpy(&meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost));
        *n_seq = meta.n_seq;
        *n_lit = meta.n_lit;
        if (meta.status) return scl_status_to_error(meta.status, what);
        if (meta.n_seq) {
            SCL_HIP_TRY(hipMemcpy(h_lit_count, d_lc, meta.n_seq * 4ull, hipMemcpyDeviceToHost));
            SCL_HIP_TRY(hipMemcpy(h_match_len, d_ml, meta.n_seq * 4ull, hipMemcpyDeviceToHost));
            SCL_HIP_TRY(hipMemcpy(h_match_off, d_mo, meta.n_seq * 4ull, hipMemcpyDeviceToHost));
        }
        if (meta.n_lit) SCL_HIP_TRY(hipMemcpy(h_literals, (u8 *)d_lit.p + start, meta.n_lit, hipMemcpyDeviceToHost));
        return SCL_OK;
    }

    template <class A>
    int replay_open(A &a, const u8 *h_window, u64 have, u64 cap, const u32 *h_lit_count, const u32 *h_match_len,
                    const u32 *h_match_off, u64 n_seq, const u8 *h_literals, u64 n_lit, u64 scratch_bytes) {
        if (int rc = alloc(cap, n_lit, n_seq, scratch_bytes)) return rc;
        meta.win_off[1] = cap;
        meta.have = (u32)have;
        meta.n_seq = (u32)n_seq;
        meta.n_lit = (u32)n_lit;
        if (have) SCL_HIP_TRY(hipMemcpy(d_win.p, h_window, have, hipMemcpyHostToDevice));
        if (n_lit) SCL_HIP_TRY(hipMemcpy(d_lit.p, h_literals, n_lit, hipMemcpyHostToDevice));
        if (n_seq) {
            SCL_HIP_TRY(hipMemcpy(d_lc, h_lit_count, n_seq * 4, hipMemcpyHostToDevice));
            SCL_HIP_TRY(hipMemcpy(d_ml, h_match_len, n_seq * 4, hipMemcpyHostToDevice));
            SCL_HIP_TRY(hipMemcpy(d_mo, h_match_off, n_seq * 4, hipMemcpyHostToDevice));
        }
        SCL_HIP_TRY(hipMemcpy(d_meta.p, &meta, sizeof(meta), hipMemcpyHostToDevice));
        LzMeta *dm = (LzMeta *)d_meta.p;
        a.d_win = (u8 *)d_win.p;
        a.d_win_off = dm->win_off;
        a.d_have = &dm->have;
        a.n_streams = 1;
        a.total_bytes = cap;
        a.seq_cap = (u32)n_seq;
        a.d_lit_count = d_lc;
        a.d_match_len = d_ml;
        a.d_match_off = d_mo;
        a.d_n_seq = &dm->n_seq;
        a.d_literals = (const u8 *)d_lit.p;
        a.lit_bytes = n_lit;
        a.d_lit_off = &dm->lit_off;
        a.d_n_lit = &dm->n_lit;
        a.d_out_len = &dm->out_len;
        a.d_status = &dm->status;
        return SCL_OK;
    }

    // what a faulted stream appended in front of the fault comes back with the error: the download is first
    int replay_close(const char *what, u8 *h_window, u64 have, u64 *out_len) {
        SCL_HIP_TRY(hipDeviceSynchronize());
        SCL_HIP_TRY(hipMemcpy(&meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost));
        *out_len = meta.out_len;
        if (meta.out_len) SCL_HIP_TRY(hipMemcpy(h_window + have, (u8 *)d_win.p + have, meta.out_len, hipMemcpyDeviceToHost));
        return scl_status_to_error(meta.status, what);
    }
};

#ifdef __HIPCC__
// ---- device code shared by the one-wave kernels and the wide ones ----------------------------------------------------
__device__ __forceinline__ u32 lz_lane() { return threadIdx.x & (SCL_WAVE - 1); }

// the L-gram at global position g as a little-endian integer; the caller guarantees g + L <= N
__device__ __forceinline__ u64 lz_gram(const u8 *win, u64 g, u32 L) {
    u64 k = 0;
    for (u32 j = 0; j < L; ++j) k |= (u64)win[g + j] << (8 * j);
    return k;
}

__device__ __forceinline__ u64 lz_readlane64(u64 v, u32 lane) {
    const u32 lo = __builtin_amdgcn_readlane((int)(u32)v, (int)lane);
    const u32 hi = __builtin_amdgcn_readlane((int)(u32)(v >> 32), (int)lane);
    return ((u64)hi << 32) | lo;
}

// first set bit in [from, to) of the bitmap, or `to`: 64 words per step, one per lane (wave-uniform result)
__device__ __forceinline__ u64 lz_next_bit(const u64 *bitmap, u64 from, u64 to) {
    if (from >= to) return to;
    const u64 w_first = from >> 6, w_last = (to - 1) >> 6;
    for (u64 wb = w_first; wb <= w_last; wb += SCL_WAVE) {
        const u64 wi = wb + lz_lane();
        u64 word = wi <= w_last ? bitmap[wi] : 0ull;
        if (wi == w_first) word &= ~0ull << (from & 63);
        if (wi == w_last && (to & 63)) word &= (1ull << (to & 63)) - 1;
        const u64 hit = __ballot(word != 0);
        if (hit) {
            const u32 l = (u32)__builtin_ctzll(hit);
            return (wb + l) * 64 + (u32)__builtin_ctzll(lz_readlane64(word, l));
        }
    }
    return to;
}

__device__ __forceinline__ u64 lz_load8(const u8 *p) {
    u64 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// largest l <= limit with a[0..l) == b[0..l), given that the first `known` bytes are equal; reads stay below a + limit
// and b + limit
__device__ __forceinline__ u32 lz_extend(const u8 *a, const u8 *b, u32 known, u32 limit) {
    u32 len = known;
    while (len + 8 <= limit) {
        const u64 x = lz_load8(a + len) ^ lz_load8(b + len);
        if (x) return len + ((u32)__builtin_ctzll(x) >> 3);
        len += 8;
    }
    while (len < limit && a[len] == b[len]) ++len;
    return len;
}

// lz_extend for matches that run far: four words a step while they are all equal (the walk of the wide parse, where one
// wavefront extends a long match alone and the loads' latency is all it waits for)
__device__ __forceinline__ u32 lz_extend_far(const u8 *a, const u8 *b, u32 known, u32 limit) {
    u32 len = known;
    while (len + 32 <= limit) {
        const u64 x0 = lz_load8(a + len) ^ lz_load8(b + len), x1 = lz_load8(a + len + 8) ^ lz_load8(b + len + 8);
        const u64 x2 = lz_load8(a + len + 16) ^ lz_load8(b + len + 16), x3 = lz_load8(a + len + 24) ^ lz_load8(b + len + 24);
        if (x0 | x1 | x2 | x3) break;
        len += 32;
    }
    return lz_extend(a, b, len, limit);
}

// How lz_score spends its time; the result is the same in every mode.  PLAIN: the one-wave parse.  CAPPED: limit is small
// (at most 8 bytes a lane): the whole wave first compares the NEWEST candidate; if that one runs to the limit nothing
// beats it -- no candidate is longer, and it is the lowest lane among the equals -- and no other candidate is extended.
// FAR: lz_extend_far.
enum { LZ_SCORE_PLAIN = 0, LZ_SCORE_CAPPED = 1, LZ_SCORE_FAR = 2 };

// Scores global position gp (of the stream that starts at `base`) against its candidates, the whole wave together; all
// arguments are wave-uniform.  The newest occurrences may overlap gp (q > gp - L): at most L - 1, they come first and are
// skipped; then lane j of a group takes the j-th most recent candidate, at most M of them (0: all).  No extension reads
// more than `limit` bytes from gp or from the candidate on.  -> the longest length (0: no candidate) and *best_q, where it
// starts: the lowest lane wins ties, an older group only on strictly longer.
template <int MODE = LZ_SCORE_PLAIN>
__device__ __forceinline__ u32 lz_score(const u8 *win, u64 base, u64 gp, u32 limit, u32 L, u32 M, const u32 *order,
                                        const u32 *rank, u32 *best_q_out) {
    const u32 lane = lz_lane();
    const u32 i = rank[gp];
    const u64 key = lz_gram(win, gp, L);
    bool near = false;
    if (lane + 1 < L && lane < i) {
        const u64 c = order[i - 1 - lane];
        near = c >= base && c < gp && c + L > gp && lz_gram(win, c, L) == key;
    }
    const u32 skip = (u32)__popcll(__ballot(near));
    u32 best_len = 0, best_q = 0;
    for (u32 group = 0;; group += SCL_WAVE) {
        const u32 nth = group + lane;  // this lane scores the nth most recent candidate
        const u64 back = (u64)skip + nth;
        bool ok = back < i && (M == 0 || nth < M);
        u32 c = 0;
        if (ok) {
            c = order[i - 1 - back];
            ok = c >= base && (u64)c + L <= gp && lz_gram(win, c, L) == key;
        }
        const u64 valid = __ballot(ok);
        if (!(valid & 1ull)) break;
        if (MODE == LZ_SCORE_CAPPED && group == 0 && limit <= 8 * SCL_WAVE && (limit & 7) == 0) {
            const u32 newest = (u32)__builtin_amdgcn_readlane((int)c, 0);
            bool differs = false;
            if (lane * 8 < limit) differs = lz_load8(win + newest + lane * 8) != lz_load8(win + gp + lane * 8);
            if (!__ballot(differs)) {
                *best_q_out = newest;
                return limit;
            }
        }
        u64 score = 0;  // (length, 63 - lane): the maximum is the longest match, the lowest lane on ties
        if (ok)
            score = ((u64)(MODE == LZ_SCORE_FAR ? lz_extend_far(win + c, win + gp, L, limit)
                                                : lz_extend(win + c, win + gp, L, limit))
                     << 6) |
                    (63u - lane);
        for (u32 d = 32; d; d >>= 1) {
            const u32 lo = __shfl_xor((u32)score, d), hi = __shfl_xor((u32)(score >> 32), d);
            const u64 other = ((u64)hi << 32) | lo;
            score = other > score ? other : score;
        }
        const u32 len = (u32)(score >> 6);
        if (len > best_len) {  // an older group replaces only on strictly longer
            best_len = len;
            best_q = (u32)__builtin_amdgcn_readlane((int)c, (int)(63u - (u32)(score & 63)));
        }
        if (valid != ~0ull || (M != 0 && group + SCL_WAVE >= M)) break;
    }
    *best_q_out = best_q;
    return best_len;
}

// ---- the sliding-window coder's match rule: the one-wave parse and the wide kernels -------------
// The best match for position p of the stream at `base` (n bytes) at horizon T <= p, the lookahead starting at E <= T; all
// arguments are wave-uniform and p + hl <= n.  The entries in front of rank[p] are p's older bucket-mates, newest first;
// those at or past T come first and are skipped (at most p - T), then lane k < C takes the k-th.  A candidate more than W
// back is not scored but keeps its lane.  -> the length after both extensions (0: none), *lits_out = where the match
// starts, counted from E, *off_out = its offset.  CAPPED: no right extension reads more than `cap` bytes, and *capped
// says that a scored candidate reached the cap with bytes left in the window (the lengths are then lower bounds only;
// with *capped false every number is the uncapped call's).  FAR: lz_extend_far, for a caller whose matches run far (the same
// numbers).
template <bool CAPPED, bool FAR = false>
__device__ __forceinline__ u32 lz_sliding_best(const u8 *win, u64 N, u64 base, u32 n, u32 E, u32 p, u32 T, u32 C, u32 W,
                                               const u32 *order, const u32 *rank, const u32 *key, u32 cap, bool *capped,
                                               u32 *lits_out, u32 *off_out) {
    const u32 lane = lz_lane();
    const u64 gp = base + p, gT = base + T;
    const u32 i = rank[gp], kp = key[gp];
    if (CAPPED) *capped = false;
    if (i >= N) return 0;  // not an index of this buffer: nothing to look at
    u32 skip = 0;
    if (T < p) {
        while (true) {
            const u64 back = (u64)skip + lane;
            bool late = false;
            if (back < i) {
                const u32 c = order[i - 1 - back];
                late = c >= gT && c < gp && key[c] == kp;
            }
            const u64 mask = __ballot(late);
            if (mask != ~0ull) {
                skip += (u32)__builtin_ctzll(~mask);
                break;
            }
            skip += SCL_WAVE;
        }
    }
    const u64 back = (u64)skip + lane;
    u32 c = 0, start = p;
    u64 score = 0;  // (length, 63 - lane): the maximum is the longest match, the newest on ties
    bool ok = lane < C && back < i, reached = false;
    if (ok) {
        c = order[i - 1 - back];
        ok = c >= base && c < gT && key[c] == kp && gp - c <= W;
    }
    if (ok) {
        const u8 *w = win + base;
        u32 q = (u32)(c - base);
        const u32 limit = CAPPED && cap < n - p ? cap : n - p;
        u32 len = FAR ? lz_extend_far(win + c, win + gp, 0, limit) : lz_extend(win + c, win + gp, 0, limit);
        if (CAPPED) reached = cap < n - p && len >= cap;
        const u32 first = E > W ? E - W : 0;  // the oldest byte the coder's window still holds
        while (start > E && q > first && w[start - 1] == w[q - 1]) {
            --start;
            --q;
            ++len;
        }
        score = ((u64)len << 6) | (63u - lane);
    }
    if (CAPPED) *capped = __ballot(reached) != 0;
    for (u32 d = 32; d; d >>= 1) {
        const u32 lo = __shfl_xor((u32)score, d), hi = __shfl_xor((u32)(score >> 32), d);
        const u64 other = ((u64)hi << 32) | lo;
        score = other > score ? other : score;
    }
    const u32 best_len = (u32)(score >> 6);
    if (best_len == 0) return 0;
    const u32 winner = 63u - (u32)(score & 63);
    *lits_out = (u32)__builtin_amdgcn_readlane((int)(start - E), (int)winner);
    *off_out = (u32)__builtin_amdgcn_readlane((int)(u32)(gp - c), (int)winner);
    return best_len;
}

// ONE SEQUENCE FROM E < n: f(E) of DESIGN.md 3.6.5, the whole wave together, all arguments wave-uniform.  From E the first
// position whose best match has mml bytes or more is taken (the bitmap says where a candidate exists at all); if `lazy`,
// the positions behind it are tried at the same horizon while each beats the best so far.  -> (*lits, *len, *off); the
// next sequence starts at E + *lits + *len.  It reads E, the index and the bytes, and nothing else.
// BOUNDED (the wide parse's speculation): right extensions are capped at `cap` bytes and the search for the first match
// stops in front of position `bound`; returns true -- OPEN, the outputs mean nothing -- if any scored candidate reached
// the cap or the search reached the bound with positions left.  Returning false, every number is the unbounded call's.
// Unbounded, the return value is false.  FAR: as in lz_sliding_best (the walk of the wide parse, where one wavefront extends
// the long matches alone).
template <bool BOUNDED, bool FAR = false>
__device__ __forceinline__ bool lz_sliding_sequence(const u8 *win, u64 N, u64 base, u32 n, u32 E, u32 hl, u32 C, u32 lazy,
                                                    u32 mml, u32 W, const u32 *order, const u32 *rank, const u32 *key,
                                                    const u64 *bitmap, u32 cap, u32 bound, u32 *lits_out, u32 *len_out,
                                                    u32 *off_out) {
    u32 lits = n - E, len = 0, off = 0;  // fewer than hl bytes left: all literals
    bool open = false, capped = false;
    if (n - E >= hl) {
        const u32 stop = n - hl + 1;  // the positions [E, stop) have a whole gram
        const u32 search_end = BOUNDED && bound < stop ? bound : stop;
        lits = stop - E;
        u32 from = E;
        while (true) {
            const u64 g = lz_next_bit(bitmap, base + from, base + search_end);
            if (g >= base + search_end) {
                open = search_end < stop;
                break;
            }
            const u32 p = (u32)(g - base);
            u32 b_lits = 0, b_off = 0;
            const u32 b_len =
                lz_sliding_best<BOUNDED, FAR>(win, N, base, n, E, p, p, C, W, order, rank, key, cap, &capped, &b_lits, &b_off);
            if (BOUNDED && capped) {
                open = true;
                break;
            }
            if (b_len >= mml) {
                len = b_len;
                lits = b_lits;
                off = b_off;
                if (lazy) {  // the positions behind p, at p's horizon, while each beats the best so far
                    for (u32 pj = p + 1; pj < stop; ++pj) {
                        const u32 l = lz_sliding_best<BOUNDED, FAR>(win, N, base, n, E, pj, p, C, W, order, rank, key, cap, &capped,
                                                               &b_lits, &b_off);
                        if (BOUNDED && capped) {
                            open = true;
                            break;
                        }
                        if (l <= len) break;
                        len = l;
                        lits = b_lits;
                        off = b_off;
                    }
                }
                break;
            }
            from = p + 1;
        }
    }
    *lits_out = lits;
    *len_out = len;
    *off_out = off;
    return open;
}

// ---- the index sort's kernels, shared by the greedy index (scl_lz77.hip) and the hash-bucket index (scl_lz77_sliding.hip)
// the stream that owns global position v: the last s with win_off[s] <= v if v < win_off[s + 1], else n_streams
__device__ __forceinline__ u32 lz_stream_of(const u64 *win_off, u32 n_streams, u64 v) {
    u32 lo = 0, hi = n_streams;  // invariant: the answer, if any, is in [lo, hi)
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (win_off[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    if (n_streams == 0 || win_off[lo] > v || v >= win_off[lo + 1]) return n_streams;
    return lo;
}

// The digit source of the greedy index: passes 0..L-1 read gram byte `pass` of position v, later ones a byte of the
// stream number.  A digit source is a small struct passed by value with `u32 operator()(u32 pass, u32 v) const`.
struct LzGramDigit {
    const u8 *win;
    u64 N;
    const u64 *win_off;
    u32 n_streams, L;
    __device__ __forceinline__ u32 operator()(u32 pass, u32 v) const {
        if (pass < L) {
            const u64 g = (u64)v + pass;
            return g < N ? win[g] : 0u;
        }
        return (lz_stream_of(win_off, n_streams, v) >> (8 * (pass - L))) & 255u;
    }
};

// in == nullptr: the identity permutation (the first pass)
template <class Digit>
__global__ __launch_bounds__(LZ_SORT_THREADS) void lz77_sort_histogram(Digit digit, u64 N, u32 pass, const u32 *in,
                                                                       u32 *hist, u64 n_tiles) {
    __shared__ u32 cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const u64 first = (u64)blockIdx.x * LZ_SORT_TILE + (u64)(threadIdx.x / SCL_WAVE) * (SCL_WAVE * LZ_SORT_ROUNDS) + lz_lane();
    for (u32 r = 0; r < LZ_SORT_ROUNDS; ++r) {
        const u64 i = first + (u64)r * SCL_WAVE;
        if (i < N) atomicAdd(&cnt[digit(pass, in ? in[i] : (u32)i)], 1u);
    }
    __syncthreads();
    hist[(u64)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// ranked scatter: hist[digit * n_tiles + tile] = where this tile's first entry with that digit goes.  Inside the tile the
// waves take their digits' places in wave order, and a wave ranks its 64 entries of a round by ballots: entry -> place
// + (entries with the same digit in lower lanes).  rank_out != nullptr on the last pass: the inverse permutation.
template <class Digit>
__global__ __launch_bounds__(LZ_SORT_THREADS) void lz77_sort_scatter(Digit digit, u64 N, u32 pass, const u32 *in, u32 *out,
                                                                     u32 *rank_out, const u32 *hist, u64 n_tiles) {
    __shared__ u32 place[LZ_SORT_WAVES][256];
    const u32 wave = threadIdx.x / SCL_WAVE, lane = lz_lane();
    for (u32 w = 0; w < LZ_SORT_WAVES; ++w) place[w][threadIdx.x] = 0;
    __syncthreads();
    const u64 first = (u64)blockIdx.x * LZ_SORT_TILE + (u64)wave * (SCL_WAVE * LZ_SORT_ROUNDS) + lane;
    u32 val[LZ_SORT_ROUNDS];
    u32 dig[LZ_SORT_ROUNDS / 4] = {};  // four digits to a word
#pragma unroll
    for (u32 r = 0; r < LZ_SORT_ROUNDS; ++r) {
        const u64 i = first + (u64)r * SCL_WAVE;
        val[r] = 0;
        if (i < N) {
            val[r] = in ? in[i] : (u32)i;
            const u32 d = digit(pass, val[r]);
            dig[r / 4] |= d << (8 * (r % 4));
            atomicAdd(&place[wave][d], 1u);
        }
    }
    __syncthreads();
    {
        u32 at = hist[(u64)threadIdx.x * n_tiles + blockIdx.x];
        for (u32 w = 0; w < LZ_SORT_WAVES; ++w) {
            const u32 c = place[w][threadIdx.x];
            place[w][threadIdx.x] = at;
            at += c;
        }
    }
    __syncthreads();
    volatile u32 *mine = place[wave];
    const u64 below = (1ull << lane) - 1;
#pragma unroll
    for (u32 r = 0; r < LZ_SORT_ROUNDS; ++r) {
        const u64 i = first + (u64)r * SCL_WAVE;
        const bool live = i < N;
        const u32 d = (dig[r / 4] >> (8 * (r % 4))) & 255u;
        u64 same = __ballot(live);
#pragma unroll
        for (u32 b = 0; b < 8; ++b) {
            const u64 set = __ballot(live && ((d >> b) & 1u));
            same &= ((d >> b) & 1u) ? set : ~set;
        }
        if (live) {
            const u32 at = mine[d];
            const u32 dest = at + (u32)__popcll(same & below);
            if ((same >> lane) == 1ull) mine[d] = at + (u32)__popcll(same);  // the highest lane of the group moves the place
            out[dest] = val[r];
            if (rank_out) rank_out[val[r]] = dest;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The stable LSD sort of the N positions over `passes` digits of `digit`, on `st`: p.order_a / p.order_b ping-pong and the
// result ends in order_a, its inverse in rank.  passes >= 1.
template <class Digit>
static inline void lz77_sort_positions(Digit digit, u64 N, u32 passes, const Lz77Scratch &lay, const Lz77ScratchPtrs &p,
                                       hipStream_t st) {
    u32 *out = (passes & 1) ? p.order_a : p.order_b;
    const u32 *in = nullptr;
    for (u32 pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(lz77_sort_histogram<Digit>, dim3((u32)lay.n_tiles), dim3(LZ_SORT_THREADS), 0, st, digit, N, pass,
                           in, p.hist, lay.n_tiles);
        lz77_scan_exclusive(p.hist, lay.n_hist, p.sums, st);
        hipLaunchKernelGGL(lz77_sort_scatter<Digit>, dim3((u32)lay.n_tiles), dim3(LZ_SORT_THREADS), 0, st, digit, N, pass, in,
                           out, pass + 1 == passes ? p.rank : nullptr, p.hist, lay.n_tiles);
        in = out;
        out = out == p.order_a ? p.order_b : p.order_a;
    }
}

static inline u32 lz_stream_passes(u64 n_streams) {  // bytes of a stream number; n_streams itself marks bytes that belong to no stream
    u32 passes = 0;
    while (n_streams >> (8 * passes)) ++passes;
    return n_streams > 1 ? passes : 0;
}

// ---- replay: one wavefront appends one stream's sequences to its slot --------------------------------------------------
// A match reads bytes this same wave stored while it executed the sequences before: the release fence and the drain in
// front of every match copy order them (workgroup scope: the wave's loads and stores go through the one L1 of its CU; no
// other wave touches the stream).  `out` is deliberately neither const nor __restrict__: the reads must take the vector
// path, not the scalar cache.  out holds d bytes of cap already.  WINDOWED (the sliding-window coder): a sequence with
// match length 0 copies nothing and its offset is not looked at, and an offset above `window` (0: no bound) is
// SCL_ST_STATE.  -> the status; *d_io = the bytes in the slot afterwards.
template <bool WINDOWED>
__device__ __forceinline__ u32 lz_replay_stream(u8 *out, u32 cap, u32 *d_io, const u32 *lc, const u32 *ml, const u32 *mo,
                                                u32 n_seq, const u8 *lit, u32 n_lit, u32 window) {
    const u32 lane = lz_lane();
    u32 status = 0, d = *d_io, lp = 0;
    for (u32 k = 0; k < n_seq; ++k) {
        const u32 run = lc[k], len = ml[k], off = mo[k];
        if (run > n_lit - lp) {
            status = SCL_ST_TRUNCATED;
            break;
        }
        if (run > cap - d) {
            status = SCL_ST_CAPACITY;
            break;
        }
        for (u32 j = lane; j < run; j += SCL_WAVE) out[d + j] = lit[lp + j];
        d += run;
        lp += run;
        if (WINDOWED && len == 0) continue;
        if (off == 0 || off > d || (WINDOWED && window && off > window)) {
            status = SCL_ST_STATE;
            break;
        }
        if (len > cap - d) {
            status = SCL_ST_CAPACITY;
            break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // out[d + j] = out[d - off + (j mod off)]: every source byte was there before this sequence began
        const u8 *src = out + (d - off);
        u32 from = lane % off;
        const u32 step = SCL_WAVE % off;
        for (u32 j = lane; j < len; j += SCL_WAVE) {
            out[d + j] = src[from];
            from += step;
            if (from >= off) from -= off;
        }
        d += len;
    }
    if (status == 0) {
        const u32 rest = n_lit - lp;
        if (rest > cap - d) {
            status = SCL_ST_CAPACITY;
        } else {
            for (u32 j = lane; j < rest; j += SCL_WAVE) out[d + j] = lit[lp + j];
            d += rest;
        }
    }
    *d_io = d;
    return status;
}

// ---- the per-stream frame of the one-wave kernels ------------------------------------------------------------------------
// the stream of this wavefront (>= n_streams: none, the wave returns)
__device__ __forceinline__ u32 lz_wave_stream() { return blockIdx.x * LZ_STREAMS_PER_BLOCK + threadIdx.x / SCL_WAVE; }

// All of a replay kernel but its name: the bounds of stream s against the buffers, its rows, lz_replay_stream, the results.
template <bool WINDOWED>
__device__ __forceinline__ void lz_replay_frame(u8 *win, u64 N, const u64 *win_off, const u32 *have_in, u32 n_streams,
                                                u32 seq_cap, u32 window, const u32 *lit_count, const u32 *match_len,
                                                const u32 *match_off, const u32 *n_seq_in, const u8 *literals,
                                                u64 lit_bytes, const u64 *lit_off, const u32 *n_lit_in, u32 *out_len,
                                                u32 *status_out) {
    const u32 s = lz_wave_stream();
    if (s >= n_streams) return;
    const u32 lane = lz_lane();
    const u64 base = win_off[s], end = win_off[s + 1];
    const u32 have = have_in[s], n_seq = n_seq_in[s], n_lit = n_lit_in[s];
    const u64 l_at = lit_off[s];
    u32 status = 0, d = have;
    if (base > end || end > N || end - base >= (1ull << 32) || have > end - base || n_seq > seq_cap ||
        l_at > lit_bytes || n_lit > lit_bytes - l_at) {
        status = SCL_ST_SIZE;
    } else {
        const u32 *lc = lit_count + (u64)s * seq_cap, *ml = match_len + (u64)s * seq_cap,
                  *mo = match_off + (u64)s * seq_cap;
        status = lz_replay_stream<WINDOWED>(win + base, (u32)(end - base), &d, lc, ml, mo, n_seq, literals + l_at, n_lit,
                                            window);
    }
    if (lane == 0) {
        out_len[s] = d - have;
        status_out[s] = status;
    }
}

// Both *_replay_batch entry points: A is scl_lz77_replay_args or scl_lz77_sliding_replay_args, `kernel` the unit's own
// __global__ around lz_replay_frame, `window` the sliding one's extra kernel argument (the greedy call passes none).
template <class A, class Kernel, class... Window>
static inline int lz77_replay_launch(const char *what, const A *a, void *stream, Kernel kernel, Window... window) {
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_win_off && a->d_have && a->d_n_seq && a->d_lit_off && a->d_n_lit && a->d_out_len && a->d_status &&
                    (a->total_bytes == 0 || a->d_win) && (a->lit_bytes == 0 || a->d_literals) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->n_streams < (1ull << 32), "%s: a batch holds less than 2^32 streams", what);
    if (a->n_streams == 0) return SCL_OK;
    const u32 n_streams = (u32)a->n_streams;
    const u32 blocks = (n_streams + LZ_STREAMS_PER_BLOCK - 1) / LZ_STREAMS_PER_BLOCK;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LZ_STREAM_THREADS), 0, (hipStream_t)stream, a->d_win, a->total_bytes,
                       a->d_win_off, a->d_have, n_streams, a->seq_cap, window..., a->d_lit_count, a->d_match_len,
                       a->d_match_off, a->d_n_seq, a->d_literals, a->lit_bytes, a->d_lit_off, a->d_n_lit, a->d_out_len,
                       a->d_status);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}
#endif  // __HIPCC__
