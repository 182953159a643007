// scl_lz77_internal.h -- shapes, scratch layout and shared device code of the LZ77 kernels (scl_lz77.hip: batches, one
// wavefront per stream; scl_lz77_wide.hip: one stream across the whole GPU).  Internal to csrc/.
#pragma once

#include "scl_common.h"
#include "scl_scan.h"

// ---- the index sort: a stable LSD radix sort of the POSITIONS, 8-bit digits ------------------------------------------
// Nothing but the permutation moves: the digit of position v in gram pass d is the byte win[v + d] (0 past the buffer),
// in stream pass k byte k of v's stream number.  A tile is 4 waves x 16 rounds x 64 positions; a wave owns 1024
// consecutive entries, so tile order, wave order, round order and lane order together are the input order (stability).
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
#endif  // __HIPCC__
