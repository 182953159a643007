// scl_lz77_internal.h -- shapes and scratch layout of the LZ77 kernels (scl_lz77.hip).  Internal to csrc/.
#pragma once

#include "scl_common.h"

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
    u64 at = 0;
    auto take = [&](u64 bytes) {
        const u64 here = at;
        at += scl_round_up(bytes ? bytes : 1, 256);
        return here;
    };
    s.order_a = take(N * 4);
    s.order_b = take(N * 4);
    s.rank = take(N * 4);
    s.bitmap = take(s.n_words * 8);
    s.hist = take(s.n_hist * 4);
    s.block_sums = take(s.n_scan_blocks * 4);
    s.total = at;
    return s;
}
