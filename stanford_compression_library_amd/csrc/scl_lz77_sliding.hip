// scl_lz77_sliding.hip -- sliding-window LZ77 for gfx950: hash-bucket index, lazy parse, windowed replay.
//
//   scl_lz77_sliding_parse_batch   <->  LZ77SlidingWindowEncoder.lz77_parse_and_generate_sequences + HashBasedMatchFinder
//   scl_lz77_sliding_replay_batch  <->  LZ77SlidingWindowDecoder.execute_lz77_sequences
//                                                                          scl/compressors/lz77_sliding_window.py
//
// The batch layout is scl_lz77.hip's.  The parse call runs
//   keys  : key[v] = bucket of the hl-gram at v (LZ_NO_KEY where v has no whole gram inside its stream);
//   index : the stable radix sort of scl_lz77_internal.h by (stream, key) -> order[] and rank[]: the positions of one
//           bucket of one stream sit together, oldest first (the reference's hash_table chains, never trimmed: a chain
//           capped at C entries is the C newest of them);
//   bitmap: one bit per position: the newest older position of its bucket lies within W.  Every candidate at every
//           horizon is such a position, so a clear bit means "no match here" for the walk that looks for the first match;
//   parse : ONE WAVEFRONT PER STREAM; at p, lane k < C takes the k-th newest bucket-mate below the horizon, extends right
//           and left, and a wave maximum over (length, 63 - lane) picks the longest, the newest on ties.  The rule itself --
//           one sequence from E -- is lz_sliding_sequence of scl_lz77_internal.h, which the kernels for ONE large stream
//           (scl_lz77_sliding_wide.hip) call too; the *_host calls below choose between the two.
// No workgroup waits on another, every loop is bounded by the data, and reads and writes are checked against the buffers'
// sizes on any input.
#include "scl_lz77_internal.h"

// CPython's hash(tuple(bytes)) % m (Objects/tupleobject.c, 64-bit build; the hash of a small int is the int itself)
__host__ __device__ static inline u32 lz_sliding_bucket(const u8 *gram, u32 hl, u64 m) {
    u64 acc = 0x27D4EB2F165667C5ull;
    for (u32 j = 0; j < hl; ++j) {
        acc += (u64)gram[j] * 0xC2B2AE3D27D4EB4Full;
        acc = (acc << 31) | (acc >> 33);
        acc *= 0x9E3779B185EBCA87ull;
    }
    acc += (u64)hl ^ (0x27D4EB2F165667C5ull ^ 3527539ull);
    if (acc == ~0ull) acc = 1546275796ull;
    const i64 r = (i64)acc % (i64)m;  // Python's %: the non-negative remainder
    return (u32)(r < 0 ? r + (i64)m : r);
}

namespace {

__global__ __launch_bounds__(256) void lz77_sliding_keys(const u8 *win, u64 N, const u64 *win_off, u32 n_streams, u32 hl,
                                                         u64 m, u32 *key) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    u32 k = LZ_NO_KEY;
    const u32 s = lz_stream_of(win_off, n_streams, g);
    if (s < n_streams) {
        u64 end = win_off[s + 1];
        if (end > N) end = N;
        if (g + hl <= end) k = lz_sliding_bucket(win + g, hl, m);
    }
    key[g] = k;
}

// digit source of the bucket index: passes 0..key_passes-1 read a byte of the key, later ones a byte of the stream number
struct LzKeyDigit {
    const u32 *key;
    const u64 *win_off;
    u32 n_streams, key_passes;
    __device__ __forceinline__ u32 operator()(u32 pass, u32 v) const {
        if (pass < key_passes) return (key[v] >> (8 * pass)) & 255u;
        return (lz_stream_of(win_off, n_streams, v) >> (8 * (pass - key_passes))) & 255u;
    }
};

// bit g: the entry in front of rank[g] is an older position of g's stream and bucket, at most W back
__global__ __launch_bounds__(256) void lz77_sliding_bitmap(u64 N, const u64 *win_off, u32 n_streams, u32 W, const u32 *order,
                                                           const u32 *rank, const u32 *key, u64 *bitmap) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (g < N) {
        const u32 k = key[g], i = rank[g];
        if (k != LZ_NO_KEY && i > 0 && i < N) {
            const u32 s = lz_stream_of(win_off, n_streams, g);
            const u64 c = order[i - 1];
            bit = s < n_streams && c >= win_off[s] && c < g && g - c <= W && key[c] == k;
        }
    }
    const u64 word = __ballot(bit);
    if (lz_lane() == 0 && (g >> 6) < (N + 63) / 64) bitmap[g >> 6] = word;
}

__global__ __launch_bounds__(LZ_STREAM_THREADS) void lz77_sliding_parse(const u8 *win, u64 N, const u64 *win_off,
                                                                        const u32 *start, u32 n_streams, u32 hl, u32 C,
                                                                        u32 lazy, u32 mml, u32 W, const u32 *order,
                                                                        const u32 *rank, const u32 *key, const u64 *bitmap,
                                                                        u32 seq_cap, u32 *lit_count, u32 *match_len,
                                                                        u32 *match_off, u8 *literals, u32 *n_seq_out,
                                                                        u32 *n_lit_out, u32 *status_out) {
    const u32 s = lz_wave_stream();
    if (s >= n_streams) return;
    const u32 lane = lz_lane();
    const u64 base = win_off[s], end = win_off[s + 1];
    const u32 st = start[s];
    u32 n_seq = 0, n_lit = 0, status = 0;
    if (base > end || end > N || end - base >= (1ull << 32) || st > end - base) {
        status = SCL_ST_SIZE;
    } else {
        const u32 n = (u32)(end - base);
        const u8 *w = win + base;
        u8 *lit = literals + base + st;  // the block's own place in a buffer laid out like the windows: n - st bytes
        u32 *out_lc = lit_count + (u64)s * seq_cap, *out_ml = match_len + (u64)s * seq_cap,
            *out_mo = match_off + (u64)s * seq_cap;
        u32 E = st;
        while (E < n) {
            if (n_seq >= seq_cap) {
                status |= SCL_ST_CAPACITY;
                break;
            }
            u32 lits, len, off;  // one sequence from E: the rule itself is lz_sliding_sequence (scl_lz77_internal.h)
            (void)lz_sliding_sequence<false>(win, N, base, n, E, hl, C, lazy, mml, W, order, rank, key, bitmap, 0, 0, &lits,
                                             &len, &off);
            for (u32 k = lane; k < lits; k += SCL_WAVE) lit[n_lit + k] = w[E + k];
            if (lane == 0) {
                out_lc[n_seq] = lits;
                out_ml[n_seq] = len;
                out_mo[n_seq] = off;
            }
            n_lit += lits;
            n_seq += 1;
            E += lits + len;
        }
    }
    if (lane == 0) {
        n_seq_out[s] = n_seq;
        n_lit_out[s] = n_lit;
        status_out[s] = status;
    }
}

// lz77_replay of scl_lz77.hip with the window's two rules (lz_replay_frame<true>)
__global__ __launch_bounds__(LZ_STREAM_THREADS) void lz77_sliding_replay(u8 *win, u64 N, const u64 *win_off,
                                                                         const u32 *have_in, u32 n_streams, u32 seq_cap,
                                                                         u32 window, const u32 *lit_count,
                                                                         const u32 *match_len, const u32 *match_off,
                                                                         const u32 *n_seq_in, const u8 *literals,
                                                                         u64 lit_bytes, const u64 *lit_off,
                                                                         const u32 *n_lit_in, u32 *out_len, u32 *status_out) {
    lz_replay_frame<true>(win, N, win_off, have_in, n_streams, seq_cap, window, lit_count, match_len, match_off, n_seq_in,
                          literals, lit_bytes, lit_off, n_lit_in, out_len, status_out);
}

u32 key_passes(u64 m) {  // bytes of the largest bucket number, at least one pass
    u32 passes = 1;
    while (passes < 4 && ((m - 1) >> (8 * passes))) ++passes;
    return passes;
}

}  // namespace

extern "C" uint64_t scl_lz77_sliding_scratch_bytes(uint64_t total_bytes, uint64_t n_streams) {
    (void)n_streams;
    return sliding_scratch_layout(total_bytes).total;
}

extern "C" int scl_lz77_sliding_kernel_names(char *index, char *parse, char *replay, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_sliding_kernel_names: cap must be at least 96");
    if (index) snprintf(index, cap, "lz77_sort_scatter");
    if (parse) snprintf(parse, cap, "lz77_sliding_parse");
    if (replay) snprintf(replay, cap, "lz77_sliding_replay");
    return SCL_OK;
}

extern "C" uint32_t scl_lz77_sliding_bucket_host(const uint8_t *gram, uint32_t hl, uint32_t m) {
    if (!gram || hl < 1 || hl > 8 || m == 0) return 0;
    return lz_sliding_bucket(gram, hl, m);
}

extern "C" int scl_lz77_sliding_parse_batch(const scl_lz77_sliding_parse_args *a, void *stream) {
    const char *what = "lz77_sliding_parse_batch";
    const auto params = [&] {
        return sliding_check_params(what, a->hash_length, a->hash_table_size, a->max_chain_length, a->min_match_length);
    };
    if (int rc = lz77_parse_check(what, a, params, scl_lz77_sliding_scratch_bytes, "scl_lz77_sliding_scratch_bytes"))
        return rc;
    if (a->n_streams == 0) return SCL_OK;
    hipStream_t st = (hipStream_t)stream;
    const u64 N = a->total_bytes;
    const u32 n_streams = (u32)a->n_streams;
    const u32 W = a->window_size ? a->window_size : 0xFFFFFFFFu;
    const SlidingScratch lay = sliding_scratch_layout(N);
    const Lz77ScratchPtrs p = lz77_scratch_carve(a->d_scratch, lay.index);
    u32 *key = (u32 *)((u8 *)a->d_scratch + lay.key);
    const u32 phases = a->phases ? a->phases : 3u;
    if ((phases & SCL_LZ77_INDEX) && N) {
        const u32 blocks = (u32)((N + 255) / 256);
        hipLaunchKernelGGL(lz77_sliding_keys, dim3(blocks), dim3(256), 0, st, a->d_win, N, a->d_win_off, n_streams,
                           a->hash_length, a->hash_table_size, key);
        const u32 kp = key_passes(a->hash_table_size);
        lz77_sort_positions(LzKeyDigit{key, a->d_win_off, n_streams, kp}, N, kp + lz_stream_passes(a->n_streams), lay.index,
                            p, st);
        hipLaunchKernelGGL(lz77_sliding_bitmap, dim3(blocks), dim3(256), 0, st, N, a->d_win_off, n_streams, W, p.order_a,
                           p.rank, key, p.bitmap);
    }
    if (phases & SCL_LZ77_PARSE) {
        const u32 blocks = (n_streams + LZ_STREAMS_PER_BLOCK - 1) / LZ_STREAMS_PER_BLOCK;
        hipLaunchKernelGGL(lz77_sliding_parse, dim3(blocks), dim3(LZ_STREAM_THREADS), 0, st, a->d_win, N, a->d_win_off,
                           a->d_start, n_streams, a->hash_length, a->max_chain_length, a->lazy, a->min_match_length, W,
                           p.order_a, p.rank, key, p.bitmap, a->seq_cap, a->d_lit_count, a->d_match_len, a->d_match_off,
                           a->d_literals, a->d_n_seq, a->d_n_lit, a->d_status);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_lz77_sliding_replay_batch(const scl_lz77_sliding_replay_args *a, void *stream) {
    return lz77_replay_launch("lz77_sliding_replay_batch", a, stream, lz77_sliding_replay, a ? a->window_size : 0u);
}

// ---- one stream in host memory (LzHostFrame, scl_lz77_internal.h) -------------------------------------------------------
extern "C" int scl_lz77_sliding_parse_host(const uint8_t *h_window, uint64_t n, uint64_t start, uint32_t hash_length,
                                           uint64_t hash_table_size, uint32_t max_chain_length, uint32_t lazy,
                                           uint32_t min_match_length, uint32_t window_size, uint32_t *h_lit_count,
                                           uint32_t *h_match_len, uint32_t *h_match_off, uint64_t seq_cap, uint64_t *n_seq,
                                           uint8_t *h_literals, uint64_t lit_cap, uint64_t *n_lit) {
    const char *what = "lz77_sliding_parse_host";
    SCL_REQUIRE(n_seq && n_lit && (h_window || n == 0) && (seq_cap == 0 || (h_lit_count && h_match_len && h_match_off)) &&
                    (h_literals || lit_cap == 0),
                "%s: null pointer argument", what);
    if (int rc = sliding_check_params(what, hash_length, hash_table_size, max_chain_length, min_match_length)) return rc;
    SCL_REQUIRE(n < (1ull << 32) && start <= n && seq_cap < (1ull << 32), "%s: start <= n < 2^32 and seq_cap < 2^32", what);
    SCL_REQUIRE(lit_cap >= n - start, "%s: h_literals must hold the block (%llu bytes)", what,
                (unsigned long long)(n - start));
    // a large block goes across the whole GPU (scl_lz77_sliding_wide.hip); the results are the same either way
    const bool wide = n - start >= scl_lz77_sliding_wide_threshold();
    const u64 scratch_bytes = wide ? scl_lz77_sliding_wide_scratch_bytes(n) : scl_lz77_sliding_scratch_bytes(n, 1);
    LzHostFrame f;
    scl_lz77_sliding_parse_args a = {};
    int rc = f.parse_open(a, h_window, n, start, seq_cap, scratch_bytes);
    if (rc) return rc;
    a.hash_length = hash_length;
    a.hash_table_size = hash_table_size;
    a.max_chain_length = max_chain_length;
    a.lazy = lazy;
    a.min_match_length = min_match_length;
    a.window_size = window_size;
    if (wide) {
        scl_lz77_sliding_wide_parse_args w = {};
        w.d_win = a.d_win;
        w.n = n;
        w.start = start;
        w.hash_table_size = hash_table_size;
        w.hash_length = hash_length;
        w.max_chain_length = max_chain_length;
        w.lazy = lazy;
        w.min_match_length = min_match_length;
        w.window_size = window_size;
        w.seq_cap = a.seq_cap;
        w.d_lit_count = a.d_lit_count;
        w.d_match_len = a.d_match_len;
        w.d_match_off = a.d_match_off;
        w.d_literals = a.d_literals;
        w.d_n_seq = a.d_n_seq;
        w.d_n_lit = a.d_n_lit;
        w.d_status = a.d_status;
        w.d_scratch = a.d_scratch;
        w.scratch_bytes = scratch_bytes;
        rc = scl_lz77_sliding_parse_wide(&w, nullptr);
    } else {
        rc = scl_lz77_sliding_parse_batch(&a, nullptr);
    }
    return rc ? rc : f.parse_close(what, start, h_lit_count, h_match_len, h_match_off, n_seq, h_literals, n_lit);
}

extern "C" int scl_lz77_sliding_replay_host(uint8_t *h_window, uint64_t have, uint64_t cap, uint32_t window_size,
                                            const uint32_t *h_lit_count, const uint32_t *h_match_len,
                                            const uint32_t *h_match_off, uint64_t n_seq, const uint8_t *h_literals,
                                            uint64_t n_lit, uint64_t *out_len) {
    const char *what = "lz77_sliding_replay_host";
    SCL_REQUIRE(out_len && (h_window || cap == 0) && (n_seq == 0 || (h_lit_count && h_match_len && h_match_off)) &&
                    (h_literals || n_lit == 0),
                "%s: null pointer argument", what);
    SCL_REQUIRE(cap < (1ull << 32) && have <= cap && n_seq < (1ull << 32) && n_lit < (1ull << 32),
                "%s: have <= cap < 2^32, n_seq and n_lit < 2^32", what);
    const bool wide = cap - have >= scl_lz77_sliding_wide_threshold();  // as in scl_lz77_sliding_parse_host
    const u64 scratch_bytes = wide ? scl_lz77_wide_replay_scratch_bytes(n_seq, cap - have) : 0;
    LzHostFrame f;
    scl_lz77_sliding_replay_args a = {};
    int rc = f.replay_open(a, h_window, have, cap, h_lit_count, h_match_len, h_match_off, n_seq, h_literals, n_lit,
                           scratch_bytes);
    if (rc) return rc;
    a.window_size = window_size;
    if (wide) {
        scl_lz77_sliding_wide_replay_args w = {};
        w.d_win = a.d_win;
        w.have = have;
        w.cap = cap;
        w.d_lit_count = a.d_lit_count;
        w.d_match_len = a.d_match_len;
        w.d_match_off = a.d_match_off;
        w.n_seq = n_seq;
        w.d_literals = a.d_literals;
        w.n_lit = n_lit;
        w.d_out_len = a.d_out_len;
        w.d_status = a.d_status;
        w.d_scratch = f.d_scr.p;
        w.scratch_bytes = scratch_bytes;
        w.window_size = window_size;
        rc = scl_lz77_sliding_replay_wide(&w, nullptr);
    } else {
        rc = scl_lz77_sliding_replay_batch(&a, nullptr);
    }
    return rc ? rc : f.replay_close(what, h_window, have, out_len);
}
