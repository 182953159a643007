// scl_lz77.hip -- the LZ layer of LZ77 for gfx950: match index, greedy parse, sequence replay.
//
//   scl_lz77_parse_batch   <->  LZ77Encoder.lz77_parse_and_generate_sequences   scl/compressors/lz77.py:525-603
//   scl_lz77_replay_batch  <->  LZ77Decoder.execute_lz77_sequences              scl/compressors/lz77.py:640-665
//
// A batch is n_streams windows back to back in one buffer of N bytes.  The parse call runs
//   index : a stable LSD radix sort of all N positions by (stream, L-gram) -> order[] and its inverse rank[]: the
//           occurrences of one gram of one stream sit together, oldest first (the reference's substring_dict lists);
//   bitmap: one bit per position: it has a candidate (an equal gram at q <= p - L) -- parallel over positions;
//   parse : ONE WAVEFRONT PER STREAM walks the stream: skip to the next set bit (4096 positions per step), score the
//           candidates 64 at a time (lane j = the j-th most recent), longest wins, lowest lane on ties.
// One LARGE stream has kernels of its own, scl_lz77_wide.hip; the *_host calls below choose.  The device code they share --
// and share with the sliding-window coder, scl_lz77_sliding.hip: the sort's histogram and scatter kernels, templates on
// the digit source, the replay kernels' body, the entry points' checks and the frame of the *_host calls -- is in
// scl_lz77_internal.h; the scans of the sort are here, behind lz77_scan_exclusive.
// No workgroup waits on another (every dependency between workgroups is a kernel boundary), every loop is bounded by the
// data, and reads and writes are checked against the buffers' sizes on any input.
#include "scl_lz77_internal.h"

namespace {

// the scan of the tile histograms in three kernels: every block scans its 2048 entries, one workgroup scans the block
// sums, every block adds its offset (the scans across a workgroup: scl_scan.h)
template <class V>
__global__ __launch_bounds__(LZ_SCAN_THREADS) void lz77_scan_blocks(V *hist, u64 n, V *block_sums) {
    __shared__ V s_wave[LZ_SCAN_THREADS / SCL_WAVE];
    const u64 at = ((u64)blockIdx.x * LZ_SCAN_THREADS + threadIdx.x) * LZ_SCAN_PER_THREAD;
    V v[LZ_SCAN_PER_THREAD], sum = 0;
#pragma unroll
    for (u32 j = 0; j < LZ_SCAN_PER_THREAD; ++j) {
        v[j] = at + j < n ? hist[at + j] : V(0);
        sum += v[j];
    }
    V total;
    V run = scl_block_scan_excl<V, LZ_SCAN_THREADS, SclScanSum>(sum, s_wave, &total);
#pragma unroll
    for (u32 j = 0; j < LZ_SCAN_PER_THREAD; ++j) {
        if (at + j < n) hist[at + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

template <class V>
__global__ __launch_bounds__(LZ_SCAN_THREADS) void lz77_scan_block_sums(V *block_sums, u64 n) {
    __shared__ V s_wave[LZ_SCAN_THREADS / SCL_WAVE];
    (void)scl_block_scan_array<V, LZ_SCAN_THREADS, SclScanSum>(block_sums, n, s_wave);
}

template <class V>
__global__ __launch_bounds__(LZ_SCAN_THREADS) void lz77_scan_add(V *hist, u64 n, const V *block_sums) {
    const u64 at = ((u64)blockIdx.x * LZ_SCAN_THREADS + threadIdx.x) * LZ_SCAN_PER_THREAD;
    const V add = block_sums[blockIdx.x];
#pragma unroll
    for (u32 j = 0; j < LZ_SCAN_PER_THREAD; ++j)
        if (at + j < n) hist[at + j] += add;
}

// ---- candidate bitmap ------------------------------------------------------------------------------------------------
// bit g: position g of its stream has a candidate.  Predecessors of g in order[] with g's (stream, gram) are earlier
// occurrences, newest first; at most L - 1 of them overlap g (q > p - L), so L looks decide.
__global__ __launch_bounds__(256) void lz77_candidate_bitmap(const u8 *win, u64 N, const u64 *win_off, u32 n_streams,
                                                             u32 L, const u32 *order, const u32 *rank, u64 *bitmap) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (g < N) {
        const u32 s = lz_stream_of(win_off, n_streams, g);
        if (s < n_streams) {
            const u64 base = win_off[s];
            u64 end = win_off[s + 1];
            if (end > N) end = N;
            if (g + L <= end) {
                const u32 i = rank[g];
                const u64 key = lz_gram(win, g, L);
                for (u32 k = 1; k <= L && k <= i; ++k) {
                    const u64 c = order[i - k];
                    if (c < base || c >= g || lz_gram(win, c, L) != key) break;
                    if (c + L <= g) {
                        bit = true;
                        break;
                    }
                }
            }
        }
    }
    const u64 word = __ballot(bit);
    if (lz_lane() == 0 && (g >> 6) < (N + 63) / 64) bitmap[g >> 6] = word;
}

// ---- parse -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LZ_STREAM_THREADS) void lz77_parse(const u8 *win, u64 N, const u64 *win_off,
                                                                const u32 *start, u32 n_streams, u32 L, u32 M,
                                                                const u32 *order, const u32 *rank, const u64 *bitmap,
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
        const u64 g_stop = n >= L ? base + (n - L) + 1 : base;  // positions at or past it have no whole gram
        u32 pos = st;
        while (true) {
            const u64 gp = lz_next_bit(bitmap, base + pos, g_stop);
            if (gp >= g_stop) break;
            const u32 p = (u32)(gp - base);
            u32 best_q;
            const u32 best_len = lz_score(win, base, gp, n - p, L, M, order, rank, &best_q);
            if (best_len == 0) {  // the bitmap promised a candidate: unreachable, and never a reason to spin
                status |= SCL_ST_STATE;
                break;
            }
            if (n_seq >= seq_cap) {
                status |= SCL_ST_CAPACITY;
                break;
            }
            const u32 run = p - pos;
            for (u32 k = lane; k < run; k += SCL_WAVE) lit[n_lit + k] = w[pos + k];
            if (lane == 0) {
                out_lc[n_seq] = run;
                out_ml[n_seq] = best_len;
                out_mo[n_seq] = (u32)(gp - best_q);
            }
            n_lit += run;
            n_seq += 1;
            pos = p + best_len;
        }
        if (status == 0) {
            const u32 run = n - pos;
            for (u32 k = lane; k < run; k += SCL_WAVE) lit[n_lit + k] = w[pos + k];
            n_lit += run;
        }
    }
    if (lane == 0) {
        n_seq_out[s] = n_seq;
        n_lit_out[s] = n_lit;
        status_out[s] = status;
    }
}

// ---- replay ----------------------------------------------------------------------------------------------------------
// One wavefront per stream appends to the stream's window: lz_replay_frame (scl_lz77_internal.h).  `win` is deliberately
// neither const nor __restrict__, see lz_replay_stream there.
__global__ __launch_bounds__(LZ_STREAM_THREADS) void lz77_replay(u8 *win, u64 N, const u64 *win_off, const u32 *have_in,
                                                                 u32 n_streams, u32 seq_cap, const u32 *lit_count,
                                                                 const u32 *match_len, const u32 *match_off,
                                                                 const u32 *n_seq_in, const u8 *literals, u64 lit_bytes,
                                                                 const u64 *lit_off, const u32 *n_lit_in, u32 *out_len,
                                                                 u32 *status_out) {
    lz_replay_frame<false>(win, N, win_off, have_in, n_streams, seq_cap, 0, lit_count, match_len, match_off, n_seq_in,
                           literals, lit_bytes, lit_off, n_lit_in, out_len, status_out);
}

}  // namespace

template <class V>
void lz77_scan_exclusive(V *data, u64 n, V *block_sums, hipStream_t st) {
    const u32 blocks = (u32)((n + LZ_SCAN_BLOCK - 1) / LZ_SCAN_BLOCK);
    if (!blocks) return;
    hipLaunchKernelGGL(lz77_scan_blocks<V>, dim3(blocks), dim3(LZ_SCAN_THREADS), 0, st, data, n, block_sums);
    hipLaunchKernelGGL(lz77_scan_block_sums<V>, dim3(1), dim3(LZ_SCAN_THREADS), 0, st, block_sums, (u64)blocks);
    hipLaunchKernelGGL(lz77_scan_add<V>, dim3(blocks), dim3(LZ_SCAN_THREADS), 0, st, data, n, (const V *)block_sums);
}
template void lz77_scan_exclusive<u32>(u32 *, u64, u32 *, hipStream_t);
template void lz77_scan_exclusive<u64>(u64 *, u64, u64 *, hipStream_t);

extern "C" uint64_t scl_lz77_scratch_bytes(uint64_t total_bytes, uint64_t n_streams) {
    (void)n_streams;
    return lz77_scratch_layout(total_bytes).total;
}

extern "C" int scl_lz77_kernel_names(char *index, char *parse, char *replay, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_kernel_names: cap must be at least 96");
    if (index) snprintf(index, cap, "lz77_sort_scatter");
    if (parse) snprintf(parse, cap, "lz77_parse");
    if (replay) snprintf(replay, cap, "lz77_replay");
    return SCL_OK;
}

extern "C" int scl_lz77_parse_batch(const scl_lz77_parse_args *a, void *stream) {
    const char *what = "lz77_parse_batch";
    const auto params = [&]() -> int {
        SCL_REQUIRE(a->min_match_length >= 1 && a->min_match_length <= 8,
                    "%s: min_match_length %u: an L-gram is one 64-bit key, 1 <= L <= 8", what, a->min_match_length);
        return SCL_OK;
    };
    if (int rc = lz77_parse_check(what, a, params, scl_lz77_scratch_bytes, "scl_lz77_scratch_bytes")) return rc;
    if (a->n_streams == 0) return SCL_OK;
    hipStream_t st = (hipStream_t)stream;
    const u64 N = a->total_bytes;
    const u32 L = a->min_match_length, n_streams = (u32)a->n_streams;
    const Lz77Scratch lay = lz77_scratch_layout(N);
    const Lz77ScratchPtrs p = lz77_scratch_carve(a->d_scratch, lay);
    const u32 phases = a->phases ? a->phases : 3u;
    const u32 passes = L + lz_stream_passes(a->n_streams);
    if ((phases & SCL_LZ77_INDEX) && N) {
        lz77_sort_positions(LzGramDigit{a->d_win, N, a->d_win_off, n_streams, L}, N, passes, lay, p, st);
        hipLaunchKernelGGL(lz77_candidate_bitmap, dim3((u32)((N + 255) / 256)), dim3(256), 0, st, a->d_win, N,
                           a->d_win_off, n_streams, L, p.order_a, p.rank, p.bitmap);
    }
    if (phases & SCL_LZ77_PARSE) {
        const u32 blocks = (n_streams + LZ_STREAMS_PER_BLOCK - 1) / LZ_STREAMS_PER_BLOCK;
        hipLaunchKernelGGL(lz77_parse, dim3(blocks), dim3(LZ_STREAM_THREADS), 0, st, a->d_win, N, a->d_win_off,
                           a->d_start, n_streams, L, a->max_matches, p.order_a, p.rank, p.bitmap, a->seq_cap,
                           a->d_lit_count, a->d_match_len, a->d_match_off, a->d_literals, a->d_n_seq, a->d_n_lit,
                           a->d_status);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_lz77_replay_batch(const scl_lz77_replay_args *a, void *stream) {
    return lz77_replay_launch("lz77_replay_batch", a, stream, lz77_replay);  // `reserved` is not a window: none is passed
}

// ---- one stream in host memory (LzHostFrame, scl_lz77_internal.h) -------------------------------------------------------
extern "C" int scl_lz77_parse_host(const uint8_t *h_window, uint64_t n, uint64_t start, uint32_t min_match_length,
                                   uint32_t max_matches, uint32_t *h_lit_count, uint32_t *h_match_len,
                                   uint32_t *h_match_off, uint64_t seq_cap, uint64_t *n_seq, uint8_t *h_literals,
                                   uint64_t lit_cap, uint64_t *n_lit) {
    const char *what = "lz77_parse_host";
    SCL_REQUIRE(n_seq && n_lit && (h_window || n == 0) && (seq_cap == 0 || (h_lit_count && h_match_len && h_match_off)) &&
                    (h_literals || lit_cap == 0),
                "%s: null pointer argument", what);
    SCL_REQUIRE(min_match_length >= 1 && min_match_length <= 8,
                "%s: min_match_length %u: an L-gram is one 64-bit key, 1 <= L <= 8", what, min_match_length);
    SCL_REQUIRE(n < (1ull << 32) && start <= n && seq_cap < (1ull << 32), "%s: start <= n < 2^32 and seq_cap < 2^32", what);
    SCL_REQUIRE(lit_cap >= n - start, "%s: h_literals must hold the block (%llu bytes)", what,
                (unsigned long long)(n - start));
    // a large block goes across the whole GPU (scl_lz77_wide.hip); the results are the same either way
    const bool wide = n - start >= scl_lz77_wide_threshold() && max_matches >= 1 && max_matches <= 64;
    const u64 scratch_bytes = wide ? scl_lz77_wide_scratch_bytes(n) : scl_lz77_scratch_bytes(n, 1);
    LzHostFrame f;
    scl_lz77_parse_args a = {};
    int rc = f.parse_open(a, h_window, n, start, seq_cap, scratch_bytes);
    if (rc) return rc;
    a.min_match_length = min_match_length;
    a.max_matches = max_matches;
    if (wide) {
        scl_lz77_wide_parse_args w = {};
        w.d_win = a.d_win;
        w.n = n;
        w.start = start;
        w.min_match_length = min_match_length;
        w.max_matches = max_matches;
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
        rc = scl_lz77_parse_wide(&w, nullptr);
    } else {
        rc = scl_lz77_parse_batch(&a, nullptr);
    }
    return rc ? rc : f.parse_close(what, start, h_lit_count, h_match_len, h_match_off, n_seq, h_literals, n_lit);
}

extern "C" int scl_lz77_replay_host(uint8_t *h_window, uint64_t have, uint64_t cap, const uint32_t *h_lit_count,
                                    const uint32_t *h_match_len, const uint32_t *h_match_off, uint64_t n_seq,
                                    const uint8_t *h_literals, uint64_t n_lit, uint64_t *out_len) {
    const char *what = "lz77_replay_host";
    SCL_REQUIRE(out_len && (h_window || cap == 0) && (n_seq == 0 || (h_lit_count && h_match_len && h_match_off)) &&
                    (h_literals || n_lit == 0),
                "%s: null pointer argument", what);
    SCL_REQUIRE(cap < (1ull << 32) && have <= cap && n_seq < (1ull << 32) && n_lit < (1ull << 32),
                "%s: have <= cap < 2^32, n_seq and n_lit < 2^32", what);
    const bool wide = cap - have >= scl_lz77_wide_threshold();  // as in scl_lz77_parse_host
    const u64 scratch_bytes = wide ? scl_lz77_wide_replay_scratch_bytes(n_seq, cap - have) : 0;
    LzHostFrame f;
    scl_lz77_replay_args a = {};
    int rc = f.replay_open(a, h_window, have, cap, h_lit_count, h_match_len, h_match_off, n_seq, h_literals, n_lit,
                           scratch_bytes);
    if (rc) return rc;
    if (wide) {
        scl_lz77_wide_replay_args w = {};
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
        rc = scl_lz77_replay_wide(&w, nullptr);
    } else {
        rc = scl_lz77_replay_batch(&a, nullptr);
    }
    return rc ? rc : f.replay_close(what, h_window, have, out_len);
}
