// scl_lz77_sliding_wide.hip -- the parse of the sliding-window LZ77 coder for ONE large stream, across the whole GPU
// (DESIGN.md 3.6.5).
//
//   scl_lz77_sliding_parse_wide   = scl_lz77_sliding_parse_batch of a batch of one, bit for bit: sequences, literals,
//                                   counts, status
//   (scl_lz77_sliding_replay_wide = scl_lz77_sliding_replay_batch of a batch of one: the replay kernels of scl_lz77_wide.hip
//                                   with the window's two rules, its entry point stands there)
//
// The score of a position depends on where the parse stands here (the left extension runs back to E, the source bound is
// max(0, E - W), the lazy walk keeps the horizon of the first match), so positions cannot be scored one by one as in
// scl_lz77_wide.hip.  But the whole sequence from E -- (literals, length, offset), and with it the next E -- is a function
// f of E and the window alone (lz_sliding_sequence, scl_lz77_internal.h): the parse is the orbit of f from `start`, and
// two parses that ever stand at the same E are the same from there on.
//   index     : the batch call's, unchanged (key[], order[], rank[], one candidate bit per position);
//   filter    : one wavefront per bitmap word clears the candidate bits that can lead to no match under ANY E: the best
//               candidate of p, extended right and then left as far as the block goes, stays below mml bytes.  A left
//               extension only grows as E moves back, so this bound holds for every E, and a position without the bit
//               is never the first match of a sequence: the searches below read the filtered bitmap.  On bytes without
//               repeats -- where hash buckets still collide -- a search then skips 4096 positions a step;
//   speculate : one wavefront per segment of LZ_SW_SEGMENT positions follows the orbit of f from the segment's first
//               position up to the first sequence start at or past the segment's end -- its EXIT -- and stores every
//               sequence in a table addressed by its E (state DONE).  Right extensions are capped at LZ_SW_CAP bytes and
//               the search for a first match stops at the end of the next segment, so that the work of a segment grows
//               neither with a match nor with a match-free stretch; if a scored candidate reaches the cap or the search
//               its bound the position is marked OPEN, nothing else is stored for it and it is the segment's exit;
//   walk      : ONE wavefront, e = start: a DONE position lies on its segment's speculated orbit, whose members all
//               share the segment's exit: e = exit; a position the walk stored before (WALK) is followed; any other
//               position (unmarked, OPEN) is computed by lz_sliding_sequence without cap or bound -- the one-wave
//               kernel's code -- stored as WALK and followed.  entry[segment] = the first chain position in it;
//   emit      : one wavefront per segment follows the chain through the table from the segment's entry, first counting
//               (sequences, matched bytes, the last sequence start), then -- after two sum scans and one max scan over
//               the segments -- writing rows and the literal bytes THAT LIE IN ITS OWN SEGMENT: a literal run that spans
//               many segments (an incompressible block is one sequence) is copied by all of them, each finding the
//               sequence that covers its front through the max scan.
// Exact by construction: a DONE entry was computed with no extension cut and no search cut, so it equals f(E); every
// other chain position is computed by the one-wave code itself; emit reads chain positions only; by induction the chain
// through the table is the orbit of f from `start`.
// Every dependency between workgroups is a kernel boundary; no kernel waits on memory; every loop is bounded by the data;
// on any scratch contents all reads and writes stay inside the window, the rows and the literal range.
#include "scl_lz77_internal.h"

// The shape and the threshold come from profiles/lz77_sliding_wide_bench.txt.
#ifndef LZ_SW_SEGMENT
#define LZ_SW_SEGMENT 4096u
#endif
#define LZ_SW_CAP 256u
#define LZ_SW_THRESHOLD (64u << 10)
#define LZ_SW_NONE 0xFFFFFFFFu  // entry table: the chain never enters this segment

static_assert(LZ_SW_SEGMENT >= SCL_WAVE && (LZ_SW_SEGMENT & (LZ_SW_SEGMENT - 1)) == 0, "a segment is a power of two");
static_assert(LZ_SW_CAP >= 8, "a capped extension still compares whole words");

namespace {

enum : u8 { LZ_SW_DONE = 1, LZ_SW_OPEN = 2, LZ_SW_WALK = 3 };  // state[E]; anything else: nothing stored

struct SwMeta {  // the batch-of-one words the index phase reads, and the walk's status
    u64 win_off[2];
    u32 start, walk_status;
};

// Device scratch of one wide parse over n positions: the batch layout first (the index phase runs on it as it is), then
// the table and the per-segment words.  Every part starts on a 256-byte boundary.
struct SwScratch {
    SlidingScratch index;
    u64 t_lits, t_len, t_off, state, filtered, exit, entry, cnt, msum, last, sums, meta, total;
    u64 n_seg;
};

SwScratch sw_scratch_layout(u64 n) {
    SwScratch s;
    s.index = sliding_scratch_layout(n);
    s.n_seg = (n + LZ_SW_SEGMENT - 1) / LZ_SW_SEGMENT;
    SclCarver c{s.index.total};
    s.t_lits = c.take(n * 4);
    s.t_len = c.take(n * 4);
    s.t_off = c.take(n * 4);
    s.state = c.take(n);
    s.filtered = c.take(s.index.index.n_words * 8);
    s.exit = c.take(s.n_seg * 4);
    s.entry = c.take(s.n_seg * 4);
    s.cnt = c.take((s.n_seg + 1) * 4);  // one entry more than segments: the exclusive scan leaves the total there
    s.msum = c.take((s.n_seg + 1) * 4);
    s.last = c.take((s.n_seg + 1) * 4);
    s.sums = c.take(((s.n_seg + 1 + LZ_SCAN_BLOCK - 1) / LZ_SCAN_BLOCK) * 4);
    s.meta = c.take(sizeof(SwMeta));
    s.total = c.at;
    return s;
}

struct SwTable {  // the sequence table, addressed by E
    u32 *lits, *len, *off;
    u8 *state;
};

struct SwParams {
    u32 hl, C, lazy, mml, W;
};

__global__ void lz77sw_parse_init(SwMeta *meta, u64 n, u32 start) {
    meta->win_off[0] = 0;
    meta->win_off[1] = n;
    meta->start = start;
    meta->walk_status = 0;
}

// One wavefront per bitmap word from word start / 64 on: bit p of `filtered` = bit p of the bitmap, and some candidate of p at
// horizon p has mml bytes or more after its right extension and a left extension that stops only at the start of the
// block or of the window -- the most any E allows.  Writes all 64 bits of its word.
__global__ __launch_bounds__(256) void lz77sw_filter(const u8 *win, u32 n, u32 start, SwParams pr, const u32 *order,
                                                     const u32 *rank, const u32 *key, const u64 *bitmap, u64 *filtered) {
    const u32 lane = lz_lane();
    const u64 word_at = (u64)(start >> 6) + (u64)blockIdx.x * (blockDim.x / SCL_WAVE) + threadIdx.x / SCL_WAVE;
    const u64 first = word_at * 64;
    if (first >= n) return;
    u64 word = bitmap[word_at], keep = 0;
    while (word) {
        const u32 b = (u32)__builtin_ctzll(word);
        word &= word - 1;
        const u64 p64 = first + b;
        if (p64 >= n) break;  // (the bitmap has no such bit)
        const u32 p = (u32)p64, i = rank[p], kp = key[p];
        bool enough = false;
        if (i < n && lane < pr.C && lane < i) {
            const u32 c = order[i - 1 - lane];
            if (c < p && key[c] == kp && p - c <= pr.W) {
                const u32 room = n - p;
                u32 len = lz_extend(win + c, win + p, 0, pr.mml < room ? pr.mml : room);
                u32 s = p, q = c;
                while (len < pr.mml && s > start && q > 0 && win[s - 1] == win[q - 1]) {
                    --s;
                    --q;
                    ++len;
                }
                enough = len >= pr.mml;
            }
        }
        if (__ballot(enough)) keep |= 1ull << b;
    }
    if (lane == 0) filtered[word_at] = keep;
}

// One wavefront per segment: the orbit of f from the segment's first block position, capped and bounded.  state[] is all
// zero when it starts.  exit[seg] = the first orbit position at or past the segment's end, or the OPEN position inside
// the segment the orbit stops at.  Also marks the segment as not entered.
__global__ __launch_bounds__(256) void lz77sw_speculate(const u8 *win, u32 n, u32 start, SwParams pr, const u32 *order,
                                                        const u32 *rank, const u32 *key, const u64 *bitmap, SwTable t,
                                                        u32 *exit, u32 *entry, u32 n_seg) {
    const u32 lane = lz_lane();
    const u32 seg = blockIdx.x * (blockDim.x / SCL_WAVE) + threadIdx.x / SCL_WAVE;
    if (seg >= n_seg) return;
    const u64 seg_begin = (u64)seg * LZ_SW_SEGMENT, seg_stop = seg_begin + LZ_SW_SEGMENT;
    const u32 seg_end = seg_stop < n ? (u32)seg_stop : n;
    const u32 bound = seg_stop + LZ_SW_SEGMENT < n ? (u32)(seg_stop + LZ_SW_SEGMENT) : n;  // the end of the next segment
    u32 e = seg_begin > start ? (u32)seg_begin : start;
    while (e < seg_end) {
        u32 lits, len, off;
        const bool open = lz_sliding_sequence<true>(win, n, 0, n, e, pr.hl, pr.C, pr.lazy, pr.mml, pr.W, order, rank, key,
                                                    bitmap, LZ_SW_CAP, bound, &lits, &len, &off);
        if (open) {
            if (lane == 0) t.state[e] = LZ_SW_OPEN;
            break;
        }
        if (lane == 0) {
            t.lits[e] = lits;
            t.len[e] = len;
            t.off[e] = off;
            t.state[e] = LZ_SW_DONE;
        }
        const u64 next = (u64)e + lits + len;  // (lits + len >= 1, and a sequence never passes the window)
        e = next < n ? (u32)next : n;
    }
    if (lane == 0) {
        exit[seg] = e;
        entry[seg] = LZ_SW_NONE;
    }
}

// ONE wavefront: the chain from e = start.  e grows with every step.
__global__ __launch_bounds__(SCL_WAVE) void lz77sw_walk(const u8 *win, u32 n, u32 start, SwParams pr, const u32 *order,
                                                        const u32 *rank, const u32 *key, const u64 *bitmap, SwTable t,
                                                        const u32 *exit, u32 *entry, SwMeta *meta) {
    const u32 lane = lz_lane();
    u32 e = start, status = 0, in_seg = LZ_SW_NONE;
    while (e < n) {
        const u32 seg = e / LZ_SW_SEGMENT;
        if (seg != in_seg) {
            if (lane == 0) entry[seg] = e;
            in_seg = seg;
        }
        const u32 state = (u32)__builtin_amdgcn_readfirstlane((int)t.state[e]);
        u64 next;
        if (state == LZ_SW_DONE) {  // on the segment's speculated orbit: all its members leave through the same exit
            next = (u32)__builtin_amdgcn_readfirstlane((int)exit[seg]);
        } else if (state == LZ_SW_WALK) {
            const u32 lits = (u32)__builtin_amdgcn_readfirstlane((int)t.lits[e]);
            const u32 len = (u32)__builtin_amdgcn_readfirstlane((int)t.len[e]);
            next = (u64)e + lits + len;
        } else {
            u32 lits, len, off;
            (void)lz_sliding_sequence<false, true>(win, n, 0, n, e, pr.hl, pr.C, pr.lazy, pr.mml, pr.W, order, rank, key, bitmap, 0,
                                             0, &lits, &len, &off);
            if (lane == 0) {
                t.lits[e] = lits;
                t.len[e] = len;
                t.off[e] = off;
                t.state[e] = LZ_SW_WALK;
            }
            next = (u64)e + lits + len;
        }
        if (next <= e) {  // unreachable on a table of this call: a sequence has at least one byte
            status = SCL_ST_STATE;
            break;
        }
        e = next < n ? (u32)next : n;
    }
    if (lane == 0) meta->walk_status = status;
}

// One wavefront per segment follows the chain through the table from the segment's entry to the segment's end.
// WRITE = false counts: cnt = sequences that start in the segment, msum = their matched bytes, last = 1 + where the last
// of them starts (0: none).  WRITE = true, with the scans of those over the segments (cnt, msum exclusive sums; last the
// exclusive maximum: 1 + the start of the sequence that covers the segment's front), stores the rows of its sequences
// and every literal byte of its own segment: a literal at position j is literal number j - start - (bytes matched before
// j).  Row k and its literal run are stored if k < seq_cap -- what the one-wave parse leaves.
template <bool WRITE>
__global__ __launch_bounds__(256) void lz77sw_emit(const u8 *win, u32 n, u32 start, u32 n_seg, SwTable t, const u32 *entry,
                                                   u32 *cnt, u32 *msum, u32 *last, u32 seq_cap, u32 *lit_count,
                                                   u32 *match_len, u32 *match_off, u8 *literals, u32 *n_lit_out) {
    const u32 lane = lz_lane();
    const u32 seg = blockIdx.x * (blockDim.x / SCL_WAVE) + threadIdx.x / SCL_WAVE;
    if (seg > n_seg) return;
    if (seg == n_seg) {  // the entry behind the last segment: the scans leave the totals there
        if (!WRITE && lane == 0) cnt[seg] = msum[seg] = last[seg] = 0;
        return;
    }
    const u64 seg_begin = (u64)seg * LZ_SW_SEGMENT, seg_stop = seg_begin + LZ_SW_SEGMENT;
    const u32 seg_end = seg_stop < n ? (u32)seg_stop : n;
    const u32 e0 = entry[seg];
    const u32 room = n - start;  // the literal range: d_literals + start holds this many bytes
    u8 *lit = literals + start;
    u32 seqs = 0, matched = 0, last_start = 0;
    if (WRITE) {  // the front of the segment, up to its entry: the tail of the sequence that covers it
        const u32 front = seg_begin > start ? (u32)seg_begin : start;
        const u32 front_end = e0 != LZ_SW_NONE && e0 < seg_end ? e0 : seg_end;
        const u32 k = cnt[seg], cover1 = last[seg];
        if (front < front_end && k >= 1 && k - 1 < seq_cap && cover1 >= 1 && cover1 - 1 < front) {
            const u32 E = cover1 - 1;
            const u64 run_end = (u64)E + t.lits[E];
            const u32 stop = run_end < front_end ? (u32)run_end : front_end;
            const u32 before = msum[seg] - t.len[E];  // bytes matched by the sequences in front of the covering one
            for (u32 j = front + lane; j < stop; j += SCL_WAVE) {
                const u32 at = j - start - before;
                if (at < room) lit[at] = win[j];
            }
        }
    }
    if (e0 != LZ_SW_NONE && e0 >= seg_begin && e0 >= start) {
        const u32 k0 = WRITE ? cnt[seg] : 0;
        u32 before = WRITE ? msum[seg] : 0;  // bytes matched by the sequences in front of the current one
        u32 e = e0;
        while (e < seg_end) {
            const u32 state = t.state[e];
            if (state != LZ_SW_DONE && state != LZ_SW_WALK) break;  // (not a table of this call)
            const u32 lits = t.lits[e], len = t.len[e];
            const u64 next = (u64)e + lits + len;
            if (next <= e) break;  // (the same)
            if (WRITE) {
                const u32 k = k0 + seqs;
                if (k < seq_cap) {
                    if (lane == 0) {
                        lit_count[k] = lits;
                        match_len[k] = len;
                        match_off[k] = t.off[e];
                    }
                    const u64 run_end = (u64)e + lits;
                    const u32 stop = run_end < seg_end ? (u32)run_end : seg_end;
                    for (u32 j = e + lane; j < stop; j += SCL_WAVE) {
                        const u32 at = j - start - before;
                        if (at < room) lit[at] = win[j];
                    }
                } else if (k == seq_cap && lane == 0) {
                    *n_lit_out = e - start - before;  // the literals of the sequences that fit
                }
            }
            last_start = e + 1;
            seqs += 1;
            matched += len;
            before += len;
            e = next < n ? (u32)next : n;
        }
    }
    if (!WRITE && lane == 0) {
        cnt[seg] = seqs;
        msum[seg] = matched;
        last[seg] = last_start;
    }
}

// exclusive running maximum of a[0..n) in place, one workgroup
__global__ __launch_bounds__(LZ_SCAN_THREADS) void lz77sw_scan_max(u32 *a, u64 n) {
    __shared__ u32 s_wave[LZ_SCAN_THREADS / SCL_WAVE];
    (void)scl_block_scan_array<u32, LZ_SCAN_THREADS, SclScanMax>(a, n, s_wave);
}

// cnt[n_seg], msum[n_seg]: the totals.  n_lit of a block with too many sequences comes from lz77sw_emit.
__global__ void lz77sw_parse_finish(u32 n, u32 start, u32 n_seg, const u32 *cnt, const u32 *msum, u32 seq_cap,
                                    const SwMeta *meta, u32 *n_seq_out, u32 *n_lit_out, u32 *status_out) {
    const u32 total = cnt[n_seg];
    u32 status = meta->walk_status;
    if (total > seq_cap) status |= SCL_ST_CAPACITY;
    *n_seq_out = total > seq_cap ? seq_cap : total;
    if (total <= seq_cap) {
        const u32 matched = msum[n_seg];
        *n_lit_out = matched <= n - start ? n - start - matched : 0;
    }
    *status_out = status;
}

__global__ void lz77sw_parse_empty(u32 *n_seq_out, u32 *n_lit_out, u32 *status_out) {
    *n_seq_out = 0;
    *n_lit_out = 0;
    *status_out = 0;
}

}  // namespace

extern "C" void scl_lz77_sliding_wide_shape(uint32_t *segment, uint32_t *cap) {
    if (segment) *segment = LZ_SW_SEGMENT;
    if (cap) *cap = LZ_SW_CAP;
}

extern "C" uint64_t scl_lz77_sliding_wide_threshold(void) { return LZ_SW_THRESHOLD; }

extern "C" uint64_t scl_lz77_sliding_wide_scratch_bytes(uint64_t n) { return sw_scratch_layout(n).total; }

extern "C" int scl_lz77_sliding_wide_kernel_names(char *speculate, char *walk, char *emit, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_sliding_wide_kernel_names: cap must be at least 96");
    if (speculate) snprintf(speculate, cap, "lz77sw_speculate");
    if (walk) snprintf(walk, cap, "lz77sw_walk");
    if (emit) snprintf(emit, cap, "lz77sw_emit");
    return SCL_OK;
}

extern "C" int scl_lz77_sliding_parse_wide(const scl_lz77_sliding_wide_parse_args *a, void *stream) {
    const char *what = "lz77_sliding_parse_wide";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_n_seq && a->d_n_lit && a->d_status && a->d_scratch && (a->n == 0 || (a->d_win && a->d_literals)) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    if (int rc = sliding_check_params(what, a->hash_length, a->hash_table_size, a->max_chain_length, a->min_match_length))
        return rc;
    SCL_REQUIRE(a->n < (1ull << 32) && a->start <= a->n, "%s: start <= n < 2^32", what);
    SCL_REQUIRE(a->phases <= 15, "%s: phases is a mask of SCL_LZ77_SLIDING_WIDE_INDEX | _SPECULATE | _WALK | _EMIT", what);
    const SwScratch lay = sw_scratch_layout(a->n);
    SCL_REQUIRE(((uintptr_t)a->d_scratch & 255) == 0 && a->scratch_bytes >= lay.total,
                "%s: d_scratch must be 256-byte aligned and hold scl_lz77_sliding_wide_scratch_bytes = %llu bytes", what,
                (unsigned long long)lay.total);
    hipStream_t st = (hipStream_t)stream;
    if (a->start == a->n) {
        hipLaunchKernelGGL(lz77sw_parse_empty, dim3(1), dim3(1), 0, st, a->d_n_seq, a->d_n_lit, a->d_status);
        SCL_HIP_TRY(hipGetLastError());
        return SCL_OK;
    }
    const u32 n = (u32)a->n, start = (u32)a->start, n_seg = (u32)lay.n_seg;
    const SwParams pr = {a->hash_length, a->max_chain_length, a->lazy, a->min_match_length,
                         a->window_size ? a->window_size : 0xFFFFFFFFu};
    u8 *scr = (u8 *)a->d_scratch;
    SwMeta *meta = (SwMeta *)(scr + lay.meta);
    const u32 *order = (const u32 *)(scr + lay.index.index.order_a), *rank = (const u32 *)(scr + lay.index.index.rank);
    const u32 *key = (const u32 *)(scr + lay.index.key);
    const u64 *candidates = (const u64 *)(scr + lay.index.index.bitmap);
    u64 *bitmap = (u64 *)(scr + lay.filtered);  // what the searches read: the candidate bits that can lead to a match
    const SwTable t = {(u32 *)(scr + lay.t_lits), (u32 *)(scr + lay.t_len), (u32 *)(scr + lay.t_off), scr + lay.state};
    u32 *exit = (u32 *)(scr + lay.exit), *entry = (u32 *)(scr + lay.entry), *cnt = (u32 *)(scr + lay.cnt);
    u32 *msum = (u32 *)(scr + lay.msum), *last = (u32 *)(scr + lay.last), *sums = (u32 *)(scr + lay.sums);

    const u32 phases = a->phases ? a->phases : 15u;
    if (phases & SCL_LZ77_SLIDING_WIDE_INDEX) {
        hipLaunchKernelGGL(lz77sw_parse_init, dim3(1), dim3(1), 0, st, meta, a->n, start);
        scl_lz77_sliding_parse_args ix = {};  // the index phase of a batch of one, on the front of the scratch
        ix.d_win = a->d_win;
        ix.d_win_off = meta->win_off;
        ix.d_start = &meta->start;
        ix.n_streams = 1;
        ix.total_bytes = a->n;
        ix.hash_table_size = a->hash_table_size;
        ix.hash_length = a->hash_length;
        ix.max_chain_length = a->max_chain_length;
        ix.lazy = a->lazy;
        ix.min_match_length = a->min_match_length;
        ix.window_size = a->window_size;
        ix.phases = SCL_LZ77_INDEX;
        ix.d_literals = a->d_literals;
        ix.d_n_seq = a->d_n_seq;
        ix.d_n_lit = a->d_n_lit;
        ix.d_status = a->d_status;
        ix.d_scratch = a->d_scratch;
        ix.scratch_bytes = lay.index.total;
        const int rc = scl_lz77_sliding_parse_batch(&ix, stream);
        if (rc) return rc;
    }
    const u32 seg_blocks = (n_seg + 3) / 4;
    if (phases & SCL_LZ77_SLIDING_WIDE_SPECULATE) {
        SCL_HIP_TRY(hipMemsetAsync(t.state, 0, n, st));
        const u32 words = (u32)(((u64)n + 63) / 64 - start / 64);
        hipLaunchKernelGGL(lz77sw_filter, dim3((words + 3) / 4), dim3(256), 0, st, a->d_win, n, start, pr, order, rank, key,
                           candidates, bitmap);
        hipLaunchKernelGGL(lz77sw_speculate, dim3(seg_blocks), dim3(256), 0, st, a->d_win, n, start, pr, order, rank, key,
                           bitmap, t, exit, entry, n_seg);
    }
    if (phases & SCL_LZ77_SLIDING_WIDE_WALK)
        hipLaunchKernelGGL(lz77sw_walk, dim3(1), dim3(SCL_WAVE), 0, st, a->d_win, n, start, pr, order, rank, key, bitmap, t,
                           exit, entry, meta);
    if (phases & SCL_LZ77_SLIDING_WIDE_EMIT) {
        const u32 emit_blocks = (u32)(((u64)n_seg + 1 + 3) / 4);
        hipLaunchKernelGGL(lz77sw_emit<false>, dim3(emit_blocks), dim3(256), 0, st, a->d_win, n, start, n_seg, t, entry, cnt,
                           msum, last, a->seq_cap, a->d_lit_count, a->d_match_len, a->d_match_off, a->d_literals, a->d_n_lit);
        lz77_scan_exclusive(cnt, (u64)n_seg + 1, sums, st);
        lz77_scan_exclusive(msum, (u64)n_seg + 1, sums, st);
        hipLaunchKernelGGL(lz77sw_scan_max, dim3(1), dim3(LZ_SCAN_THREADS), 0, st, last, (u64)n_seg + 1);
        hipLaunchKernelGGL(lz77sw_parse_finish, dim3(1), dim3(1), 0, st, n, start, n_seg, cnt, msum, a->seq_cap, meta,
                           a->d_n_seq, a->d_n_lit, a->d_status);
        hipLaunchKernelGGL(lz77sw_emit<true>, dim3(emit_blocks), dim3(256), 0, st, a->d_win, n, start, n_seg, t, entry, cnt,
                           msum, last, a->seq_cap, a->d_lit_count, a->d_match_len, a->d_match_off, a->d_literals, a->d_n_lit);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}
