// scl_lz77_wide.hip -- the LZ layer of LZ77 for ONE large stream, across the whole GPU ("One stream, wide").
//
//   scl_lz77_parse_wide   = scl_lz77_parse_batch  of a batch of one, bit for bit: sequences, literals, counts, status
//   scl_lz77_replay_wide  = scl_lz77_replay_batch of a batch of one, bit for bit: bytes, out_len, status
//
// Parse.  The score of a position p -- (best_len, best_q) -- depends on p and the window alone, not on where the parse
// stands, so every position is scored in parallel and the greedy chain pos -> p -> p + best_len is followed through a
// table:
//   index : the batch call's, unchanged (order[], rank[], one candidate bit per position);
//   score : one wavefront per bitmap word scores its set bits with lz_score, extensions capped at LZ_WIDE_CAP bytes.  Below
//           the cap the result is exact; at the cap the position is LONG and nothing else is stored.  The newest candidate
//           is compared first, by the whole wave: where it reaches the cap (repetitive data) nothing else is extended;
//   exits : per tile of LZ_WIDE_TILE positions, where the chain that enters at p leaves the tile (pointer jumping in LDS):
//           the first chain position >= tile end, or the LONG position inside the tile it stops at;
//   walk  : ONE wavefront goes tile to tile: entry[tile] = e, e = exit[e]; a LONG stop x is scored in full (lz_score
//           without a cap), the exact (len, q) goes into the table and e = x + len.  LZ_WIDE_CAP >= LZ_WIDE_TILE, so a
//           resolved long match leaves its tile: every tile is entered at most once, and e grows with every step;
//   emit  : one wavefront per entered tile follows its chain, first counting (sequences, matched bytes, last match end),
//           then -- after two sum scans and one max scan over the tiles -- writing rows and literal bytes.
// Replay.  64-bit prefix sums of literal_count and literal_count + match_length place every sequence; every sequence is
// validated from them in the one-wave kernel's order of checks, the first fault found by a minimum; literal bytes are
// written at once, a match byte gets root = the earlier byte it copies, root = root[root] is iterated (each hop lands in a
// strictly earlier sequence), and one gather finishes.
// Every dependency between workgroups is a kernel boundary; no kernel waits on memory; every loop is bounded by the data.
#include "scl_lz77_internal.h"

// The shape and the threshold come from profiles/lz77_bench.txt: at tile = cap = 512 the walk is 30 % of
// the parse of a 16 MiB Markov stream; 64 KiB is the smallest measured size from which both wide calls are faster than
// the one-wave kernels at every larger measured size, on the Markov source and on all-equal bytes.
#define LZ_WIDE_TILE 512u
#define LZ_WIDE_CAP 512u
#define LZ_WIDE_THRESHOLD (64u << 10)
#define LZ_WIDE_LONG 0xFFFFFFFFu  // score table: an extension reached the cap
#define LZ_WIDE_NONE 0xFFFFFFFFu  // entry table: the chain never enters this tile
#define LZ_WIDE_ROUND_FLAGS 40    // more than ceil(log2(2^32 + 1)) + 1 rounds are never launched

static_assert(LZ_WIDE_TILE <= LZ_WIDE_CAP && (LZ_WIDE_TILE & (LZ_WIDE_TILE - 1)) == 0 && (LZ_WIDE_CAP & (LZ_WIDE_CAP - 1)) == 0,
              "tile <= cap, both powers of two");
static_assert(LZ_WIDE_TILE >= SCL_WAVE && LZ_WIDE_TILE <= 1024, "one thread per position of a tile");
static_assert(LZ_WIDE_CAP <= 8 * SCL_WAVE, "LZ_SCORE_CAPPED compares the newest candidate in one step up to 8 bytes a lane");

namespace {

struct WideMeta {  // the batch-of-one words the index phase reads, and the walk's status
    u64 win_off[2];
    u32 start, walk_status;
};

// Device scratch of one wide parse over n positions: the batch layout first (the index phase runs on it as it is), then
// the tables.  Every part starts on a 256-byte boundary.
struct WideScratch {
    Lz77Scratch index;
    u64 slen, sq, exit, entry, cnt, msum, lend, sums, meta, total;
    u64 n_tiles;
};

WideScratch wide_scratch_layout(u64 n) {
    WideScratch s;
    s.index = lz77_scratch_layout(n);
    s.n_tiles = (n + LZ_WIDE_TILE - 1) / LZ_WIDE_TILE;
    SclCarver c{s.index.total};
    s.slen = c.take(n * 4);
    s.sq = c.take(n * 4);
    s.exit = c.take(n * 4);
    s.entry = c.take(s.n_tiles * 4);
    s.cnt = c.take((s.n_tiles + 1) * 4);  // one entry more than tiles: the exclusive scan leaves the total there
    s.msum = c.take((s.n_tiles + 1) * 4);
    s.lend = c.take((s.n_tiles + 1) * 4);
    s.sums = c.take(((s.n_tiles + 1 + LZ_SCAN_BLOCK - 1) / LZ_SCAN_BLOCK) * 4);
    s.meta = c.take(sizeof(WideMeta));
    s.total = c.at;
    return s;
}

struct ReplayMeta {
    u32 first;    // the first faulting sequence, n_seq without one
    u32 status;
    u64 out_end;  // the slot holds [0, out_end) afterwards
    u32 changed[LZ_WIDE_ROUND_FLAGS];  // changed[r]: round r has work (round r - 1 moved a root)
};

struct ReplayScratch {
    u64 lit_sum, all_sum, sums, root, meta, total;
};

ReplayScratch replay_scratch_layout(u64 n_seq, u64 grow) {
    ReplayScratch s;
    SclCarver c;
    s.lit_sum = c.take((n_seq + 1) * 8);
    s.all_sum = c.take((n_seq + 1) * 8);
    s.sums = c.take(((n_seq + 1 + LZ_SCAN_BLOCK - 1) / LZ_SCAN_BLOCK) * 8);
    s.root = c.take(grow * 4);
    s.meta = c.take(sizeof(ReplayMeta));
    s.total = c.at;
    return s;
}

// ---- parse -----------------------------------------------------------------------------------------------------------
__global__ void lz77w_parse_init(WideMeta *meta, u64 n, u32 start) {
    meta->win_off[0] = 0;
    meta->win_off[1] = n;
    meta->start = start;
    meta->walk_status = 0;
}

// One wavefront per bitmap word from word start / 64 on: slen[p] = 0 (no candidate: a literal step), the exact length
// below the cap with sq[p] = where the match starts, or LZ_WIDE_LONG.  Writes slen for all 64 positions of its word.
__global__ __launch_bounds__(256) void lz77w_score(const u8 *win, u32 n, u32 start, u32 L, u32 M, const u32 *order,
                                                   const u32 *rank, const u64 *bitmap, u32 *slen, u32 *sq) {
    const u32 lane = lz_lane();
    const u64 word_at = (u64)(start >> 6) + (u64)blockIdx.x * (blockDim.x / SCL_WAVE) + threadIdx.x / SCL_WAVE;
    const u64 first = word_at * 64;
    if (first >= n) return;
    u64 word = bitmap[word_at];
    if (first < start) word &= ~0ull << (start - first);
    u32 my_len = 0, my_q = 0;
    while (word) {
        const u32 b = (u32)__builtin_ctzll(word);
        word &= word - 1;
        const u32 p = (u32)first + b;
        if (p >= n) break;  // (the bitmap has no such bit)
        const u32 room = n - p;
        u32 q;
        const u32 len = lz_score<LZ_SCORE_CAPPED>(win, 0, p, room < LZ_WIDE_CAP ? room : LZ_WIDE_CAP, L, M, order, rank, &q);
        if (lane == b) {
            my_len = len >= LZ_WIDE_CAP ? LZ_WIDE_LONG : len;
            my_q = q;
        }
    }
    const u64 p = first + lane;
    if (p < n) {
        slen[p] = my_len;
        sq[p] = my_q;
    }
}

// One workgroup per tile, one thread per position.  jump[p] = p for a position that ends a walk inside the tile (LONG, or
// outside the block), else the next chain position; after log2(tile) doublings jump[p] is where the chain from p leaves
// the tile or stops.  Also marks the tile as not entered.
__global__ __launch_bounds__(LZ_WIDE_TILE) void lz77w_tile_exits(u32 n, u32 start, const u32 *slen, u32 *exit, u32 *entry) {
    __shared__ u32 jump[LZ_WIDE_TILE];
    const u32 t = threadIdx.x;
    const u64 tile_begin = (u64)blockIdx.x * LZ_WIDE_TILE, tile_end = tile_begin + LZ_WIDE_TILE;
    if (t == 0) entry[blockIdx.x] = LZ_WIDE_NONE;
    if (tile_end <= start) return;  // (the whole workgroup)
    const u64 p = tile_begin + t;
    u64 to = p < n ? p : n;  // (positions past the window: n, which ends every walk)
    if (p >= start && p < n) {
        const u32 len = slen[p];
        if (len != LZ_WIDE_LONG) {
            to = p + (len ? len : 1u);
            if (to > n) to = n;  // (a match never passes the window)
        }
    }
    jump[t] = (u32)to;  // to <= n < 2^32
    __syncthreads();
    for (u32 d = 1; d < LZ_WIDE_TILE; d <<= 1) {
        const u32 v = jump[t];
        u32 next = v;
        if (v != p && v < tile_end && v < n) next = jump[v - (u32)tile_begin];
        __syncthreads();
        jump[t] = next;
        __syncthreads();
    }
    if (p >= start && p < n) exit[p] = jump[t];
}

// ONE wavefront: from e = start, entry[tile of e] = e and e = exit[e]; an exit inside the tile is a LONG position x, which
// gets its exact score.  e grows with every step: at most n / tile + (long matches) steps.
__global__ __launch_bounds__(SCL_WAVE) void lz77w_walk(const u8 *win, u32 n, u32 start, u32 L, u32 M, const u32 *order,
                                                       const u32 *rank, u32 *slen, u32 *sq, const u32 *exit, u32 *entry,
                                                       WideMeta *meta) {
    const u32 lane = lz_lane();
    u32 e = start, status = 0;
    while (e < n) {
        const u32 tile = e / LZ_WIDE_TILE;
        if (lane == 0) entry[tile] = e;
        const u32 x = (u32)__builtin_amdgcn_readfirstlane((int)exit[e]);
        if (x < n && x / LZ_WIDE_TILE == tile) {
            u32 q;
            const u32 len = lz_score<LZ_SCORE_FAR>(win, 0, x, n - x, L, M, order, rank, &q);
            if (len < LZ_WIDE_TILE) {  // a LONG position has a match of at least the cap: unreachable, never a reason to spin
                status = SCL_ST_STATE;
                break;
            }
            if (lane == 0) {
                slen[x] = len;
                sq[x] = q;
            }
            e = x + len;
        } else {
            if (x <= e) {  // unreachable: an exit lies past its position
                status = SCL_ST_STATE;
                break;
            }
            e = x;
        }
    }
    if (lane == 0) meta->walk_status = status;
}

// One wavefront per tile follows the chain from the tile's entry to the tile's end: the next set candidate bit is the
// next sequence, everything in between is literals.  WRITE = false counts: cnt = sequences that start in the tile, msum =
// their matched bytes, lend = where the last of them ends (0: none).  WRITE = true, with the scans of those over the tiles
// (seq_off, m_off exclusive sums; prev_end the exclusive maximum), stores rows and the tile's own literal bytes: a
// literal at position j is literal number j - start - (bytes matched before j).  The run of literals in front of sequence
// k is stored if k < seq_cap, the run behind the last sequence if all sequences fit -- what the one-wave parse leaves.
template <bool WRITE>
__global__ __launch_bounds__(256) void lz77w_tile_emit(const u8 *win, u32 n, u32 start, u32 n_tiles, const u64 *bitmap,
                                                       const u32 *slen, const u32 *sq, const u32 *entry, u32 *cnt,
                                                       u32 *msum, u32 *lend, u32 seq_cap, u32 *lit_count, u32 *match_len,
                                                       u32 *match_off, u8 *literals, u32 *n_lit_out) {
    const u32 lane = lz_lane();
    const u32 tile = blockIdx.x * (blockDim.x / SCL_WAVE) + threadIdx.x / SCL_WAVE;
    if (tile > n_tiles) return;
    if (tile == n_tiles) {  // the entry behind the last tile: the scans leave the totals there
        if (!WRITE && lane == 0) cnt[tile] = msum[tile] = lend[tile] = 0;
        return;
    }
    const u64 tile_stop = (u64)(tile + 1) * LZ_WIDE_TILE;
    const u32 tile_end = tile_stop < n ? (u32)tile_stop : n;
    const u32 e = entry[tile];
    u32 seqs = 0, matched = 0, last_end = 0;
    if (e != LZ_WIDE_NONE) {
        const u32 total_seqs = WRITE ? cnt[n_tiles] : 0;
        const u32 k0 = WRITE ? cnt[tile] : 0;
        u32 before = WRITE ? msum[tile] : 0;  // bytes matched by the sequences in front of the current one
        u32 prev = WRITE ? lend[tile] : 0;    // where the sequence in front of the current one ends
        if (prev < start) prev = start;
        u8 *lit = literals + start;
        u32 pos = e;
        while (pos < tile_end) {
            const u32 p = (u32)lz_next_bit(bitmap, pos, tile_end);
            const u32 k = k0 + seqs;
            if (WRITE && (k < seq_cap || (k == total_seqs && total_seqs <= seq_cap)))
                for (u32 j = pos + lane; j < p; j += SCL_WAVE) lit[j - start - before] = win[j];
            if (p >= tile_end) break;
            const u32 len = slen[p];
            if (WRITE && lane == 0) {
                if (k < seq_cap) {
                    lit_count[k] = p - prev;
                    match_len[k] = len;
                    match_off[k] = p - sq[p];
                } else if (k == seq_cap) {
                    *n_lit_out = prev - start - before;  // the literals of the sequences that fit
                }
            }
            u64 next = (u64)p + (len ? len : 1u);
            if (next > n) next = n;  // (a match never passes the window; keeps the loop bounded on any table)
            pos = prev = last_end = (u32)next;
            seqs += 1;
            matched += len;
            before += len;
        }
    }
    if (!WRITE && lane == 0) {
        cnt[tile] = seqs;
        msum[tile] = matched;
        lend[tile] = last_end;
    }
}

// exclusive running maximum of a[0..n) in place, one workgroup
__global__ __launch_bounds__(LZ_SCAN_THREADS) void lz77w_scan_max(u32 *a, u64 n) {
    __shared__ u32 s_wave[LZ_SCAN_THREADS / SCL_WAVE];
    (void)scl_block_scan_array<u32, LZ_SCAN_THREADS, SclScanMax>(a, n, s_wave);
}

// cnt[n_tiles], msum[n_tiles]: the totals.  n_lit of a block with too many sequences comes from lz77w_tile_emit.
__global__ void lz77w_parse_finish(u32 n, u32 start, u32 n_tiles, const u32 *cnt, const u32 *msum, u32 seq_cap,
                                   const WideMeta *meta, u32 *n_seq_out, u32 *n_lit_out, u32 *status_out) {
    const u32 total = cnt[n_tiles];
    u32 status = meta->walk_status;
    if (total > seq_cap) status |= SCL_ST_CAPACITY;
    *n_seq_out = total > seq_cap ? seq_cap : total;
    if (total <= seq_cap) *n_lit_out = n - start - msum[n_tiles];
    *status_out = status;
}

__global__ void lz77w_parse_empty(u32 *n_seq_out, u32 *n_lit_out, u32 *status_out) {
    *n_seq_out = 0;
    *n_lit_out = 0;
    *status_out = 0;
}

// ---- replay ----------------------------------------------------------------------------------------------------------
// lit_sum[k] = literal_count[k], all_sum[k] = literal_count[k] + match_length[k] (a value of 2^32 or more stands for
// 2^32: it faults in any slot, and the sums of 2^32 such values stay below 2^64); entry n_seq = 0 takes the totals
__global__ __launch_bounds__(256) void lz77w_replay_sums(const u32 *lit_count, const u32 *match_len, u64 n_seq,
                                                         u64 *lit_sum, u64 *all_sum, ReplayMeta *meta) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        meta->first = (u32)n_seq;
        meta->status = 0;
        meta->out_end = 0;
        for (u32 r = 0; r < LZ_WIDE_ROUND_FLAGS; ++r) meta->changed[r] = r == 0;
    }
    if (k > n_seq) return;
    u64 run = 0, both = 0;
    if (k < n_seq) {
        run = lit_count[k];
        both = run + match_len[k];
        if (both > (1ull << 32)) both = 1ull << 32;
    }
    lit_sum[k] = run;
    all_sum[k] = both;
}

// the checks of sequence k in the one-wave kernel's order; d = output position and lp = literal position in front of it.
// -> 0, or the status; *with_literals: the literal run is produced all the same (the fault is in the match).  The one
// place that decides statuses, for both coders: WINDOWED (the sliding-window coder, lz_replay_stream<true>) a sequence
// with match length 0 copies nothing and its offset is not looked at, and an offset above `window` (0: no bound) is
// SCL_ST_STATE.
template <bool WINDOWED>
__device__ __forceinline__ u32 lz77w_check(u64 d, u64 lp, u32 run, u32 len, u32 off, u64 cap, u64 n_lit, u32 window,
                                           bool *with_literals) {
    *with_literals = false;
    if (lp > n_lit || run > n_lit - lp) return SCL_ST_TRUNCATED;
    if (d > cap || run > cap - d) return SCL_ST_CAPACITY;
    *with_literals = true;
    d += run;
    if (WINDOWED && len == 0) return 0;
    if (off == 0 || off > d || (WINDOWED && window && off > window)) return SCL_ST_STATE;
    if (len > cap - d) return SCL_ST_CAPACITY;
    return 0;
}

template <bool WINDOWED>
__global__ __launch_bounds__(256) void lz77w_replay_validate(const u32 *lit_count, const u32 *match_len,
                                                             const u32 *match_off, u64 n_seq, const u64 *lit_sum,
                                                             const u64 *all_sum, u64 have, u64 cap, u64 n_lit,
                                                             u32 window, ReplayMeta *meta) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_seq) return;
    bool with_literals;
    if (lz77w_check<WINDOWED>(have + all_sum[k], lit_sum[k], lit_count[k], match_len[k], match_off[k], cap, n_lit, window,
                              &with_literals))
        atomicMin(&meta->first, (u32)k);
}

// one thread: what the stream produces up to its first fault -> meta->out_end, out_len, status
template <bool WINDOWED>
__global__ void lz77w_replay_plan(const u32 *lit_count, const u32 *match_len, const u32 *match_off, u64 n_seq,
                                  const u64 *lit_sum, const u64 *all_sum, u64 have, u64 cap, u64 n_lit, u32 window,
                                  ReplayMeta *meta, u32 *out_len, u32 *status_out) {
    const u64 f = meta->first;
    const u64 d = have + all_sum[f], lp = lit_sum[f];
    u64 end = d;
    u32 status = 0;
    if (f < n_seq) {
        bool with_literals;
        status = lz77w_check<WINDOWED>(d, lp, lit_count[f], match_len[f], match_off[f], cap, n_lit, window, &with_literals);
        if (with_literals) end = d + lit_count[f];
    } else {  // the literals left over
        const u64 rest = n_lit - lp;
        if (rest > cap - d)
            status = SCL_ST_CAPACITY;
        else
            end = d + rest;
    }
    meta->status = status;
    meta->out_end = end;
    *out_len = (u32)(end - have);
    *status_out = status;
}

// One thread per produced byte i: its sequence k is the last with have + all_sum[k] <= i (k = n_seq: the literals left
// over).  A literal byte is stored and is its own root; a match byte's root is the earlier byte it copies.
// A sequence without a match has no match byte, whatever its offset says: the remainder is taken of a validated offset
// only (an offset of 0 on a byte that no input reaches makes the byte its own root).
__global__ __launch_bounds__(256) void lz77w_resolve_init(u8 *out, u64 have, const u32 *lit_count, const u32 *match_off,
                                                          u64 n_seq, const u64 *lit_sum, const u64 *all_sum,
                                                          const u8 *literals, const ReplayMeta *meta, u32 *root) {
    const u64 i = have + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= meta->out_end) return;
    const u64 at = i - have;
    u64 lo = 0, hi = n_seq + 1;  // invariant: all_sum[lo] <= at, and the answer is in [lo, hi)
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (all_sum[mid] <= at)
            lo = mid;
        else
            hi = mid;
    }
    const u64 d = have + all_sum[lo];
    const u64 run = lo < n_seq ? lit_count[lo] : ~0ull;
    if (i - d < run) {
        out[i] = literals[lit_sum[lo] + (i - d)];
        root[at] = (u32)i;
    } else {
        const u64 m = d + run, off = match_off[lo];
        root[at] = off ? (u32)(m - off + (i - m) % off) : (u32)i;
    }
}

// root = root[root] for every byte whose root is neither history nor a stored literal; a round after one that moved
// nothing does nothing.  A root read while another thread replaces it is the old or the new one: both are earlier bytes
// this byte equals.
__global__ __launch_bounds__(256) void lz77w_resolve_round(u64 have, ReplayMeta *meta, u32 *root, u32 round) {
    if (!meta->changed[round]) return;
    const u64 at = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool moved = false;
    if (have + at < meta->out_end) {
        const u32 v = root[at];
        if (v >= have && v != have + at) {
            const u32 u = root[v - have];
            if (u != v) {
                root[at] = u;
                moved = true;
            }
        }
    }
    if (__ballot(moved) && lz_lane() == 0) meta->changed[round + 1] = 1;
}

__global__ __launch_bounds__(256) void lz77w_resolve_gather(u8 *out, u64 have, const ReplayMeta *meta, const u32 *root) {
    const u64 at = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = have + at;
    if (i >= meta->out_end) return;
    const u32 v = root[at];
    if (v != i) out[i] = out[v];  // v: history, or a literal byte stored by lz77w_resolve_init
}

u32 wide_rounds(u64 n_seq) {  // ceil(log2(n_seq + 1)) + 1
    u32 r = 0;
    while ((1ull << r) < n_seq + 1) ++r;
    return r + 1;
}

}  // namespace

extern "C" void scl_lz77_wide_shape(uint32_t *tile, uint32_t *cap) {
    if (tile) *tile = LZ_WIDE_TILE;
    if (cap) *cap = LZ_WIDE_CAP;
}

extern "C" uint64_t scl_lz77_wide_threshold(void) { return LZ_WIDE_THRESHOLD; }

extern "C" uint64_t scl_lz77_wide_scratch_bytes(uint64_t n) { return wide_scratch_layout(n).total; }

extern "C" uint64_t scl_lz77_wide_replay_scratch_bytes(uint64_t n_seq, uint64_t grow_bytes) {
    return replay_scratch_layout(n_seq, grow_bytes).total;
}

extern "C" int scl_lz77_wide_kernel_names(char *score, char *walk, char *resolve, uint64_t cap) {
    SCL_REQUIRE(cap >= 96, "lz77_wide_kernel_names: cap must be at least 96");
    if (score) snprintf(score, cap, "lz77w_score");
    if (walk) snprintf(walk, cap, "lz77w_walk");
    if (resolve) snprintf(resolve, cap, "lz77w_resolve_round");
    return SCL_OK;
}

extern "C" int scl_lz77_parse_wide(const scl_lz77_wide_parse_args *a, void *stream) {
    const char *what = "lz77_parse_wide";
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_n_seq && a->d_n_lit && a->d_status && a->d_scratch && (a->n == 0 || (a->d_win && a->d_literals)) &&
                    (a->seq_cap == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->min_match_length >= 1 && a->min_match_length <= 8,
                "%s: min_match_length %u: an L-gram is one 64-bit key, 1 <= L <= 8", what, a->min_match_length);
    SCL_REQUIRE(a->max_matches >= 1 && a->max_matches <= 64,
                "%s: max_matches %u: every position is scored against one wavefront of candidates, 1 <= M <= 64", what,
                a->max_matches);
    SCL_REQUIRE(a->n < (1ull << 32) && a->start <= a->n, "%s: start <= n < 2^32", what);
    SCL_REQUIRE(a->phases <= 15, "%s: phases is a mask of SCL_LZ77_WIDE_INDEX | _SCORE | _WALK | _EMIT", what);
    const WideScratch lay = wide_scratch_layout(a->n);
    SCL_REQUIRE(((uintptr_t)a->d_scratch & 255) == 0 && a->scratch_bytes >= lay.total,
                "%s: d_scratch must be 256-byte aligned and hold scl_lz77_wide_scratch_bytes = %llu bytes", what,
                (unsigned long long)lay.total);
    hipStream_t st = (hipStream_t)stream;
    if (a->start == a->n) {
        hipLaunchKernelGGL(lz77w_parse_empty, dim3(1), dim3(1), 0, st, a->d_n_seq, a->d_n_lit, a->d_status);
        SCL_HIP_TRY(hipGetLastError());
        return SCL_OK;
    }
    const u32 n = (u32)a->n, start = (u32)a->start, L = a->min_match_length, M = a->max_matches;
    const u32 n_tiles = (u32)lay.n_tiles;
    u8 *scr = (u8 *)a->d_scratch;
    WideMeta *meta = (WideMeta *)(scr + lay.meta);
    const u32 *order = (const u32 *)(scr + lay.index.order_a), *rank = (const u32 *)(scr + lay.index.rank);
    const u64 *bitmap = (const u64 *)(scr + lay.index.bitmap);
    u32 *slen = (u32 *)(scr + lay.slen), *sq = (u32 *)(scr + lay.sq), *exit = (u32 *)(scr + lay.exit);
    u32 *entry = (u32 *)(scr + lay.entry), *cnt = (u32 *)(scr + lay.cnt), *msum = (u32 *)(scr + lay.msum);
    u32 *lend = (u32 *)(scr + lay.lend), *sums = (u32 *)(scr + lay.sums);

    const u32 phases = a->phases ? a->phases : 15u;
    if (phases & SCL_LZ77_WIDE_INDEX) {
        hipLaunchKernelGGL(lz77w_parse_init, dim3(1), dim3(1), 0, st, meta, a->n, start);
        scl_lz77_parse_args ix = {};  // the index phase of a batch of one, on the front of the scratch
        ix.d_win = a->d_win;
        ix.d_win_off = meta->win_off;
        ix.d_start = &meta->start;
        ix.n_streams = 1;
        ix.total_bytes = a->n;
        ix.min_match_length = L;
        ix.max_matches = M;
        ix.phases = SCL_LZ77_INDEX;
        ix.d_literals = a->d_literals;
        ix.d_n_seq = a->d_n_seq;
        ix.d_n_lit = a->d_n_lit;
        ix.d_status = a->d_status;
        ix.d_scratch = a->d_scratch;
        ix.scratch_bytes = lay.index.total;
        const int rc = scl_lz77_parse_batch(&ix, stream);
        if (rc) return rc;
    }
    const u32 words = (u32)(((u64)n + 63) / 64 - start / 64);
    if (phases & SCL_LZ77_WIDE_SCORE) {
        hipLaunchKernelGGL(lz77w_score, dim3((words + 3) / 4), dim3(256), 0, st, a->d_win, n, start, L, M, order, rank, bitmap,
                           slen, sq);
        hipLaunchKernelGGL(lz77w_tile_exits, dim3(n_tiles), dim3(LZ_WIDE_TILE), 0, st, n, start, slen, exit, entry);
    }
    if (phases & SCL_LZ77_WIDE_WALK)
        hipLaunchKernelGGL(lz77w_walk, dim3(1), dim3(SCL_WAVE), 0, st, a->d_win, n, start, L, M, order, rank, slen, sq, exit,
                           entry, meta);
    if (phases & SCL_LZ77_WIDE_EMIT) {
        const u32 emit_blocks = (u32)(((u64)n_tiles + 1 + 3) / 4);
        hipLaunchKernelGGL(lz77w_tile_emit<false>, dim3(emit_blocks), dim3(256), 0, st, a->d_win, n, start, n_tiles, bitmap, slen,
                           sq, entry, cnt, msum, lend, a->seq_cap, a->d_lit_count, a->d_match_len, a->d_match_off,
                           a->d_literals, a->d_n_lit);
        lz77_scan_exclusive(cnt, (u64)n_tiles + 1, sums, st);
        lz77_scan_exclusive(msum, (u64)n_tiles + 1, sums, st);
        hipLaunchKernelGGL(lz77w_scan_max, dim3(1), dim3(LZ_SCAN_THREADS), 0, st, lend, (u64)n_tiles + 1);
        hipLaunchKernelGGL(lz77w_parse_finish, dim3(1), dim3(1), 0, st, n, start, n_tiles, cnt, msum, a->seq_cap, meta,
                           a->d_n_seq, a->d_n_lit, a->d_status);
        hipLaunchKernelGGL(lz77w_tile_emit<true>, dim3(emit_blocks), dim3(256), 0, st, a->d_win, n, start, n_tiles, bitmap, slen,
                           sq, entry, cnt, msum, lend, a->seq_cap, a->d_lit_count, a->d_match_len, a->d_match_off,
                           a->d_literals, a->d_n_lit);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

// Both *_replay_wide entry points: A is scl_lz77_wide_replay_args or scl_lz77_sliding_wide_replay_args (the same fields,
// the second with a window_size behind them), WINDOWED and `window` the sliding-window coder's two rules.
template <bool WINDOWED, class A>
static int replay_wide_run(const char *what, const A *a, u32 window, void *stream) {
    SCL_REQUIRE(a, "%s: null pointer argument", what);
    SCL_REQUIRE(a->d_out_len && a->d_status && a->d_scratch && (a->cap == 0 || a->d_win) &&
                    (a->n_lit == 0 || a->d_literals) &&
                    (a->n_seq == 0 || (a->d_lit_count && a->d_match_len && a->d_match_off)),
                "%s: null pointer argument", what);
    SCL_REQUIRE(a->cap < (1ull << 32) && a->have <= a->cap && a->n_seq < (1ull << 32) && a->n_lit < (1ull << 32),
                "%s: have <= cap < 2^32, n_seq and n_lit < 2^32", what);
    const u64 grow = a->cap - a->have;
    const ReplayScratch lay = replay_scratch_layout(a->n_seq, grow);
    SCL_REQUIRE(((uintptr_t)a->d_scratch & 255) == 0 && a->scratch_bytes >= lay.total,
                "%s: d_scratch must be 256-byte aligned and hold scl_lz77_wide_replay_scratch_bytes = %llu bytes", what,
                (unsigned long long)lay.total);
    hipStream_t st = (hipStream_t)stream;
    u8 *scr = (u8 *)a->d_scratch;
    u64 *lit_sum = (u64 *)(scr + lay.lit_sum), *all_sum = (u64 *)(scr + lay.all_sum), *sums = (u64 *)(scr + lay.sums);
    u32 *root = (u32 *)(scr + lay.root);
    ReplayMeta *meta = (ReplayMeta *)(scr + lay.meta);
    const u64 n_seq = a->n_seq;
    hipLaunchKernelGGL(lz77w_replay_sums, dim3((u32)((n_seq + 256) / 256)), dim3(256), 0, st, a->d_lit_count, a->d_match_len,
                       n_seq, lit_sum, all_sum, meta);
    lz77_scan_exclusive(lit_sum, n_seq + 1, sums, st);
    lz77_scan_exclusive(all_sum, n_seq + 1, sums, st);
    if (n_seq)
        hipLaunchKernelGGL(lz77w_replay_validate<WINDOWED>, dim3((u32)((n_seq + 255) / 256)), dim3(256), 0, st, a->d_lit_count,
                           a->d_match_len, a->d_match_off, n_seq, lit_sum, all_sum, a->have, a->cap, a->n_lit, window, meta);
    hipLaunchKernelGGL(lz77w_replay_plan<WINDOWED>, dim3(1), dim3(1), 0, st, a->d_lit_count, a->d_match_len, a->d_match_off,
                       n_seq, lit_sum, all_sum, a->have, a->cap, a->n_lit, window, meta, a->d_out_len, a->d_status);
    if (grow) {
        const u32 blocks = (u32)((grow + 255) / 256);
        hipLaunchKernelGGL(lz77w_resolve_init, dim3(blocks), dim3(256), 0, st, a->d_win, a->have, a->d_lit_count,
                           a->d_match_off, n_seq, lit_sum, all_sum, a->d_literals, meta, root);
        const u32 rounds = n_seq ? wide_rounds(n_seq) : 0;
        for (u32 r = 0; r < rounds; ++r)
            hipLaunchKernelGGL(lz77w_resolve_round, dim3(blocks), dim3(256), 0, st, a->have, meta, root, r);
        hipLaunchKernelGGL(lz77w_resolve_gather, dim3(blocks), dim3(256), 0, st, a->d_win, a->have, meta, root);
    }
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_lz77_replay_wide(const scl_lz77_wide_replay_args *a, void *stream) {
    return replay_wide_run<false>("lz77_replay_wide", a, 0u, stream);
}

// the sliding-window coder's replay of one stream (scl_lz77_sliding_wide.hip has its parse): these kernels, WINDOWED
extern "C" int scl_lz77_sliding_replay_wide(const scl_lz77_sliding_wide_replay_args *a, void *stream) {
    return replay_wide_run<true>("lz77_sliding_replay_wide", a, a ? a->window_size : 0u, stream);
}
