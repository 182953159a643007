// scl_bit_block.h -- the pieces of "one block of variable-length codewords across the whole grid" that do not depend on
// whose codewords they are: the shapes; the encoder (the bodies of the tile-bits and tile-emit kernels over a value policy, the
// scan of the tile sums, the tail kernel); the decoder (its input window, the bodies of the self-synchronising scheme -- walk,
// sync, end-of-stream scan, write -- over a codeword policy, the verdict kernel); the host side (the launchers with the entry
// points' checks, the pass loop of a section, the staging of one block in host memory).  ONE copy, used by
// scl_prefix_block.hip (tables of a scl_prefix_model), scl_uint_block.hip (Golomb, universal, Elias-delta: a rule, no table)
// and scl_lz77_entropy_wide.hip (the four fields of an LZ77 stream at any bit position, tables built on the device, its own
// seven-section scan and verdict).  Each keeps its two policies and its __global__ kernels over them (thin: tables in LDS, one
// call).  Internal to csrc/; DESIGN.md 3.5.1, 3.5.2, 3.6.3.
#pragma once

#include "scl_common.h"
#include "scl_scan.h"

#define PFB_THREADS 256
#define PFB_PER_THREAD 16u
#define PFB_MAX_LEN 32u                  // the longest codeword (or run of residual bits) a tile value may have
#define PFB_TILE (PFB_THREADS * PFB_PER_THREAD)  // 4096 symbols: <= 131072 bits = 4096 words (+ 2 for the offset)
#define PFB_TILE_WORDS (PFB_TILE * PFB_MAX_LEN / 32u + 2u)
#define PFB_SUB 128u                     // S: bits per decoder thread (>= 32: a codeword spans at most two)
#define PFB_GROUP (PFB_THREADS * PFB_SUB)  // W: bits per decoder workgroup
#define PFB_WIN_WORDS (PFB_GROUP / 32u + 4u)  // a walk ends before W + 64; + 31 bits of offset, + 1 word of lookahead
#define PFB_SCAN_THREADS 1024
#define PFB_NONE64 0xFFFFFFFFFFFFFFFFull

// how a thread's walk over its subsequence ended
#define PFB_END_EXIT 0u   // at a codeword boundary at or past the end of the subsequence (or at the end of the stream)
#define PFB_END_TRUNC 1u  // in_nbits cuts the codeword that starts at `end`
#define PFB_END_STATE 2u  // the codeword that starts at `end` walks into a missing child
// one u32 per subsequence: start - i*S (0..31) | symbols << 6 (0..128) | how it ended << 15 | (end - i*S) << 17 (0..159)
#define PFB_PACK(start_off, count, kind, end_off) ((start_off) | ((count) << 6) | ((kind) << 15) | ((end_off) << 17))

struct PfbEncScratch {  // head of the encoder's scratch
    u32 fits;           // the stream fits out_cap_bytes: set before a tile is emitted
    u32 tail_word;      // the output word that out_cap_bytes cuts, in memory byte order
};

struct PfbDecHead {   // head of the decoder's scratch (zeroed by the entry point); the host reads the two pass words
    u32 start_pass;   // the last pass in which a workgroup moved its start
    u32 exit_pass;    // the last pass in which a workgroup's last exit changed
    u64 n_total;      // scan_groups: symbols of the stream (before the cap)
    u64 last_group;   // scan_groups: the workgroup the stream ends in
};

struct PfbDecGroups {  // device pointers into the decoder's scratch
    u32 *sub;          // [n_groups * 256] PFB_PACK
    u64 *group_exit;   // [2][n_groups] relative to the stream, PFB_NONE64: the workgroup's last thread has no exit
    u64 *group_count;  // [n_groups] symbols up to the workgroup's first cut; scan_groups: their exclusive scan
    u64 *group_end;    // [n_groups] PFB_NONE64, or (position of the codeword that ends the stream) << 2 | PFB_END_*
};

// ---- the scratch of a coder of one block of n values / of a stream of nbits bits (host) -----------------------------------
// encoder: PfbEncScratch, then u64 tile_bits[tiles] at byte 64; decoder: PfbDecHead, then the arrays of PfbDecGroups at byte 64
struct PfbDecScratch {  // device pointers into the decoder's scratch
    PfbDecHead *head;
    PfbDecGroups g;
};

struct PfbDecResult {  // what a block decoder reports: the layout of scl_prefix_block_result and scl_uint_block_result
    u64 n_out, consumed;
    u32 status, sync_passes;
};
#define PFB_RESULT_IS(T)                                                                                                   \
    static_assert(sizeof(T) == 24 && offsetof(T, consumed) == 8 && offsetof(T, status) == 16 && offsetof(T, sync_passes) == 20, \
                  #T " is PfbDecResult under another name")

static inline u64 pfb_tiles(u64 n) { return (n + PFB_TILE - 1) / PFB_TILE; }
static inline u64 pfb_subs(u64 nbits) { return (nbits + PFB_SUB - 1) / PFB_SUB; }
static inline u64 pfb_groups(u64 nbits) { return (pfb_subs(nbits) + PFB_THREADS - 1) / PFB_THREADS; }
static inline u64 pfb_enc_scratch(u64 n) { return 64 + pfb_tiles(n) * 8; }
static inline u64 pfb_dec_scratch(u64 nbits) { return 64 + pfb_groups(nbits) * (PFB_THREADS * 4 + 4 * 8); }

static inline PfbDecScratch pfb_dec_carve(void *d_scratch, u64 n_groups) {
    PfbDecScratch sc;
    u8 *p = (u8 *)d_scratch;
    sc.head = (PfbDecHead *)p;
    sc.g.group_exit = (u64 *)(p + 64);
    sc.g.group_count = sc.g.group_exit + 2 * n_groups;
    sc.g.group_end = sc.g.group_count + n_groups;
    sc.g.sub = (u32 *)(sc.g.group_end + n_groups);
    return sc;
}

#ifdef __HIPCC__
// ---- encode: one tile of PFB_TILE values -----------------------------------------------------------------------------------
// EVERY thread of the workgroup calls.  e[j] = {bits, length} of the thread's PFB_PER_THREAD consecutive values (length 0:
// none; the bits right-aligned, nothing above them), `bits` the sum of the lengths, `base` the bit of the stream at which the
// tile starts -- any position.  The thread's values are contiguous bits: whole words go to s_words (zeroed by the caller,
// behind a barrier) as they fill; the first and the last one are shared with the neighbouring threads, so every word is
// ORed in.  Whole big-endian words then leave coalesced; the first and last word of a tile can be shared with its
// neighbours (any number of them: a tile may be a few bits) and are merged with atomicOr into an output that was zeroed.
// The word `tail_index` (the one out_cap_bytes cuts, or PFB_NONE64) goes to head->tail_word instead.
__device__ __forceinline__ void pfb_emit_tile(const uint2 (&e)[PFB_PER_THREAD], u32 bits, u64 base, u32 *s_words /* [PFB_TILE_WORDS] */,
                                              u32 *s_wave /* [PFB_THREADS / 64] */, PfbEncScratch *__restrict__ head,
                                              u32 *__restrict__ out32, u64 tail_index) {
    const u32 tid = threadIdx.x;
    u32 tile_total;
    const u32 mine = scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &tile_total);
    const u32 r = (u32)(base & 31u);
    u32 wi = (r + mine) >> 5, nacc = (r + mine) & 31u;
    u64 acc = 0;
#pragma unroll
    for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
        if (e[j].y == 0) continue;
        acc = (acc << e[j].y) | e[j].x;
        nacc += e[j].y;
        if (nacc >= 32) {
            atomicOr(&s_words[wi++], (u32)(acc >> (nacc - 32)));
            nacc -= 32;
        }
    }
    if (nacc && bits) atomicOr(&s_words[wi], (u32)(acc << (32 - nacc)));
    __syncthreads();
    const u32 n_words = (r + tile_total + 31) >> 5;  // <= PFB_TILE_WORDS - 1
    const u64 word0 = base >> 5;
    for (u32 w = tid; w < n_words; w += PFB_THREADS) {
        const u32 v = scl_bswap32(s_words[w]);
        const u64 index = word0 + w;
        u32 *dst = index == tail_index ? &head->tail_word : out32 + index;
        if (w == 0 || w + 1 == n_words) {
            if (v) atomicOr(dst, v);  // a word this tile may share with its neighbours
        } else {
            *dst = v;
        }
    }
}

// ---- encode: the bodies of the tile kernels over a value policy ENC, which owns its input and its tables -------------------
//   kTables, load()        EVERY thread calls load(), in front of a barrier: it fills the policy's LDS tables (kTables: it
//                          has some; without, tile-bits needs no barrier)
//   codes(block, e, bad)   the {bits, length} of the thread's PFB_PER_THREAD consecutive values of tile `block` (the contract of
//                          pfb_emit_tile) -> the sum of the lengths; bad = 1 on a value of the block that has no codeword
//   kFault                 the status bit that tile-bits raises for such a value (0: none, the caller finds them elsewhere)
//   tile_base(block)       the bit of the stream at which tile `block` starts (tile-emit; called behind codes(block, ...))
// One workgroup per tile.  tile-bits: tile_bits[tile] = the bits of the tile, *status |= kFault.
template <class ENC>
__device__ __forceinline__ void pfb_tile_bits_body(ENC E, u64 *__restrict__ tile_bits, u32 *__restrict__ status) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    E.load();
    if constexpr (ENC::kTables) __syncthreads();
    uint2 e[PFB_PER_THREAD];
    u32 bad = 0, total;
    const u32 bits = E.codes(blockIdx.x, e, bad);
    (void)scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &total);
    const int any_bad = ENC::kFault ? __syncthreads_or((int)bad) : 0;
    if (threadIdx.x == 0) {
        tile_bits[blockIdx.x] = total;
        if (any_bad) atomicOr(status, (u32)ENC::kFault);
    }
}

// tile-emit: the tile's codewords go to the output at tile_base (pfb_emit_tile).  A stream that does not fit, or that a fault
// stopped, stores nothing (uniform: the whole grid leaves).
template <class ENC>
__device__ __forceinline__ void pfb_encode_tile_body(ENC E, PfbEncScratch *__restrict__ head, u32 *__restrict__ out32,
                                                     u64 tail_index) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_words[PFB_TILE_WORDS];
    if (!head->fits) return;
    E.load();
    for (u32 i = threadIdx.x; i < PFB_TILE_WORDS; i += PFB_THREADS) s_words[i] = 0;
    __syncthreads();
    uint2 e[PFB_PER_THREAD];
    u32 bad = 0;
    const u32 bits = E.codes(blockIdx.x, e, bad);
    pfb_emit_tile(e, bits, E.tile_base(blockIdx.x), s_words, s_wave, head, out32, tail_index);
}

// ONE workgroup: the tile sums become the tile offsets (exclusive 64-bit scan), and the verdict.  STOP: the status bits (of
// tile-bits, the kernel in front) that stop the coding: such a stream has no length and stores nothing.
template <u32 STOP>
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    pfb_scan_tiles_kernel(u64 *__restrict__ tile_bits, u64 n_tiles, u64 out_cap_bytes, PfbEncScratch *__restrict__ head,
                          u64 *__restrict__ nbits, u32 *__restrict__ status) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    const u64 total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(tile_bits, n_tiles, s_wave);
    if (threadIdx.x == 0) {
        const bool coded = (*status & STOP) == 0;
        const bool fits = coded && (total + 7) / 8 <= out_cap_bytes;
        head->fits = fits ? 1u : 0u;
        *nbits = coded ? total : 0ull;
        if (coded && !fits) atomicOr(status, (u32)SCL_ST_CAPACITY);
    }
}

// out_cap_bytes % 4 != 0: the bytes of the last, partial word come from head->tail_word (one thread)
static __global__ void pfb_encode_tail_kernel(const PfbEncScratch *__restrict__ head, const u64 *__restrict__ nbits,
                                              u8 *__restrict__ out, u64 out_cap_bytes) {
    if (!head->fits || ((*nbits + 31) >> 5) <= (out_cap_bytes >> 2)) return;  // nothing written, or not as far as that word
    const u32 v = head->tail_word;
    for (u64 b = out_cap_bytes & ~3ull; b < out_cap_bytes; ++b) out[b] = (u8)(v >> (8 * (b & 3)));
}

// ---- decode: the input a workgroup can reach, in LDS -----------------------------------------------------------------------
// big-endian words from the one that holds the workgroup's first bit, one pad word per 32 (threads read S / 32 = 4 words
// apart: without it four lanes of every eight share a bank).  `in` is 4-byte aligned; no byte at or past in_size_bytes is read.
#define PFB_WIN_AT(i) ((i) + ((i) >> 5))
#define PFB_WIN_LDS (PFB_WIN_WORDS + PFB_WIN_WORDS / 32 + 1)

__device__ __forceinline__ void pfb_load_window(u32 *s_win, const u8 *__restrict__ in, u64 in_size_bytes, u64 first_bit) {
    const u64 word0 = first_bit >> 5;
    for (u32 i = threadIdx.x; i < PFB_WIN_WORDS; i += PFB_THREADS) {
        const u64 b = (word0 + i) * 4;
        u32 v = 0;
        if (b + 4 <= in_size_bytes) {
            v = scl_bswap32(*reinterpret_cast<const u32 *>(in + b));
        } else {
            for (u32 k = 0; k < 4; ++k) v = (v << 8) | (b + k < in_size_bytes ? (u32)in[b + k] : 0u);
        }
        s_win[PFB_WIN_AT(i)] = v;
    }
}

// the 32 bits from bit `pos` of the window (pos counts from the first bit of the window's first word), left-aligned
__device__ __forceinline__ u32 pfb_peek(const u32 *s_win, u32 pos) {
    const u32 i = pos >> 5, o = pos & 31u;
    const u64 two = ((u64)s_win[PFB_WIN_AT(i)] << 32) | s_win[PFB_WIN_AT(i + 1)];
    return (u32)((two << o) >> 32);
}

// ---- decode: the self-synchronising scheme (Weissenberger & Schmidt; scl_prefix_block.hip describes it) --------------------
// The bodies of the sync, scan_groups and write kernels over a codeword policy CODE, which owns its tables:
//   load()                          EVERY thread calls it, in front of the barrier behind pfb_load_window
//   codeword(bits, rem, len, sym)   one codeword from the left-aligned `bits`, of which `rem` >= 1 belong to the stream:
//                                   PFB_END_EXIT (symbol `sym` of `len` bits), or the PFB_END_* that ends the walk
//   len_gcd()                       pass 0 starts thread i at i*S rounded up to it (1: at i*S)
// The stream is `nbits` bits from bit `base_bit` of `in`.  Positions inside a kernel are relative to the workgroup's first
// bit (32-bit): `avail` = bits of the stream from there on, clamped to W + 64, which no walk reaches; `shift` = bit of the
// window's first word at which the workgroup starts.

// Walks from `start` to the first boundary at or past `stop`; returns how the walk ended and where.
template <class CODE>
__device__ __forceinline__ u32 pfb_walk(const CODE &C, const u32 *s_win, u32 shift, u32 start, u32 stop, u32 avail, u32 &count,
                                        u32 &end) {
    u32 pos = start, n = 0, kind = PFB_END_EXIT;
    while (pos < stop) {  // every turn moves pos forward by a codeword or leaves
        u32 len, sym;
        kind = C.codeword(pfb_peek(s_win, shift + pos), avail - pos, len, sym);
        if (kind != PFB_END_EXIT) break;
        pos += len;
        ++n;
    }
    count = n;
    end = pos;
    return kind;
}

template <class CODE>
__device__ __forceinline__ void pfb_sync_body(const CODE &C, const u8 *__restrict__ in, u64 in_size_bytes, u64 base_bit,
                                              u64 nbits, u64 n_sub, u64 n_groups, PfbDecHead *head, const PfbDecGroups &sc,
                                              u32 pass) {
    __shared__ u32 s_win[PFB_WIN_LDS];
    __shared__ u32 s_exit[PFB_THREADS];  // relative to the workgroup, 0xFFFFFFFF: no exit
    __shared__ u64 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_first_cut;
    __shared__ int s_rerun;
    const u32 tid = threadIdx.x;
    const u64 group = blockIdx.x;
    const u64 group_bit = group * PFB_GROUP;  // relative to the stream
    const u64 sub_index = group * PFB_THREADS + tid;
    const bool active = sub_index < n_sub;
    const u64 left64 = nbits - group_bit;
    const u32 avail = (u32)(left64 < PFB_GROUP + 64u ? left64 : PFB_GROUP + 64u);
    const u32 sub0 = tid * PFB_SUB;
    const u32 stop = min(sub0 + PFB_SUB, avail);
    const u64 *exit_in = sc.group_exit + ((pass + 1u) & 1u) * n_groups;
    u64 *exit_out = sc.group_exit + (pass & 1u) * n_groups;

    u32 start = 0, count = 0, kind = PFB_END_EXIT, end = 0;
    u32 from_left = 0xFFFFFFFFu;  // thread 0: the exit of the workgroup on the left
    if (pass == 0) {
        if (active) {  // the guess: i*S rounded up to a multiple of the gcd of the code lengths (sub 0: bit 0, exact)
            const u64 abs_bit = sub_index * PFB_SUB;
            const u32 g = C.len_gcd();
            start = min(sub0 + (u32)((g - (u32)(abs_bit % g)) % g), avail);
        }
    } else {
        if (tid == 0) {
            const u32 packed = sc.sub[sub_index];
            const u64 ex = group ? exit_in[group - 1] : PFB_NONE64;
            const bool moved = ex != PFB_NONE64 && (u32)(ex - group_bit) != (packed & 63u);
            s_rerun = moved ? 1 : 0;
            if (!moved) exit_out[group] = exit_in[group];
            else from_left = (u32)(ex - group_bit);
        }
        __syncthreads();
        if (!s_rerun) return;  // uniform: this workgroup stands as it is
        if (active) {
            const u32 packed = sc.sub[sub_index];
            start = sub0 + (packed & 63u);
            count = (packed >> 6) & 511u;
            kind = (packed >> 15) & 3u;
            end = sub0 + (packed >> 17);
        }
    }
    C.load();
    const u64 first_bit = base_bit + group_bit;
    pfb_load_window(s_win, in, in_size_bytes, first_bit);
    __syncthreads();
    const u32 shift = (u32)(first_bit & 31u);
    if (pass == 0 && active) kind = pfb_walk(C, s_win, shift, start, stop, avail, count, end);
    s_exit[tid] = active && kind == PFB_END_EXIT ? end : 0xFFFFFFFFu;
    __syncthreads();
    // after round r threads 0..r are final: thread r's left neighbour was final when it read its exit
    for (u32 round = 0; round < PFB_THREADS; ++round) {
        const u32 left = tid ? s_exit[tid - 1] : from_left;
        __syncthreads();  // every exit is read before any is written
        const bool moved = active && left != 0xFFFFFFFFu && left != start;
        if (moved) {
            start = left;
            kind = pfb_walk(C, s_win, shift, start, stop, avail, count, end);
            s_exit[tid] = kind == PFB_END_EXIT ? end : 0xFFFFFFFFu;
        }
        if (!__syncthreads_or(moved ? 1 : 0)) break;
    }
    if (active) sc.sub[sub_index] = PFB_PACK(start - sub0, count, kind, end - sub0);
    // what the workgroup contributes if the stream reaches it: the symbols up to its first cut, and the cut
    if (tid == 0) s_first_cut = PFB_THREADS;
    __syncthreads();
    if (active && kind != PFB_END_EXIT) atomicMin(&s_first_cut, tid);
    __syncthreads();
    const u32 first_cut = s_first_cut;
    u64 total;
    (void)scl_block_scan_excl<u64, PFB_THREADS, SclScanSum>(active && tid <= first_cut ? (u64)count : 0ull, s_wave, &total);
    if (tid == first_cut) sc.group_end[group] = ((group_bit + end) << 2) | kind;
    if (tid == 0) {
        sc.group_count[group] = total;
        if (first_cut == PFB_THREADS) sc.group_end[group] = PFB_NONE64;
    }
    if (tid == PFB_THREADS - 1) {
        const u64 ex = active && kind == PFB_END_EXIT ? group_bit + end : PFB_NONE64;
        if (pass) {
            head->start_pass = pass;  // this workgroup moved its start
            if (ex != exit_in[group]) head->exit_pass = pass;
        }
        exit_out[group] = ex;
    }
}

// ONE workgroup of PFB_SCAN_THREADS: the first workgroup whose walk ends the stream (the last one if none does) and, in
// sc.group_count, the exclusive scan of the symbol counts up to it; returns that workgroup, *total = the symbols in front of
// the end.  The verdict on sc.group_end[that workgroup] is the caller's.
__device__ __forceinline__ u64 pfb_scan_to_end(const PfbDecGroups &sc, u64 n_groups, u64 *total) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    __shared__ unsigned long long s_first;
    if (threadIdx.x == 0) s_first = n_groups - 1;
    __syncthreads();
    u64 mine = PFB_NONE64;
    for (u64 i = threadIdx.x; i < n_groups && mine == PFB_NONE64; i += PFB_SCAN_THREADS)
        if (sc.group_end[i] != PFB_NONE64) mine = i;
    if (mine != PFB_NONE64) atomicMin(&s_first, (unsigned long long)mine);
    __syncthreads();
    const u64 last_group = s_first;
    *total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(sc.group_count, last_group + 1, s_wave);
    return last_group;
}

// ONE workgroup: where the stream ends, the symbol offsets of the workgroups up to there, the result as the one-lane decoder
// reports it.  A codeword that in_nbits cuts is SCL_ST_TRUNCATED; CUT: the status of any other end of a walk.
template <u32 CUT>
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    pfb_scan_groups_kernel(PfbDecScratch sc, u64 n_groups, u64 in_nbits, u64 out_cap, u32 sync_passes,
                           PfbDecResult *__restrict__ result) {
    u64 total;
    const u64 last_group = pfb_scan_to_end(sc.g, n_groups, &total);
    if (threadIdx.x == 0) {
        const u64 cut = sc.g.group_end[last_group];
        const u64 end = cut == PFB_NONE64 ? in_nbits : cut >> 2;
        u32 status = cut == PFB_NONE64 ? 0u : ((cut & 3u) == PFB_END_TRUNC ? SCL_ST_TRUNCATED : CUT);
        u64 consumed = end;
        // the one-lane decoder looks at out_cap before every codeword: bits left after out_cap symbols are
        // SCL_ST_CAPACITY whatever they hold.  total > out_cap: the write kernel stores `consumed` (0 for out_cap = 0)
        if (total > out_cap || (total == out_cap && end < in_nbits)) status = SCL_ST_CAPACITY;
        if (total > out_cap) consumed = 0;
        sc.head->n_total = total;
        sc.head->last_group = last_group;
        result->n_out = total < out_cap ? total : out_cap;
        result->consumed = consumed;
        result->status = status;
        result->sync_passes = sync_passes;
    }
}

// every thread decodes its final range once more and stores its symbols at its offset, up to out_cap of them.
// consumed_at_cap (or null): with more than out_cap symbols in the stream, the bit behind symbol out_cap - 1 is stored there
template <class CODE, typename SYM>
__device__ __forceinline__ void pfb_write_body(const CODE &C, const u8 *__restrict__ in, u64 in_size_bytes, u64 base_bit,
                                               u64 nbits, u64 n_sub, const PfbDecHead *head, const PfbDecGroups &sc,
                                               SYM *__restrict__ out, u64 out_cap, u64 *consumed_at_cap) {
    __shared__ u32 s_win[PFB_WIN_LDS];
    __shared__ u64 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_first_cut;
    const u32 tid = threadIdx.x;
    const u64 group = blockIdx.x;
    if (group > head->last_group) return;  // behind the end of the stream (uniform)
    const u64 group_first = sc.group_count[group];
    if (group_first >= out_cap) return;  // nothing of this workgroup is stored (uniform)
    const u64 n_total = head->n_total;
    const u64 group_bit = group * PFB_GROUP;
    const u64 sub_index = group * PFB_THREADS + tid;
    const bool active = sub_index < n_sub;
    const u64 left64 = nbits - group_bit;
    const u32 avail = (u32)(left64 < PFB_GROUP + 64u ? left64 : PFB_GROUP + 64u);
    const u32 packed = active ? sc.sub[sub_index] : 0u;
    const u32 kind = (packed >> 15) & 3u;
    if (tid == 0) s_first_cut = PFB_THREADS;
    C.load();
    const u64 first_bit = base_bit + group_bit;
    pfb_load_window(s_win, in, in_size_bytes, first_bit);
    __syncthreads();
    if (active && kind != PFB_END_EXIT) atomicMin(&s_first_cut, tid);
    __syncthreads();
    const u32 count = active && tid <= s_first_cut ? (packed >> 6) & 511u : 0u;
    u64 total;
    u64 index = group_first + scl_block_scan_excl<u64, PFB_THREADS, SclScanSum>((u64)count, s_wave, &total);
    const u32 shift = (u32)(first_bit & 31u);
    u32 pos = tid * PFB_SUB + (packed & 63u);
    for (u32 k = 0; k < count && index < out_cap; ++k, ++index) {
        u32 len, sym;
        if (C.codeword(pfb_peek(s_win, shift + pos), avail - pos, len, sym) != PFB_END_EXIT)
            break;  // (not reached: the same walk counted these symbols)
        pos += len;
        out[index] = (SYM)sym;
        if (consumed_at_cap && index + 1 == out_cap && n_total > out_cap) *consumed_at_cap = group_bit + pos;
    }
}
#endif  // __HIPCC__

// ---- decode: one section of `nbits` >= 1 bits, the host's pass loop ---------------------------------------------------------
// sync(grid, n_sub, n_groups, p) enqueues sync pass p on `st`.  Pass 0, then passes 1 .. n_groups - 1 at the most (workgroup w
// is final after pass w), fewer when a pass changes no workgroup's exit: after each the host reads {start_pass, exit_pass} at
// d_pass_words.  *sync_passes grows by the passes in which a workgroup moved its start.  Then scan(n_groups, *sync_passes) and
// write(grid, n_sub) enqueue the caller's scan_groups and write kernels.
template <class SYNC, class SCAN, class WRITE>
static int pfb_decode_section(u64 nbits, const void *d_pass_words, hipStream_t st, u32 *sync_passes, SYNC sync, SCAN scan,
                              WRITE write) {
    const u64 n_sub = pfb_subs(nbits), n_groups = pfb_groups(nbits);
    const dim3 grid((u32)n_groups);
    sync(grid, n_sub, n_groups, 0u);
    SCL_HIP_TRY(hipGetLastError());
    for (u64 pass = 1; pass < n_groups; ++pass) {
        sync(grid, n_sub, n_groups, (u32)pass);
        SCL_HIP_TRY(hipGetLastError());
        u32 flags[2];
        SCL_HIP_TRY(hipMemcpyAsync(flags, d_pass_words, 8, hipMemcpyDeviceToHost, st));
        SCL_HIP_TRY(hipStreamSynchronize(st));
        if (flags[0] == (u32)pass) ++*sync_passes;
        if (flags[1] != (u32)pass) break;
    }
    scan(n_groups, *sync_passes);
    write(grid, n_sub);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

// ---- the entry points of a coder of one block (prefix-free codes, integer codes) --------------------------------------------
struct PfbWords {  // what the two coders' messages name differently
    const char *values, *scratch_fn;         // what a block holds ("symbols"); the function that sizes the scratch
    const char *enc_aligned, *dec_aligned;  // the alignment rule of the encode call, of the decode call
};
// what an encode / a decode call takes behind its model or rule, under the names of include/scl_hip.h
struct PfbEncodeArgs {
    const void *d_val;
    u64 n;
    u8 *d_out;
    u64 out_cap_bytes, *d_nbits;
    u32 *d_status;
    void *d_scratch;
    u64 scratch_bytes;
};
struct PfbDecodeArgs {
    const u8 *d_in;
    u64 in_size_bytes, in_bit_offset, in_nbits;
    void *d_out;
    u64 out_cap;
    PfbDecResult *d_result;
    void *d_scratch;
    u64 scratch_bytes;
};

#ifdef __HIPCC__
// Encode: the caller has checked its model or rule, and that its own pointers (values, status) are `aligned`.  `reach`: the
// bytes of the longest stream of a.n values (the tiles OR their shared words in, so the output is zeroed that far).
// tile_bits(grid, tile_bits, status) and emit(grid, tile_off, head, out32, tail_index) enqueue the caller's two tile kernels.
template <u32 STOP, class BITS, class EMIT>
static int pfb_encode_launch(const char *what, const PfbWords &w, const PfbEncodeArgs &a, bool aligned, u64 reach, hipStream_t st,
                             BITS tile_bits_launch, EMIT emit_launch) {
    SCL_REQUIRE(a.d_out && a.d_nbits && a.d_status && a.d_scratch && (a.d_val || a.n == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(a.n < (1ull << 32), "%s: %llu %s: a block holds fewer than 2^32", what, (unsigned long long)a.n, w.values);
    SCL_REQUIRE(((uintptr_t)a.d_out & 3) == 0 && ((uintptr_t)a.d_scratch & 7) == 0 && ((uintptr_t)a.d_nbits & 7) == 0 && aligned,
                "%s: %s", what, w.enc_aligned);
    SCL_REQUIRE(a.scratch_bytes >= pfb_enc_scratch(a.n), "%s: scratch of %llu bytes, %s asks for %llu", what,
                (unsigned long long)a.scratch_bytes, w.scratch_fn, (unsigned long long)pfb_enc_scratch(a.n));
    SCL_HIP_TRY(hipMemsetAsync(a.d_nbits, 0, 8, st));
    SCL_HIP_TRY(hipMemsetAsync(a.d_status, 0, 4, st));
    if (a.n == 0) return SCL_OK;
    PfbEncScratch *head = (PfbEncScratch *)a.d_scratch;
    u64 *tile_bits = (u64 *)((u8 *)a.d_scratch + 64);
    const dim3 grid((u32)pfb_tiles(a.n));
    const u64 zeroed = reach < a.out_cap_bytes ? reach : a.out_cap_bytes;
    if (zeroed) SCL_HIP_TRY(hipMemsetAsync(a.d_out, 0, zeroed, st));
    SCL_HIP_TRY(hipMemsetAsync(head, 0, 64, st));
    tile_bits_launch(grid, tile_bits, a.d_status);
    hipLaunchKernelGGL(pfb_scan_tiles_kernel<STOP>, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, tile_bits, pfb_tiles(a.n),
                       a.out_cap_bytes, head, a.d_nbits, a.d_status);
    const u64 tail_index = (a.out_cap_bytes & 3) ? a.out_cap_bytes >> 2 : PFB_NONE64;
    emit_launch(grid, (const u64 *)tile_bits, head, (u32 *)a.d_out, tail_index);
    if (a.out_cap_bytes & 3)
        hipLaunchKernelGGL(pfb_encode_tail_kernel, dim3(1), dim3(1), 0, st, (const PfbEncScratch *)head, (const u64 *)a.d_nbits,
                           a.d_out, a.out_cap_bytes);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

// Decode: as encode.  sync(grid, n_sub, n_groups, sc, pass) and write(grid, n_sub, sc) enqueue the caller's two kernels.
template <u32 CUT, class SYNC, class WRITE>
static int pfb_decode_launch(const char *what, const PfbWords &w, const PfbDecodeArgs &a, bool aligned, hipStream_t st,
                             SYNC sync_launch, WRITE write_launch) {
    SCL_REQUIRE(a.d_in && a.d_result && a.d_scratch && (a.d_out || a.out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(a.in_nbits < (1ull << 46) && a.in_bit_offset < (1ull << 62), "%s: stream of %llu bits: 2^46 and more are not coded",
                what, (unsigned long long)a.in_nbits);
    SCL_REQUIRE(((uintptr_t)a.d_in & 3) == 0 && ((uintptr_t)a.d_scratch & 7) == 0 && ((uintptr_t)a.d_result & 7) == 0 && aligned,
                "%s: %s", what, w.dec_aligned);
    SCL_REQUIRE(a.scratch_bytes >= pfb_dec_scratch(a.in_nbits), "%s: scratch of %llu bytes, %s asks for %llu", what,
                (unsigned long long)a.scratch_bytes, w.scratch_fn, (unsigned long long)pfb_dec_scratch(a.in_nbits));
    SCL_REQUIRE((a.in_bit_offset + a.in_nbits + 7) / 8 <= a.in_size_bytes, "%s: the stream ends behind in_size_bytes", what);
    if (a.in_nbits == 0) {  // an empty stream: nothing decoded, nothing is launched
        SCL_HIP_TRY(hipMemsetAsync(a.d_result, 0, sizeof(PfbDecResult), st));
        return SCL_OK;
    }
    const PfbDecScratch sc = pfb_dec_carve(a.d_scratch, pfb_groups(a.in_nbits));
    SCL_HIP_TRY(hipMemsetAsync(sc.head, 0, 64, st));
    u32 sync_passes = 0;
    return pfb_decode_section(
        a.in_nbits, sc.head, st, &sync_passes,
        [&](dim3 grid, u64 n_sub, u64 n_groups, u32 pass) { sync_launch(grid, n_sub, n_groups, sc, pass); },
        [&](u64 n_groups, u32 passes) {
            hipLaunchKernelGGL(pfb_scan_groups_kernel<CUT>, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, n_groups, a.in_nbits,
                               a.out_cap, passes, a.d_result);
        },
        [&](dim3 grid, u64 n_sub) { write_launch(grid, n_sub, sc); });
}
#endif  // __HIPCC__

// ---- one block in host memory: four device buffers, copy in, run, wait, read the result, copy out ---------------------------
// run(const PfbEncodeArgs &) is the coder's encode call on the null stream (its checks included).  -> *nbits, *status; the
// stream's bytes reach h_out with status 0 only.
template <class RUN>
static int pfb_encode_staged(const char *what, const PfbWords &w, const void *h_val, u64 n, u64 val_bytes, u64 reach, u8 *h_out,
                             u64 out_cap_bytes, u64 *nbits, u32 *status, RUN run) {
    SCL_REQUIRE(n < (1ull << 32), "%s: %llu %s: a block holds fewer than 2^32", what, (unsigned long long)n, w.values);
    const u64 cap = reach < out_cap_bytes ? reach : out_cap_bytes;  // no stream of n values is longer than `reach`
    const u64 scratch_bytes = pfb_enc_scratch(n);
    ScratchDev d_val, d_out, d_meta, d_scr;
    int rc;
    if ((rc = d_val.alloc(n * val_bytes)) || (rc = d_out.alloc(cap)) || (rc = d_meta.alloc(16)) || (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    if (n) SCL_HIP_TRY(hipMemcpy(d_val.p, h_val, n * val_bytes, hipMemcpyHostToDevice));
    rc = run(PfbEncodeArgs{d_val.p, n, (u8 *)d_out.p, cap, (u64 *)d_meta.p, (u32 *)d_meta.p + 2, d_scr.p, scratch_bytes});
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    u64 meta[2];
    SCL_HIP_TRY(hipMemcpy(meta, d_meta.p, 16, hipMemcpyDeviceToHost));
    const u64 bytes = (meta[0] + 7) / 8;
    SCL_REQUIRE(bytes <= out_cap_bytes, "%s: output needs %llu bytes, capacity %llu", what, (unsigned long long)bytes,
                (unsigned long long)out_cap_bytes);
    *nbits = meta[0];
    *status = (u32)meta[1];
    if (*status == 0 && bytes) SCL_HIP_TRY(hipMemcpy(h_out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return SCL_OK;
}

// run(const PfbDecodeArgs &) is the coder's decode call on the null stream.  The device copy is padded to the words a window
// load reaches, EVERY byte behind the stream zero (no policy trusts a bit past in_nbits -- each tests `len > rem` / `d == rem`
// first -- but what it looks at is defined).  -> *n_out, *consumed, *status; the values reach h_out with status 0, and in front
// of a fault if `partial`.
template <class RUN>
static int pfb_decode_staged(const char *what, const u8 *h_in, u64 in_nbits, void *h_out, u64 val_bytes, u64 out_cap, bool partial,
                             u64 *n_out, u64 *consumed, u32 *status, RUN run) {
    SCL_REQUIRE(in_nbits < (1ull << 46), "%s: stream of %llu bits: 2^46 and more are not coded", what,
                (unsigned long long)in_nbits);
    const u64 in_bytes = (in_nbits + 7) / 8, in_size = scl_round_up(in_bytes, 4) + 4;
    const u64 scratch_bytes = pfb_dec_scratch(in_nbits);
    ScratchDev d_in, d_out, d_res, d_scr;
    int rc;
    if ((rc = d_in.alloc(in_size)) || (rc = d_out.alloc(out_cap * val_bytes)) || (rc = d_res.alloc(sizeof(PfbDecResult))) ||
        (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    SCL_HIP_TRY(hipMemset((u8 *)d_in.p + in_bytes, 0, in_size - in_bytes));
    if (in_bytes) SCL_HIP_TRY(hipMemcpy(d_in.p, h_in, in_bytes, hipMemcpyHostToDevice));
    rc = run(PfbDecodeArgs{(const u8 *)d_in.p, in_size, 0, in_nbits, d_out.p, out_cap, (PfbDecResult *)d_res.p, d_scr.p,
                           scratch_bytes});
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    PfbDecResult res;
    SCL_HIP_TRY(hipMemcpy(&res, d_res.p, sizeof(res), hipMemcpyDeviceToHost));
    *n_out = res.n_out;
    *consumed = res.consumed;
    *status = res.status;
    if (res.n_out && (res.status == 0 || partial)) SCL_HIP_TRY(hipMemcpy(h_out, d_out.p, res.n_out * val_bytes, hipMemcpyDeviceToHost));
    return SCL_OK;
}
