// scl_prefix_block.hip -- prefix-free (Huffman, ...) coding of ONE large block by the whole grid, for gfx950.
//
// scl_prefix.hip gives a chunk to one lane, as every coder here does; a prefix-free stream has no state that chains a
// symbol to the one before, so a single block can use every CU and still be the reference's stream bit for bit
// (PrefixFreeEncoder.encode_block, prefix_free_compressors.py:31-50: the codewords back to back, nothing else).
// Tables are scl_prefix_model's (scl_prefix_internal.h): byte alphabets keep them in LDS, u16 alphabets read them
// where they are.  Every position and count inside a block is 64-bit; what is relative to a workgroup is 32-bit.
//
// encode   pfb_tile_bits    a workgroup sums the code lengths of its tile of PFB_TILE symbols
//          pfb_scan_tiles   ONE workgroup: exclusive 64-bit scan of the tile sums, nbits, SCL_ST_CAPACITY
//          pfb_encode_tile  a workgroup scans its tile's lengths, ORs the codewords into LDS words laid at the tile's
//                           bit offset mod 32, and stores whole big-endian words coalesced; the first and last word
//                           of a tile can be shared with its neighbours (any number of them: a tile may be a few bits)
//                           and are merged with atomicOr into the output the entry point zeroed
//          pfb_encode_tail  out_cap_bytes % 4 != 0: the bytes of the last, partial word come from scratch
// decode   Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs" (2018): the stream is cut into
//          subsequences of PFB_SUB bits, one per thread, 256 per workgroup (W = 32768 bits).  Thread i owns the
//          codewords that START in its subsequence: it decodes from its start to the first codeword boundary at or past
//          the end of the subsequence (its exit).  The true start of i is the exit of i - 1; a decoder started anywhere
//          else almost always falls into step with the true boundaries after a few codewords.
//          pfb_sync         pass 0: every thread starts at i*S rounded up to the gcd of the code lengths.  Then, under
//                           __syncthreads, a thread whose left neighbour's exit differs from its start takes it and
//                           decodes again, until no thread of the workgroup changed (<= 256 rounds: after round r
//                           threads 0..r are final).  pass p > 0: workgroup w takes the last exit of w - 1 as written by
//                           pass p - 1 (two buffers: a pass never reads what it writes) and synchronises again if that
//                           moves its start.  The host relaunches until a pass changed no workgroup's exit; after pass p
//                           workgroups 0..p are final, so n_workgroups - 1 further passes always suffice.
//          pfb_scan_groups  ONE workgroup: first workgroup whose walk ends the stream (cut codeword / missing child),
//                           exclusive 64-bit scan of the symbol counts up to it, the result triple
//          pfb_write        every thread decodes its final range once more and stores its symbols at its offset
// No kernel waits on another workgroup: no flag is spun on, no look-back, no cooperative launch -- a grid that is not
// resident all at once finishes like any other.  Every loop is bounded by the data: symbols in a tile, bits left in a
// subsequence, 256 rounds, a walk of at most 32 bits.
//
// LDS per workgroup: encode 16.4 KiB of words + 2 KiB table; decode 4 KiB + 2 KiB tables, 4.3 KiB of input, 2 KiB of
// exits.  Both far below the 40 KiB that four workgroups per CU allow (160 KiB per CU).
#include <string.h>

#include "scl_bit_block.h"
#include "scl_entry.h"
#include "scl_prefix_internal.h"
#include "scl_scan.h"

static_assert(PFB_MAX_LEN == PF_MAX_LEN, "a tile's LDS words are sized by the longest codeword");

// ---- encode ---------------------------------------------------------------------------------------------------------------
// (the shapes, PfbEncScratch -- the head of the encoder's scratch; u64 tile_bits[n_tiles] follows at byte 64 -- and the tile
// emitter: scl_bit_block.h)

// the {code, len} of the thread's PFB_PER_THREAD consecutive symbols (len 0 past the end of the block)
template <typename SYM>
__device__ __forceinline__ u32 pfb_load_codes(const PrefixDev &P, const uint2 *s_enc, const SYM *__restrict__ sym, u64 n,
                                              u64 first, uint2 (&e)[PFB_PER_THREAD], u32 &bad) {
    u32 s[PFB_PER_THREAD];
    const bool whole = first + PFB_PER_THREAD <= n && (((uintptr_t)(sym + first)) & 15) == 0;
    if (whole) {
        if constexpr (sizeof(SYM) == 1) {
            const uint4 v = *reinterpret_cast<const uint4 *>(sym + first);
            const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (u32 j = 0; j < 16; ++j) s[j] = (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
        } else {
            const uint4 v0 = *reinterpret_cast<const uint4 *>(sym + first);
            const uint4 v1 = *reinterpret_cast<const uint4 *>(sym + first + 8);
            const u32 w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (u32 j = 0; j < 16; ++j) s[j] = (w[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu;
        }
    } else {
#pragma unroll
        for (u32 j = 0; j < PFB_PER_THREAD; ++j) s[j] = first + j < n ? (u32)sym[first + j] : 0xFFFFFFFFu;
    }
    u32 bits = 0;
#pragma unroll
    for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
        const bool in = whole || first + j < n;
        u32 x = s[j];
        if (in && x >= P.K) {
            bad = 1;
            x = 0;
        }
        uint2 c = make_uint2(0u, 0u);
        if (in) {
            if constexpr (sizeof(SYM) == 1) c = s_enc[x];
            else c = P.d_enc[x];
        }
        e[j] = c;
        bits += c.y;
    }
    return bits;
}

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_tile_bits_kernel(PrefixDev P, const SYM *__restrict__ sym, u64 n, u64 *__restrict__ tile_bits,
                         u32 *__restrict__ status) {
    __shared__ uint2 s_enc[256];
    __shared__ u32 s_wave[PFB_THREADS / 64];
    const u32 tid = threadIdx.x;
    if constexpr (sizeof(SYM) == 1) {
        s_enc[tid] = tid < P.K ? P.d_enc[tid] : make_uint2(0u, 0u);
        __syncthreads();
    }
    uint2 e[PFB_PER_THREAD];
    u32 bad = 0, total;
    const u32 bits = pfb_load_codes<SYM>(P, s_enc, sym, n, (u64)blockIdx.x * PFB_TILE + tid * PFB_PER_THREAD, e, bad);
    (void)scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &total);
    const int any_bad = __syncthreads_or((int)bad);
    if (tid == 0) {
        tile_bits[blockIdx.x] = total;
        if (any_bad) atomicOr(status, (u32)SCL_ST_SYMBOL);
    }
}

__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    pfb_scan_tiles_kernel(u64 *__restrict__ tile_bits, u64 n_tiles, u64 out_cap_bytes, PfbEncScratch *__restrict__ head,
                          u64 *__restrict__ nbits, u32 *__restrict__ status) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    const u64 total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(tile_bits, n_tiles, s_wave);
    if (threadIdx.x == 0) {
        const bool fits = (total + 7) / 8 <= out_cap_bytes;
        head->fits = fits ? 1u : 0u;
        *nbits = total;
        if (!fits) atomicOr(status, (u32)SCL_ST_CAPACITY);
    }
}

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_encode_tile_kernel(PrefixDev P, const SYM *__restrict__ sym, u64 n, const u64 *__restrict__ tile_off,
                           PfbEncScratch *__restrict__ head, u32 *__restrict__ out32, u64 tail_index) {
    __shared__ uint2 s_enc[256];
    __shared__ u32 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_words[PFB_TILE_WORDS];
    if (!head->fits) return;  // SCL_ST_CAPACITY: nothing is written (uniform: the whole grid leaves)
    const u32 tid = threadIdx.x;
    if constexpr (sizeof(SYM) == 1) s_enc[tid] = tid < P.K ? P.d_enc[tid] : make_uint2(0u, 0u);
    for (u32 i = tid; i < PFB_TILE_WORDS; i += PFB_THREADS) s_words[i] = 0;
    __syncthreads();
    uint2 e[PFB_PER_THREAD];
    u32 bad = 0;
    const u32 bits = pfb_load_codes<SYM>(P, s_enc, sym, n, (u64)blockIdx.x * PFB_TILE + tid * PFB_PER_THREAD, e, bad);
    pfb_emit_tile(e, bits, tile_off[blockIdx.x], s_words, s_wave, head, out32, tail_index);
}

__global__ void pfb_encode_tail_kernel(const PfbEncScratch *__restrict__ head, const u64 *__restrict__ nbits,
                                       u8 *__restrict__ out, u64 out_cap_bytes) {
    pfb_store_tail(head, *nbits, out, out_cap_bytes);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
struct PfbDecHead {      // head of the decoder's scratch (64 bytes)
    u32 start_pass;      // the last pass in which a workgroup moved its start
    u32 exit_pass;       // the last pass in which a workgroup's last exit changed
    u64 n_total;         // pfb_scan_groups: symbols of the stream (before out_cap)
    u64 last_group;      // pfb_scan_groups: the workgroup the stream ends in
};

struct PfbDecScratch {  // device pointers into the scratch
    PfbDecHead *head;
    u32 *sub;           // [n_groups * 256] PFB_PACK
    u64 *group_exit;    // [2][n_groups] relative to the stream, PFB_NONE64: the workgroup's last thread has no exit
    u64 *group_count;   // [n_groups] symbols up to the workgroup's first cut; pfb_scan_groups: their exclusive scan
    u64 *group_end;     // [n_groups] PFB_NONE64, or (position of the codeword that ends the stream) << 2 | PFB_END_*
};

// (the input window a workgroup can reach, pfb_load_window / pfb_peek: scl_bit_block.h)

// One codeword from the left-aligned `bits`, of which `rem` >= 1 belong to the stream.  Exactly what the one-lane
// decoders of scl_prefix.hip decide: PFB_END_EXIT (a symbol of `len` bits), PFB_END_TRUNC, PFB_END_STATE.
template <bool FAST>
__device__ __forceinline__ u32 pfb_codeword(const PrefixDev &P, const u16 *s_lut, const u32 *s_deep, u32 bits, u32 rem,
                                            u32 &len, u32 &sym) {
    if constexpr (FAST) {
        const u32 T = P.lut_bits;
        const u32 e = s_lut[bits >> (32u - T)];
        const u32 kind = (e >> 4) & 3u;
        len = e & 15u;
        sym = e >> 6;
        if (len > rem) return PFB_END_TRUNC;
        if (kind == PF_KIND_SYM) return PFB_END_EXIT;
        if (kind == PF_KIND_NONE) return PFB_END_STATE;
        u32 node = sym;
        for (u32 d = T; d < PF_MAX_LEN; ++d) {
            if (d == rem) return PFB_END_TRUNC;
            const u32 next = (s_deep[node] >> (16u * ((bits >> (31u - d)) & 1u))) & 0xFFFFu;
            if (next == PF16_NONE) return PFB_END_STATE;
            if (next & PF16_LEAF) {
                sym = next & 0xFFu;
                len = d + 1;
                return PFB_END_EXIT;
            }
            node = next;
        }
        return PFB_END_STATE;  // (not reached: the tree is at most 32 deep)
    } else {
        u32 node = 0;
        for (u32 d = 0; d < PF_MAX_LEN; ++d) {
            if (d == rem) return PFB_END_TRUNC;
            const uint2 ch = P.d_nodes[node];
            const u32 next = ((bits >> (31u - d)) & 1u) ? ch.y : ch.x;
            if (next == PF_NONE) return PFB_END_STATE;
            if (next & PF_LEAF) {
                sym = next & 0xFFFFu;
                len = d + 1;
                return PFB_END_EXIT;
            }
            node = next;
        }
        return rem > PF_MAX_LEN ? PFB_END_STATE : PFB_END_TRUNC;  // (not reached)
    }
}

template <bool FAST>
__device__ __forceinline__ void pfb_load_tables(const PrefixDev &P, u16 *s_lut, u32 *s_deep) {
    if constexpr (FAST) {
        for (u32 i = threadIdx.x; i < (1u << P.lut_bits); i += PFB_THREADS) s_lut[i] = P.d_lut[i];
        for (u32 i = threadIdx.x; i < P.n_deep; i += PFB_THREADS) s_deep[i] = P.d_deep[i];
    }
}

// Positions below are relative to the workgroup's first bit (32-bit): `avail` = bits of the stream from there on, clamped
// to W + 64, which no walk reaches; `shift` = bit of the window's first word at which the workgroup starts.
// Walks from `start` to the first boundary at or past `stop`; returns how the walk ended and where.
template <bool FAST>
__device__ __forceinline__ u32 pfb_walk(const PrefixDev &P, const u16 *s_lut, const u32 *s_deep, const u32 *s_win, u32 shift,
                                        u32 start, u32 stop, u32 avail, u32 &count, u32 &end) {
    u32 pos = start, n = 0, kind = PFB_END_EXIT;
    while (pos < stop) {  // every turn moves pos forward by a codeword or leaves
        u32 len, sym;
        kind = pfb_codeword<FAST>(P, s_lut, s_deep, pfb_peek(s_win, shift + pos), avail - pos, len, sym);
        if (kind != PFB_END_EXIT) break;
        pos += len;
        ++n;
    }
    count = n;
    end = pos;
    return kind;
}

template <bool FAST>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_sync_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                    u64 n_groups, PfbDecScratch sc, u32 pass) {
    __shared__ u16 s_lut[FAST ? (1u << PF_LUT_BITS) : 1];
    __shared__ u32 s_deep[FAST ? PF_DEEP_NODES : 1];
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
    const u64 left64 = in_nbits - group_bit;
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
            const u32 g = P.len_gcd;
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
    pfb_load_tables<FAST>(P, s_lut, s_deep);
    const u64 first_bit = in_bit_offset + group_bit;
    pfb_load_window(s_win, in, in_size_bytes, first_bit);
    __syncthreads();
    const u32 shift = (u32)(first_bit & 31u);
    if (pass == 0 && active) kind = pfb_walk<FAST>(P, s_lut, s_deep, s_win, shift, start, stop, avail, count, end);
    s_exit[tid] = active && kind == PFB_END_EXIT ? end : 0xFFFFFFFFu;
    __syncthreads();
    // after round r threads 0..r are final: thread r's left neighbour was final when it read its exit
    for (u32 round = 0; round < PFB_THREADS; ++round) {
        const u32 left = tid ? s_exit[tid - 1] : from_left;
        __syncthreads();  // every exit is read before any is written
        const bool moved = active && left != 0xFFFFFFFFu && left != start;
        if (moved) {
            start = left;
            kind = pfb_walk<FAST>(P, s_lut, s_deep, s_win, shift, start, stop, avail, count, end);
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
            sc.head->start_pass = pass;  // this workgroup moved its start
            if (ex != exit_in[group]) sc.head->exit_pass = pass;
        }
        exit_out[group] = ex;
    }
}

// ONE workgroup: where the stream ends, the symbol offsets of the workgroups up to there, the result
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    pfb_scan_groups_kernel(PfbDecScratch sc, u64 n_groups, u64 in_nbits, u64 out_cap, u32 sync_passes,
                           scl_prefix_block_result *__restrict__ result) {
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
    const u64 total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(sc.group_count, last_group + 1, s_wave);
    if (threadIdx.x == 0) {
        const u64 cut = sc.group_end[last_group];
        const u64 end = cut == PFB_NONE64 ? in_nbits : cut >> 2;
        u32 status = cut == PFB_NONE64 ? 0u : ((cut & 3u) == PFB_END_TRUNC ? SCL_ST_TRUNCATED : SCL_ST_STATE);
        u64 consumed = end;
        // the one-lane decoder looks at out_cap before every codeword: bits left after out_cap symbols are
        // SCL_ST_CAPACITY whatever they hold.  total > out_cap: pfb_write stores `consumed` (0 for out_cap = 0)
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

template <typename SYM, bool FAST>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_write_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                     PfbDecScratch sc, SYM *__restrict__ out, u64 out_cap, scl_prefix_block_result *__restrict__ result) {
    __shared__ u16 s_lut[FAST ? (1u << PF_LUT_BITS) : 1];
    __shared__ u32 s_deep[FAST ? PF_DEEP_NODES : 1];
    __shared__ u32 s_win[PFB_WIN_LDS];
    __shared__ u64 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_first_cut;
    const u32 tid = threadIdx.x;
    const u64 group = blockIdx.x;
    if (group > sc.head->last_group) return;  // behind the end of the stream (uniform)
    const u64 group_first = sc.group_count[group];
    if (group_first >= out_cap) return;  // nothing of this workgroup is stored (uniform)
    const u64 n_total = sc.head->n_total;
    const u64 group_bit = group * PFB_GROUP;
    const u64 sub_index = group * PFB_THREADS + tid;
    const bool active = sub_index < n_sub;
    const u64 left64 = in_nbits - group_bit;
    const u32 avail = (u32)(left64 < PFB_GROUP + 64u ? left64 : PFB_GROUP + 64u);
    const u32 packed = active ? sc.sub[sub_index] : 0u;
    const u32 kind = (packed >> 15) & 3u;
    if (tid == 0) s_first_cut = PFB_THREADS;
    pfb_load_tables<FAST>(P, s_lut, s_deep);
    const u64 first_bit = in_bit_offset + group_bit;
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
        if (pfb_codeword<FAST>(P, s_lut, s_deep, pfb_peek(s_win, shift + pos), avail - pos, len, sym) != PFB_END_EXIT)
            break;  // (not reached: the same walk counted these symbols)
        pos += len;
        out[index] = (SYM)sym;
        if (index + 1 == out_cap && n_total > out_cap) result->consumed = group_bit + pos;
    }
}

// ---- host API -------------------------------------------------------------------------------------------------------------
extern "C" int scl_prefix_block_info_get(const scl_prefix_model *m, scl_prefix_block_info *info) {
    SCL_REQUIRE(m && info, "prefix_block_info_get: null argument");
    info->sub_bits = PFB_SUB;
    info->tile_symbols = PFB_TILE;
    info->code_len_gcd = m->dev.len_gcd;
    return SCL_OK;
}

static u64 pfb_tiles(u64 n) { return (n + PFB_TILE - 1) / PFB_TILE; }
static u64 pfb_subs(u64 nbits) { return (nbits + PFB_SUB - 1) / PFB_SUB; }
static u64 pfb_groups(u64 nbits) { return (pfb_subs(nbits) + PFB_THREADS - 1) / PFB_THREADS; }
static u64 pfb_enc_scratch(u64 n) { return 64 + pfb_tiles(n) * 8; }
static u64 pfb_dec_scratch(u64 nbits) {
    const u64 g = pfb_groups(nbits);
    return 64 + g * (PFB_THREADS * 4 + 4 * 8);
}

extern "C" uint64_t scl_prefix_block_scratch_bytes(const scl_prefix_model *m, uint64_t n_symbols, uint64_t in_nbits) {
    if (!m) return 0;
    const u64 e = pfb_enc_scratch(n_symbols), d = pfb_dec_scratch(in_nbits);
    return scl_round_up(e > d ? e : d, 256);
}

template <class SYM>
static int pfb_encode(const char *what, const scl_prefix_model *m, const SYM *d_sym, u64 n, u8 *d_out, u64 out_cap_bytes,
                      u64 *d_nbits, u32 *d_status, void *d_scratch, u64 scratch_bytes, hipStream_t st) {
    SCL_REQUIRE(m && d_out && d_nbits && d_status && d_scratch && (d_sym || n == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(sizeof(SYM) == 2 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K, what);
    if (int rc = scl_check_device(m->device, what)) return rc;
    SCL_REQUIRE(n < (1ull << 32), "%s: %llu symbols: a block holds fewer than 2^32", what, (unsigned long long)n);
    SCL_REQUIRE(((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_nbits & 7) == 0 &&
                    ((uintptr_t)d_sym & (sizeof(SYM) - 1)) == 0,
                "%s: d_out must be 4-byte, d_scratch and d_nbits 8-byte aligned", what);
    SCL_REQUIRE(scratch_bytes >= pfb_enc_scratch(n), "%s: scratch of %llu bytes, scl_prefix_block_scratch_bytes asks for %llu",
                what, (unsigned long long)scratch_bytes, (unsigned long long)pfb_enc_scratch(n));
    SCL_HIP_TRY(hipMemsetAsync(d_nbits, 0, 8, st));
    SCL_HIP_TRY(hipMemsetAsync(d_status, 0, 4, st));
    if (n == 0) return SCL_OK;
    PfbEncScratch *head = (PfbEncScratch *)d_scratch;
    u64 *tile_bits = (u64 *)((u8 *)d_scratch + 64);
    const u64 n_tiles = pfb_tiles(n);
    // the tiles OR their shared words in: zero what the longest possible stream can reach
    const u64 reach = scl_round_up((n * m->dev.max_len + 7) / 8, 4);
    const u64 zeroed = reach < out_cap_bytes ? reach : out_cap_bytes;
    if (zeroed) SCL_HIP_TRY(hipMemsetAsync(d_out, 0, zeroed, st));
    SCL_HIP_TRY(hipMemsetAsync(head, 0, 64, st));
    hipLaunchKernelGGL(pfb_tile_bits_kernel<SYM>, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, m->dev, d_sym, n, tile_bits,
                       d_status);
    hipLaunchKernelGGL(pfb_scan_tiles_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, tile_bits, n_tiles, out_cap_bytes, head,
                       d_nbits, d_status);
    const u64 tail_index = (out_cap_bytes & 3) ? out_cap_bytes >> 2 : PFB_NONE64;
    hipLaunchKernelGGL(pfb_encode_tile_kernel<SYM>, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, m->dev, d_sym, n,
                       (const u64 *)tile_bits, head, (u32 *)d_out, tail_index);
    if (out_cap_bytes & 3)
        hipLaunchKernelGGL(pfb_encode_tail_kernel, dim3(1), dim3(1), 0, st, (const PfbEncScratch *)head, (const u64 *)d_nbits,
                           d_out, out_cap_bytes);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class SYM, bool FAST>
static int pfb_decode_run(const scl_prefix_model *m, const u8 *d_in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits,
                          SYM *d_out_sym, u64 out_cap, scl_prefix_block_result *d_result, void *d_scratch, hipStream_t st) {
    const u64 n_sub = pfb_subs(in_nbits), n_groups = pfb_groups(in_nbits);
    PfbDecScratch sc;
    u8 *p = (u8 *)d_scratch;
    sc.head = (PfbDecHead *)p;
    sc.group_exit = (u64 *)(p + 64);
    sc.group_count = sc.group_exit + 2 * n_groups;
    sc.group_end = sc.group_count + n_groups;
    sc.sub = (u32 *)(sc.group_end + n_groups);
    SCL_HIP_TRY(hipMemsetAsync(sc.head, 0, 64, st));
    const dim3 grid((u32)n_groups), block(PFB_THREADS);
    hipLaunchKernelGGL(pfb_sync_kernel<FAST>, grid, block, 0, st, m->dev, d_in, in_size_bytes, in_bit_offset, in_nbits, n_sub,
                       n_groups, sc, 0u);
    SCL_HIP_TRY(hipGetLastError());
    // workgroup w is final after pass w: passes 1 .. n_groups - 1 at the most, fewer when a pass changes no exit
    u32 sync_passes = 0;
    for (u64 pass = 1; pass < n_groups; ++pass) {
        hipLaunchKernelGGL(pfb_sync_kernel<FAST>, grid, block, 0, st, m->dev, d_in, in_size_bytes, in_bit_offset, in_nbits,
                           n_sub, n_groups, sc, (u32)pass);
        SCL_HIP_TRY(hipGetLastError());
        u32 flags[2];  // {start_pass, exit_pass}
        SCL_HIP_TRY(hipMemcpyAsync(flags, sc.head, 8, hipMemcpyDeviceToHost, st));
        SCL_HIP_TRY(hipStreamSynchronize(st));
        if (flags[0] == (u32)pass) ++sync_passes;
        if (flags[1] != (u32)pass) break;
    }
    hipLaunchKernelGGL(pfb_scan_groups_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, n_groups, in_nbits, out_cap,
                       sync_passes, d_result);
    hipLaunchKernelGGL((pfb_write_kernel<SYM, FAST>), grid, block, 0, st, m->dev, d_in, in_size_bytes, in_bit_offset, in_nbits,
                       n_sub, sc, d_out_sym, out_cap, d_result);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

template <class SYM>
static int pfb_decode(const char *what, const scl_prefix_model *m, const u8 *d_in, u64 in_size_bytes, u64 in_bit_offset,
                      u64 in_nbits, SYM *d_out_sym, u64 out_cap, scl_prefix_block_result *d_result, void *d_scratch,
                      u64 scratch_bytes, hipStream_t st) {
    SCL_REQUIRE(m && d_in && d_result && d_scratch && (d_out_sym || out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(sizeof(SYM) == 2 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K, what);
    if (int rc = scl_check_device(m->device, what)) return rc;
    SCL_REQUIRE(in_nbits < (1ull << 46) && in_bit_offset < (1ull << 62), "%s: stream of %llu bits: 2^46 and more are not coded",
                what, (unsigned long long)in_nbits);
    SCL_REQUIRE(((uintptr_t)d_in & 3) == 0 && ((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_result & 7) == 0 &&
                    ((uintptr_t)d_out_sym & (sizeof(SYM) - 1)) == 0,
                "%s: d_in must be 4-byte, d_scratch and d_result 8-byte aligned", what);
    SCL_REQUIRE(scratch_bytes >= pfb_dec_scratch(in_nbits),
                "%s: scratch of %llu bytes, scl_prefix_block_scratch_bytes asks for %llu", what,
                (unsigned long long)scratch_bytes, (unsigned long long)pfb_dec_scratch(in_nbits));
    SCL_REQUIRE((in_bit_offset + in_nbits + 7) / 8 <= in_size_bytes, "%s: the stream ends behind in_size_bytes", what);
    if (in_nbits == 0) {  // an empty stream: zero symbols, nothing is launched
        SCL_HIP_TRY(hipMemsetAsync(d_result, 0, sizeof(scl_prefix_block_result), st));
        return SCL_OK;
    }
    if constexpr (sizeof(SYM) == 1) {
        if (m->fast && !scl_force_generic())
            return pfb_decode_run<SYM, true>(m, d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, d_result,
                                             d_scratch, st);
    }
    return pfb_decode_run<SYM, false>(m, d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, d_result, d_scratch,
                                      st);
}

extern "C" int scl_prefix_encode_block(const scl_prefix_model *m, const uint8_t *d_sym, uint64_t n, uint8_t *d_out,
                                       uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                       uint64_t scratch_bytes, void *stream) {
    return pfb_encode<u8>("prefix_encode_block", m, d_sym, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch,
                          scratch_bytes, (hipStream_t)stream);
}

extern "C" int scl_prefix_encode_block_u16(const scl_prefix_model *m, const uint16_t *d_sym, uint64_t n, uint8_t *d_out,
                                           uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                           uint64_t scratch_bytes, void *stream) {
    return pfb_encode<u16>("prefix_encode_block_u16", m, d_sym, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch,
                           scratch_bytes, (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_block(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                       uint64_t in_bit_offset, uint64_t in_nbits, uint8_t *d_out_sym, uint64_t out_cap,
                                       scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                       void *stream) {
    return pfb_decode<u8>("prefix_decode_block", m, d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, d_result,
                          d_scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_block_u16(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                           uint64_t in_bit_offset, uint64_t in_nbits, uint16_t *d_out_sym, uint64_t out_cap,
                                           scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                           void *stream) {
    return pfb_decode<u16>("prefix_decode_block_u16", m, d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap,
                           d_result, d_scratch, scratch_bytes, (hipStream_t)stream);
}

// ---- one block in host memory ---------------------------------------------------------------------------------------------
template <class SYM>
static int pfb_encode_host(const char *what, const scl_prefix_model *m, const SYM *h_sym, u64 n, u8 *h_out, u64 out_cap_bytes,
                           u64 *nbits) {
    SCL_REQUIRE(m && h_out && nbits && (h_sym || n == 0), "%s: null argument", what);
    SCL_REQUIRE(n < (1ull << 32), "%s: %llu symbols: a block holds fewer than 2^32", what, (unsigned long long)n);
    const u64 reach = scl_round_up((n * m->dev.max_len + 7) / 8, 4);
    const u64 cap = reach < out_cap_bytes ? reach : out_cap_bytes;  // no stream of n symbols is longer than `reach`
    const u64 scratch_bytes = pfb_enc_scratch(n);
    ScratchDev d_sym, d_out, d_meta, d_scr;
    int rc;
    if ((rc = d_sym.alloc(n * sizeof(SYM))) || (rc = d_out.alloc(cap)) || (rc = d_meta.alloc(16)) ||
        (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    if (n) SCL_HIP_TRY(hipMemcpy(d_sym.p, h_sym, n * sizeof(SYM), hipMemcpyHostToDevice));
    rc = pfb_encode<SYM>(what, m, (const SYM *)d_sym.p, n, (u8 *)d_out.p, cap, (u64 *)d_meta.p, (u32 *)d_meta.p + 2, d_scr.p,
                         scratch_bytes, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    u64 meta[2];
    SCL_HIP_TRY(hipMemcpy(meta, d_meta.p, 16, hipMemcpyDeviceToHost));
    const u32 status = (u32)meta[1];
    const u64 bytes = (meta[0] + 7) / 8;
    if (bytes > out_cap_bytes) {
        scl_set_error("%s: output needs %llu bytes, capacity %llu", what, (unsigned long long)bytes,
                      (unsigned long long)out_cap_bytes);
        return SCL_E_PARAM;
    }
    if ((rc = scl_status_to_error(status, what))) return rc;
    if (bytes) SCL_HIP_TRY(hipMemcpy(h_out, d_out.p, bytes, hipMemcpyDeviceToHost));
    *nbits = meta[0];
    return SCL_OK;
}

template <class SYM>
static int pfb_decode_host(const char *what, const scl_prefix_model *m, const u8 *h_in, u64 in_nbits, SYM *h_out_sym,
                           u64 out_cap, u64 *n_out, u64 *consumed) {
    SCL_REQUIRE(m && h_in && n_out && consumed && (h_out_sym || out_cap == 0), "%s: null argument", what);
    SCL_REQUIRE(in_nbits < (1ull << 46), "%s: stream of %llu bits: 2^46 and more are not coded", what,
                (unsigned long long)in_nbits);
    const u64 in_bytes = (in_nbits + 7) / 8, in_size = scl_round_up(in_bytes, 4) + 4;
    const u64 scratch_bytes = pfb_dec_scratch(in_nbits);
    ScratchDev d_in, d_out, d_res, d_scr;
    int rc;
    if ((rc = d_in.alloc(in_size)) || (rc = d_out.alloc(out_cap * sizeof(SYM))) ||
        (rc = d_res.alloc(sizeof(scl_prefix_block_result))) || (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    SCL_HIP_TRY(hipMemset((u8 *)d_in.p + (in_size - 4), 0, 4));  // the bytes behind the stream that a word load reaches
    if (in_bytes) SCL_HIP_TRY(hipMemcpy(d_in.p, h_in, in_bytes, hipMemcpyHostToDevice));
    rc = pfb_decode<SYM>(what, m, (const u8 *)d_in.p, in_size, 0, in_nbits, (SYM *)d_out.p, out_cap,
                         (scl_prefix_block_result *)d_res.p, d_scr.p, scratch_bytes, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    scl_prefix_block_result res;
    SCL_HIP_TRY(hipMemcpy(&res, d_res.p, sizeof(res), hipMemcpyDeviceToHost));
    *n_out = res.n_out;
    *consumed = res.consumed;
    if ((rc = scl_status_to_error(res.status, what))) return rc;
    if (res.n_out) SCL_HIP_TRY(hipMemcpy(h_out_sym, d_out.p, res.n_out * sizeof(SYM), hipMemcpyDeviceToHost));
    return SCL_OK;
}

extern "C" int scl_prefix_encode_block_host(const scl_prefix_model *m, const uint8_t *h_sym, uint64_t n, uint8_t *h_out,
                                            uint64_t out_cap_bytes, uint64_t *nbits) {
    return pfb_encode_host<u8>("prefix_encode_block_host", m, h_sym, n, h_out, out_cap_bytes, nbits);
}

extern "C" int scl_prefix_decode_block_host(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                            uint8_t *h_out_sym, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed) {
    return pfb_decode_host<u8>("prefix_decode_block_host", m, h_in, in_nbits, h_out_sym, out_cap, n_out, consumed);
}

extern "C" int scl_prefix_encode_block_host_u16(const scl_prefix_model *m, const uint16_t *h_sym, uint64_t n, uint8_t *h_out,
                                                uint64_t out_cap_bytes, uint64_t *nbits) {
    return pfb_encode_host<u16>("prefix_encode_block_host_u16", m, h_sym, n, h_out, out_cap_bytes, nbits);
}

extern "C" int scl_prefix_decode_block_host_u16(const scl_prefix_model *m, const uint8_t *h_in, uint64_t in_nbits,
                                                uint16_t *h_out_sym, uint64_t out_cap, uint64_t *n_out,
                                                uint64_t *consumed) {
    return pfb_decode_host<u16>("prefix_decode_block_host_u16", m, h_in, in_nbits, h_out_sym, out_cap, n_out, consumed);
}
