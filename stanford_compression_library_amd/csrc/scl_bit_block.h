// scl_bit_block.h -- the pieces of "one block of variable-length codewords across the whole grid" that do not depend on
// whose codewords they are: the shapes, the encoder's tile emitter and the decoder's input window.  ONE copy, used by
// scl_prefix_block.hip (one prefix-free block, tables of a scl_prefix_model) and by scl_lz77_entropy_wide.hip (the four
// fields of an LZ77 stream at any bit position, tables built on the device).  Internal to csrc/; DESIGN.md 3.5.1, 3.6.3.
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

// out_cap_bytes % 4 != 0: the bytes of the last, partial word come from head->tail_word (one thread)
__device__ __forceinline__ void pfb_store_tail(const PfbEncScratch *__restrict__ head, u64 nbits, u8 *__restrict__ out,
                                               u64 out_cap_bytes) {
    if (!head->fits || ((nbits + 31) >> 5) <= (out_cap_bytes >> 2)) return;  // nothing written, or not as far as that word
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
#endif  // __HIPCC__
