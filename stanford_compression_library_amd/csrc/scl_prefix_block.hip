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
//          The scheme's code stands ONCE, in scl_bit_block.h (pfb_sync_body, pfb_scan_to_end, pfb_write_body, the host's
//          pass loop), shared with scl_lz77_entropy_wide.hip.  Owned here: the codeword policy PfbCode<FAST> over the tables
//          of a scl_prefix_model, the three kernels as thin wrappers, and the verdict of pfb_scan_groups.
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
// (PfbDecHead -- the head of the decoder's scratch, 64 bytes --, the input window and the bodies of the three kernels over a
// codeword policy: scl_bit_block.h.  Here: the policy over the tables of a scl_prefix_model, and the verdict)

// FAST: the 11-bit table and the deep nodes in LDS (byte alphabets); otherwise the node array where it is
template <bool FAST>
struct PfbCode {
    const PrefixDev &P;
    u16 *s_lut;   // [1 << PF_LUT_BITS]
    u32 *s_deep;  // [PF_DEEP_NODES]

    __device__ __forceinline__ void load() const {
        if constexpr (FAST) {
            for (u32 i = threadIdx.x; i < (1u << P.lut_bits); i += PFB_THREADS) s_lut[i] = P.d_lut[i];
            for (u32 i = threadIdx.x; i < P.n_deep; i += PFB_THREADS) s_deep[i] = P.d_deep[i];
        }
    }
    __device__ __forceinline__ u32 len_gcd() const { return P.len_gcd; }
    // Exactly what the one-lane decoders of scl_prefix.hip decide: PFB_END_EXIT, PFB_END_TRUNC (the stream cuts the
    // codeword), PFB_END_STATE (a missing child).
    __device__ __forceinline__ u32 codeword(u32 bits, u32 rem, u32 &len, u32 &sym) const {
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
};

template <bool FAST>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_sync_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                    u64 n_groups, PfbDecScratch sc, u32 pass) {
    __shared__ u16 s_lut[FAST ? (1u << PF_LUT_BITS) : 1];
    __shared__ u32 s_deep[FAST ? PF_DEEP_NODES : 1];
    pfb_sync_body(PfbCode<FAST>{P, s_lut, s_deep}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, n_groups, sc.head, sc.g,
                  pass);
}

// ONE workgroup: where the stream ends, the symbol offsets of the workgroups up to there, the result
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    pfb_scan_groups_kernel(PfbDecScratch sc, u64 n_groups, u64 in_nbits, u64 out_cap, u32 sync_passes,
                           scl_prefix_block_result *__restrict__ result) {
    u64 total;
    const u64 last_group = pfb_scan_to_end(sc.g, n_groups, &total);
    if (threadIdx.x == 0) {
        const u64 cut = sc.g.group_end[last_group];
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
    pfb_write_body(PfbCode<FAST>{P, s_lut, s_deep}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, sc.head, sc.g, out, out_cap,
                   &result->consumed);
}


// ---- host API -------------------------------------------------------------------------------------------------------------
extern "C" int scl_prefix_block_info_get(const scl_prefix_model *m, scl_prefix_block_info *info) {
    SCL_REQUIRE(m && info, "prefix_block_info_get: null argument");
    info->sub_bits = PFB_SUB;
    info->tile_symbols = PFB_TILE;
    info->code_len_gcd = m->dev.len_gcd;
    return SCL_OK;
}

// (the sizes and the layout of the scratch: pfb_enc_scratch, pfb_dec_scratch, pfb_dec_carve of scl_bit_block.h)
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
    const PfbDecScratch sc = pfb_dec_carve(d_scratch, n_groups);
    SCL_HIP_TRY(hipMemsetAsync(sc.head, 0, 64, st));
    const dim3 grid((u32)n_groups), block(PFB_THREADS);
    u32 sync_passes = 0;
    const auto sync = [&](u32 pass) {
        hipLaunchKernelGGL(pfb_sync_kernel<FAST>, grid, block, 0, st, m->dev, d_in, in_size_bytes, in_bit_offset, in_nbits, n_sub,
                           n_groups, sc, pass);
    };
    if (int rc = pfb_run_sync_passes(sync, sc.head, n_groups, st, &sync_passes)) return rc;
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
