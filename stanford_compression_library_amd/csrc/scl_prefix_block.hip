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
// All of it stands ONCE, in scl_bit_block.h, shared with scl_uint_block.hip and scl_lz77_entropy_wide.hip: the bodies of
// the kernels over a policy, the kernels without one (pfb_scan_tiles, pfb_encode_tail, pfb_scan_groups), the entry points'
// checks and launches, the staging of a block in host memory.  Owned here: the value policy PfbEnc<SYM> and the codeword
// policy PfbCode<FAST> over the tables of a scl_prefix_model, the four kernels over them as thin wrappers, the model checks.
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
// the value policy of pfb_tile_bits_body / pfb_encode_tile_body: byte alphabets keep the code table in LDS
template <typename SYM>
struct PfbEnc {
    const PrefixDev &P;
    const SYM *__restrict__ sym;
    u64 n;
    const u64 *tile_off;  // the scanned tile sums (tile-emit)
    uint2 *s_enc;         // [256]
    static constexpr bool kTables = sizeof(SYM) == 1;
    static constexpr u32 kFault = SCL_ST_SYMBOL;

    __device__ __forceinline__ void load() const {
        if constexpr (kTables) s_enc[threadIdx.x] = threadIdx.x < P.K ? P.d_enc[threadIdx.x] : make_uint2(0u, 0u);
    }
    __device__ __forceinline__ u64 tile_base(u32 block) const { return tile_off[block]; }
    // the {code, len} of the thread's PFB_PER_THREAD consecutive symbols (len 0 past the end of the block)
    __device__ __forceinline__ u32 codes(u32 block, uint2 (&e)[PFB_PER_THREAD], u32 &bad) const {
        const u64 first = (u64)block * PFB_TILE + threadIdx.x * PFB_PER_THREAD;
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
};

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_tile_bits_kernel(PrefixDev P, const SYM *__restrict__ sym, u64 n, u64 *__restrict__ tile_bits,
                         u32 *__restrict__ status) {
    __shared__ uint2 s_enc[256];
    pfb_tile_bits_body(PfbEnc<SYM>{P, sym, n, nullptr, s_enc}, tile_bits, status);
}

template <typename SYM>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_encode_tile_kernel(PrefixDev P, const SYM *__restrict__ sym, u64 n, const u64 *__restrict__ tile_off,
                           PfbEncScratch *__restrict__ head, u32 *__restrict__ out32, u64 tail_index) {
    __shared__ uint2 s_enc[256];
    pfb_encode_tile_body(PfbEnc<SYM>{P, sym, n, tile_off, s_enc}, head, out32, tail_index);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
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

template <typename SYM, bool FAST>
__global__ void __launch_bounds__(PFB_THREADS, 4)
    pfb_write_kernel(PrefixDev P, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                     PfbDecScratch sc, SYM *__restrict__ out, u64 out_cap, PfbDecResult *__restrict__ result) {
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

PFB_RESULT_IS(scl_prefix_block_result);
static const PfbWords PFB_WORDS = {"symbols", "scl_prefix_block_scratch_bytes",
                                   "d_out must be 4-byte, d_scratch and d_nbits 8-byte aligned",
                                   "d_in must be 4-byte, d_scratch and d_result 8-byte aligned"};

// the bytes of the longest stream of n symbols
static u64 pfb_reach(const scl_prefix_model *m, u64 n) { return scl_round_up((n * m->dev.max_len + 7) / 8, 4); }

// what every call checks of its model in front of the shared launchers (scl_bit_block.h)
template <class SYM>
static int pfb_check_model(const char *what, const scl_prefix_model *m) {
    SCL_REQUIRE(m, "%s: null pointer argument", what);
    SCL_REQUIRE(sizeof(SYM) == 2 || m->dev.K <= 256, "%s: alphabet of %u symbols: use scl_%s_u16", what, m->dev.K, what);
    return scl_check_device(m->device, what);
}

template <class SYM>
static int pfb_encode(const char *what, const scl_prefix_model *m, const PfbEncodeArgs &a, hipStream_t st) {
    if (int rc = pfb_check_model<SYM>(what, m)) return rc;
    const SYM *d_sym = (const SYM *)a.d_val;
    return pfb_encode_launch<0u>(
        what, PFB_WORDS, a, ((uintptr_t)d_sym & (sizeof(SYM) - 1)) == 0, pfb_reach(m, a.n), st,
        [&](dim3 grid, u64 *tile_bits, u32 *status) {
            hipLaunchKernelGGL(pfb_tile_bits_kernel<SYM>, grid, dim3(PFB_THREADS), 0, st, m->dev, d_sym, a.n, tile_bits, status);
        },
        [&](dim3 grid, const u64 *tile_off, PfbEncScratch *head, u32 *out32, u64 tail_index) {
            hipLaunchKernelGGL(pfb_encode_tile_kernel<SYM>, grid, dim3(PFB_THREADS), 0, st, m->dev, d_sym, a.n, tile_off, head,
                               out32, tail_index);
        });
}

template <class SYM, bool FAST>
static int pfb_decode_run(const char *what, const scl_prefix_model *m, const PfbDecodeArgs &a, hipStream_t st) {
    return pfb_decode_launch<SCL_ST_STATE>(
        what, PFB_WORDS, a, ((uintptr_t)a.d_out & (sizeof(SYM) - 1)) == 0, st,
        [&](dim3 grid, u64 n_sub, u64 n_groups, const PfbDecScratch &sc, u32 pass) {
            hipLaunchKernelGGL(pfb_sync_kernel<FAST>, grid, dim3(PFB_THREADS), 0, st, m->dev, a.d_in, a.in_size_bytes,
                               a.in_bit_offset, a.in_nbits, n_sub, n_groups, sc, pass);
        },
        [&](dim3 grid, u64 n_sub, const PfbDecScratch &sc) {
            hipLaunchKernelGGL((pfb_write_kernel<SYM, FAST>), grid, dim3(PFB_THREADS), 0, st, m->dev, a.d_in, a.in_size_bytes,
                               a.in_bit_offset, a.in_nbits, n_sub, sc, (SYM *)a.d_out, a.out_cap, a.d_result);
        });
}

template <class SYM>
static int pfb_decode(const char *what, const scl_prefix_model *m, const PfbDecodeArgs &a, hipStream_t st) {
    if (int rc = pfb_check_model<SYM>(what, m)) return rc;
    if constexpr (sizeof(SYM) == 1) {
        if (m->fast && !scl_force_generic()) return pfb_decode_run<SYM, true>(what, m, a, st);
    }
    return pfb_decode_run<SYM, false>(what, m, a, st);
}

extern "C" int scl_prefix_encode_block(const scl_prefix_model *m, const uint8_t *d_sym, uint64_t n, uint8_t *d_out,
                                       uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                       uint64_t scratch_bytes, void *stream) {
    return pfb_encode<u8>("prefix_encode_block", m, {d_sym, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch, scratch_bytes},
                          (hipStream_t)stream);
}

extern "C" int scl_prefix_encode_block_u16(const scl_prefix_model *m, const uint16_t *d_sym, uint64_t n, uint8_t *d_out,
                                           uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                           uint64_t scratch_bytes, void *stream) {
    return pfb_encode<u16>("prefix_encode_block_u16", m,
                           {d_sym, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch, scratch_bytes}, (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_block(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                       uint64_t in_bit_offset, uint64_t in_nbits, uint8_t *d_out_sym, uint64_t out_cap,
                                       scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                       void *stream) {
    return pfb_decode<u8>("prefix_decode_block", m,
                          {d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, (PfbDecResult *)d_result, d_scratch,
                           scratch_bytes},
                          (hipStream_t)stream);
}

extern "C" int scl_prefix_decode_block_u16(const scl_prefix_model *m, const uint8_t *d_in, uint64_t in_size_bytes,
                                           uint64_t in_bit_offset, uint64_t in_nbits, uint16_t *d_out_sym, uint64_t out_cap,
                                           scl_prefix_block_result *d_result, void *d_scratch, uint64_t scratch_bytes,
                                           void *stream) {
    return pfb_decode<u16>("prefix_decode_block_u16", m,
                           {d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_sym, out_cap, (PfbDecResult *)d_result, d_scratch,
                            scratch_bytes},
                           (hipStream_t)stream);
}

// ---- one block in host memory (the staging: scl_bit_block.h); a status is an error here ------------------------------------
template <class SYM>
static int pfb_encode_host(const char *what, const scl_prefix_model *m, const SYM *h_sym, u64 n, u8 *h_out, u64 out_cap_bytes,
                           u64 *nbits) {
    SCL_REQUIRE(m && h_out && nbits && (h_sym || n == 0), "%s: null argument", what);
    u64 coded;
    u32 status;
    int rc = pfb_encode_staged(what, PFB_WORDS, h_sym, n, sizeof(SYM), pfb_reach(m, n), h_out, out_cap_bytes, &coded, &status,
                               [&](const PfbEncodeArgs &a) { return pfb_encode<SYM>(what, m, a, nullptr); });
    if (rc || (rc = scl_status_to_error(status, what))) return rc;
    *nbits = coded;
    return SCL_OK;
}

template <class SYM>
static int pfb_decode_host(const char *what, const scl_prefix_model *m, const u8 *h_in, u64 in_nbits, SYM *h_out_sym,
                           u64 out_cap, u64 *n_out, u64 *consumed) {
    SCL_REQUIRE(m && h_in && n_out && consumed && (h_out_sym || out_cap == 0), "%s: null argument", what);
    u32 status;
    int rc = pfb_decode_staged(what, h_in, in_nbits, h_out_sym, sizeof(SYM), out_cap, false, n_out, consumed, &status,
                               [&](const PfbDecodeArgs &a) { return pfb_decode<SYM>(what, m, a, nullptr); });
    return rc ? rc : scl_status_to_error(status, what);
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
