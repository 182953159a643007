// scl_uint_block.hip -- Golomb, universal and Elias-delta coding of ONE block of uint32 values by the whole grid, for gfx950.
//
// The third user of scl_bit_block.h, beside scl_prefix_block.hip and scl_lz77_entropy_wide.hip, and the thinnest: the
// alphabet is unbounded, so no table sits in LDS -- the codeword policy is the rule of scl_uint_code.h, computed per value
// (encode) and per 32-bit look (decode: one count of leading bits and a shift).  The stream is the reference's: the codewords
// of GolombUintEncoder(M) / UniversalUintEncoder / EliasDeltaUintEncoder back to back, nothing else.
//
// encode   ub_tile_bits     pfb_tile_bits_body: the codeword lengths of a tile; SCL_ST_SIZE for a codeword above 32 bits
//          (scan, tail)     pfb_scan_tiles_kernel<SCL_ST_SIZE>: SIZE stops the coding (nbits 0, nothing fits, the capacity is not
//                           looked at), else nbits, the fits flag, SCL_ST_CAPACITY; pfb_encode_tail_kernel
//          ub_encode_tile   pfb_encode_tile_body: pfb_emit_tile on the tile's codewords (nothing on SCL_ST_SIZE / SCL_ST_CAPACITY)
// decode   ub_sync          pfb_sync_body, relaunched by pfb_decode_section
//          (verdict)        pfb_scan_groups_kernel<SCL_ST_SIZE>: a cut codeword is SCL_ST_TRUNCATED, a prefix that announces
//                           more than 32 bits SCL_ST_SIZE (the status the LZ77 entropy stage gives such a codeword)
//          ub_write         pfb_write_body with uint32 symbols
// Owned here: the two policies, the four kernels over them, the two rule probes and the extern "C" wrappers; the checks, the
// launches and the staging of a block in host memory are scl_bit_block.h's.
// As in scl_prefix_block.hip no kernel waits on another workgroup: every dependency between workgroups is a kernel boundary.
// LDS per workgroup: encode 16.4 KiB of words; decode 4.3 KiB of input and 1 KiB of exits.  DESIGN.md 3.5.2.
#include "scl_bit_block.h"
#include "scl_uint_code.h"

// ---- encode ---------------------------------------------------------------------------------------------------------------
// the value policy of pfb_tile_bits_body / pfb_encode_tile_body: the rule, no table
struct UbEnc {
    SclUintRule C;
    const u32 *__restrict__ val;
    u64 n;
    const u64 *tile_off;  // the scanned tile sums (tile-emit)
    static constexpr bool kTables = false;
    static constexpr u32 kFault = SCL_ST_SIZE;

    __device__ __forceinline__ void load() const {}
    __device__ __forceinline__ u64 tile_base(u32 block) const { return tile_off[block]; }
    // the {bits, length} of the thread's PFB_PER_THREAD consecutive values (length 0 past the end of the block)
    __device__ __forceinline__ u32 codes(u32 block, uint2 (&e)[PFB_PER_THREAD], u32 &bad) const {
        const u64 first = (u64)block * PFB_TILE + threadIdx.x * PFB_PER_THREAD;
        u32 v[PFB_PER_THREAD];
        const bool whole = first + PFB_PER_THREAD <= n && (((uintptr_t)(val + first)) & 15) == 0;
        if (whole) {
#pragma unroll
            for (u32 k = 0; k < PFB_PER_THREAD / 4; ++k) {
                const uint4 q = *reinterpret_cast<const uint4 *>(val + first + 4 * k);
                v[4 * k] = q.x, v[4 * k + 1] = q.y, v[4 * k + 2] = q.z, v[4 * k + 3] = q.w;
            }
        } else {
#pragma unroll
            for (u32 j = 0; j < PFB_PER_THREAD; ++j) v[j] = first + j < n ? val[first + j] : 0u;
        }
        u32 bits = 0;
#pragma unroll
        for (u32 j = 0; j < PFB_PER_THREAD; ++j) {
            uint2 c = make_uint2(0u, 0u);
            if (whole || first + j < n) {
                const SclUintWord w = scl_uint_codeword(C, v[j]);
                c = make_uint2(w.bits, w.len);
                if (w.len == 0) bad = 1;  // a value of the block without a codeword of 32 bits
            }
            e[j] = c;
            bits += c.y;
        }
        return bits;
    }
};

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_tile_bits_kernel(SclUintRule C, const u32 *__restrict__ val, u64 n, u64 *__restrict__ tile_bits,
                        u32 *__restrict__ status) {
    pfb_tile_bits_body(UbEnc{C, val, n, nullptr}, tile_bits, status);
}

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_encode_tile_kernel(SclUintRule C, const u32 *__restrict__ val, u64 n, const u64 *__restrict__ tile_off,
                          PfbEncScratch *__restrict__ head, u32 *__restrict__ out32, u64 tail_index) {
    pfb_encode_tile_body(UbEnc{C, val, n, tile_off}, head, out32, tail_index);
}

// ---- decode ---------------------------------------------------------------------------------------------------------------
// the codeword policy of pfb_sync_body / pfb_write_body: the rule, no table
struct UbCode {
    SclUintRule C;
    __device__ __forceinline__ void load() const {}
    // every universal codeword has an even length: pass 0 starts on even bits and is exact
    __device__ __forceinline__ u32 len_gcd() const { return C.kind == SCL_UINT_UNIVERSAL ? 2u : 1u; }
    __device__ __forceinline__ u32 codeword(u32 bits, u32 rem, u32 &len, u32 &sym) const {
        return scl_uint_decode(C, bits, rem, len, sym);
    }
};

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_sync_kernel(SclUintRule C, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                   u64 n_groups, PfbDecScratch sc, u32 pass) {
    pfb_sync_body(UbCode{C}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, n_groups, sc.head, sc.g, pass);
}

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_write_kernel(SclUintRule C, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                    PfbDecScratch sc, u32 *__restrict__ out, u64 out_cap, PfbDecResult *__restrict__ result) {
    pfb_write_body(UbCode{C}, in, in_size_bytes, in_bit_offset, in_nbits, n_sub, sc.head, sc.g, out, out_cap,
                   &result->consumed);
}

// ---- host API -------------------------------------------------------------------------------------------------------------
extern "C" uint64_t scl_uint_block_scratch_bytes(uint64_t n_values, uint64_t in_nbits) {
    const u64 e = pfb_enc_scratch(n_values), d = pfb_dec_scratch(in_nbits);
    return scl_round_up(e > d ? e : d, 256);
}

extern "C" int scl_uint_codeword_host(const scl_uint_code *code, uint32_t x, uint32_t *bits, uint32_t *len) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked("uint_codeword_host", code, &C)) return rc;
    SCL_REQUIRE(bits && len, "uint_codeword_host: null pointer argument");
    const SclUintWord w = scl_uint_codeword(C, x);
    *bits = w.bits;
    *len = w.len;
    return SCL_OK;
}

extern "C" int scl_uint_decode_one_host(const scl_uint_code *code, uint32_t bits32, uint32_t rem, uint32_t *len, uint32_t *x) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked("uint_decode_one_host", code, &C)) return rc;
    SCL_REQUIRE(len && x, "uint_decode_one_host: null pointer argument");
    SCL_REQUIRE(rem >= 1, "uint_decode_one_host: rem = 0: at least one bit belongs to the stream");
    *len = *x = 0;
    const u32 kind = scl_uint_decode(C, bits32, rem, *len, *x);
    return kind == PFB_END_EXIT ? 0 : kind == PFB_END_TRUNC ? (int)SCL_ST_TRUNCATED : (int)SCL_ST_SIZE;
}

PFB_RESULT_IS(scl_uint_block_result);
static const PfbWords UB_WORDS = {"values", "scl_uint_block_scratch_bytes",
                                  "d_out, d_val and d_status must be 4-byte, d_scratch and d_nbits 8-byte aligned",
                                  "d_in and d_out_val must be 4-byte, d_scratch and d_result 8-byte aligned"};

static int ub_encode(const char *what, const scl_uint_code *code, const PfbEncodeArgs &a, hipStream_t st) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    const u32 *d_val = (const u32 *)a.d_val;
    return pfb_encode_launch<SCL_ST_SIZE>(
        what, UB_WORDS, a, (((uintptr_t)d_val | (uintptr_t)a.d_status) & 3) == 0, a.n * (PFB_MAX_LEN / 8), st,
        [&](dim3 grid, u64 *tile_bits, u32 *status) {
            hipLaunchKernelGGL(ub_tile_bits_kernel, grid, dim3(PFB_THREADS), 0, st, C, d_val, a.n, tile_bits, status);
        },
        [&](dim3 grid, const u64 *tile_off, PfbEncScratch *head, u32 *out32, u64 tail_index) {
            hipLaunchKernelGGL(ub_encode_tile_kernel, grid, dim3(PFB_THREADS), 0, st, C, d_val, a.n, tile_off, head, out32,
                               tail_index);
        });
}

static int ub_decode(const char *what, const scl_uint_code *code, const PfbDecodeArgs &a, hipStream_t st) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    return pfb_decode_launch<SCL_ST_SIZE>(
        what, UB_WORDS, a, ((uintptr_t)a.d_out & 3) == 0, st,
        [&](dim3 grid, u64 n_sub, u64 n_groups, const PfbDecScratch &sc, u32 pass) {
            hipLaunchKernelGGL(ub_sync_kernel, grid, dim3(PFB_THREADS), 0, st, C, a.d_in, a.in_size_bytes, a.in_bit_offset,
                               a.in_nbits, n_sub, n_groups, sc, pass);
        },
        [&](dim3 grid, u64 n_sub, const PfbDecScratch &sc) {
            hipLaunchKernelGGL(ub_write_kernel, grid, dim3(PFB_THREADS), 0, st, C, a.d_in, a.in_size_bytes, a.in_bit_offset,
                               a.in_nbits, n_sub, sc, (u32 *)a.d_out, a.out_cap, a.d_result);
        });
}

extern "C" int scl_uint_encode_block(const scl_uint_code *code, const uint32_t *d_val, uint64_t n, uint8_t *d_out,
                                     uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                     uint64_t scratch_bytes, void *stream) {
    return ub_encode("uint_encode_block", code, {d_val, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch, scratch_bytes},
                     (hipStream_t)stream);
}

extern "C" int scl_uint_decode_block(const scl_uint_code *code, const uint8_t *d_in, uint64_t in_size_bytes,
                                     uint64_t in_bit_offset, uint64_t in_nbits, uint32_t *d_out_val, uint64_t out_cap,
                                     scl_uint_block_result *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream) {
    return ub_decode("uint_decode_block", code,
                     {d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_val, out_cap, (PfbDecResult *)d_result, d_scratch,
                      scratch_bytes},
                     (hipStream_t)stream);
}

// ---- one block in host memory (the staging: scl_bit_block.h); the status goes back to the caller --------------------------
extern "C" int scl_uint_encode_block_host(const scl_uint_code *code, const uint32_t *h_val, uint64_t n, uint8_t *h_out,
                                          uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status) {
    const char *what = "uint_encode_block_host";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(h_out && nbits && status && (h_val || n == 0), "%s: null pointer argument", what);
    return pfb_encode_staged(what, UB_WORDS, h_val, n, 4, n * (PFB_MAX_LEN / 8), h_out, out_cap_bytes, nbits, status,
                             [&](const PfbEncodeArgs &a) { return ub_encode(what, code, a, nullptr); });
}

extern "C" int scl_uint_decode_block_host(const scl_uint_code *code, const uint8_t *h_in, uint64_t in_nbits,
                                          uint32_t *h_out_val, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                                          uint32_t *status) {
    const char *what = "uint_decode_block_host";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(h_in && n_out && consumed && status && (h_out_val || out_cap == 0), "%s: null pointer argument", what);
    return pfb_decode_staged(what, h_in, in_nbits, h_out_val, 4, out_cap, true, n_out, consumed, status,
                             [&](const PfbDecodeArgs &a) { return ub_decode(what, code, a, nullptr); });
}
