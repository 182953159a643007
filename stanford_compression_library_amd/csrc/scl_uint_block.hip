// scl_uint_block.hip -- Golomb, universal and Elias-delta coding of ONE block of uint32 values by the whole grid, for gfx950.
//
// The third user of scl_bit_block.h, beside scl_prefix_block.hip and scl_lz77_entropy_wide.hip, and the thinnest: the
// alphabet is unbounded, so no table sits in LDS -- the codeword policy is the rule of scl_uint_code.h, computed per value
// (encode) and per 32-bit look (decode: one count of leading bits and a shift).  The stream is the reference's: the codewords
// of GolombUintEncoder(M) / UniversalUintEncoder / EliasDeltaUintEncoder back to back, nothing else.
//
// encode   ub_tile_bits     a workgroup sums the codeword lengths of its tile; SCL_ST_SIZE for a codeword above 32 bits
//          ub_scan_tiles    ONE workgroup: exclusive 64-bit scan of the tile sums, nbits, the fits flag, SCL_ST_CAPACITY
//          ub_encode_tile   pfb_emit_tile on the tile's codewords (nothing on SCL_ST_SIZE / SCL_ST_CAPACITY)
//          ub_encode_tail   pfb_store_tail
// decode   ub_sync          pfb_sync_body, relaunched by pfb_run_sync_passes
//          ub_scan_groups   pfb_scan_to_end and the verdict: a cut codeword is SCL_ST_TRUNCATED, a prefix that announces more
//                           than 32 bits SCL_ST_SIZE (the status the LZ77 entropy stage gives such a codeword)
//          ub_write         pfb_write_body with uint32 symbols
// As in scl_prefix_block.hip no kernel waits on another workgroup: every dependency between workgroups is a kernel boundary.
// LDS per workgroup: encode 16.4 KiB of words; decode 4.3 KiB of input and 1 KiB of exits.  DESIGN.md 3.5.2.
#include "scl_bit_block.h"
#include "scl_uint_code.h"

// ---- encode ---------------------------------------------------------------------------------------------------------------
// the {bits, length} of the thread's PFB_PER_THREAD consecutive values (length 0 past the end of the block)
__device__ __forceinline__ u32 ub_load_codes(const SclUintRule &C, const u32 *__restrict__ val, u64 n, u64 first,
                                             uint2 (&e)[PFB_PER_THREAD]) {
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
        }
        e[j] = c;
        bits += c.y;
    }
    return bits;
}

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_tile_bits_kernel(SclUintRule C, const u32 *__restrict__ val, u64 n, u64 *__restrict__ tile_bits,
                        u32 *__restrict__ status) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    uint2 e[PFB_PER_THREAD];
    u32 bad = 0, total;
    const u64 first = (u64)blockIdx.x * PFB_TILE + threadIdx.x * PFB_PER_THREAD;
    const u32 bits = ub_load_codes(C, val, n, first, e);
#pragma unroll
    for (u32 j = 0; j < PFB_PER_THREAD; ++j)
        if (first + j < n && e[j].y == 0) bad = 1;  // a value of the block without a codeword of 32 bits
    (void)scl_block_scan_excl<u32, PFB_THREADS, SclScanSum>(bits, s_wave, &total);
    const int any_bad = __syncthreads_or((int)bad);
    if (threadIdx.x == 0) {
        tile_bits[blockIdx.x] = total;
        if (any_bad) atomicOr(status, (u32)SCL_ST_SIZE);
    }
}

// *status holds what ub_tile_bits found (the kernel in front of this one)
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    ub_scan_tiles_kernel(u64 *__restrict__ tile_bits, u64 n_tiles, u64 out_cap_bytes, PfbEncScratch *__restrict__ head,
                         u64 *__restrict__ nbits, u32 *__restrict__ status) {
    __shared__ u64 s_wave[PFB_SCAN_THREADS / 64];
    const u64 total = scl_block_scan_array<u64, PFB_SCAN_THREADS, SclScanSum>(tile_bits, n_tiles, s_wave);
    if (threadIdx.x == 0) {
        const bool coded = (*status & SCL_ST_SIZE) == 0;
        const bool fits = (total + 7) / 8 <= out_cap_bytes;
        head->fits = coded && fits ? 1u : 0u;
        *nbits = coded ? total : 0ull;
        if (coded && !fits) *status = SCL_ST_CAPACITY;
    }
}

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_encode_tile_kernel(SclUintRule C, const u32 *__restrict__ val, u64 n, const u64 *__restrict__ tile_off,
                          PfbEncScratch *__restrict__ head, u32 *__restrict__ out32, u64 tail_index) {
    __shared__ u32 s_wave[PFB_THREADS / 64];
    __shared__ u32 s_words[PFB_TILE_WORDS];
    if (!head->fits) return;  // SCL_ST_SIZE / SCL_ST_CAPACITY: nothing is written (uniform: the whole grid leaves)
    for (u32 i = threadIdx.x; i < PFB_TILE_WORDS; i += PFB_THREADS) s_words[i] = 0;
    __syncthreads();
    uint2 e[PFB_PER_THREAD];
    const u32 bits = ub_load_codes(C, val, n, (u64)blockIdx.x * PFB_TILE + threadIdx.x * PFB_PER_THREAD, e);
    pfb_emit_tile(e, bits, tile_off[blockIdx.x], s_words, s_wave, head, out32, tail_index);
}

__global__ void ub_encode_tail_kernel(const PfbEncScratch *__restrict__ head, const u64 *__restrict__ nbits,
                                      u8 *__restrict__ out, u64 out_cap_bytes) {
    pfb_store_tail(head, *nbits, out, out_cap_bytes);
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

// ONE workgroup: where the stream ends, the value offsets of the workgroups up to there, the result
__global__ void __launch_bounds__(PFB_SCAN_THREADS)
    ub_scan_groups_kernel(PfbDecScratch sc, u64 n_groups, u64 in_nbits, u64 out_cap, u32 sync_passes,
                          scl_uint_block_result *__restrict__ result) {
    u64 total;
    const u64 last_group = pfb_scan_to_end(sc.g, n_groups, &total);
    if (threadIdx.x == 0) {
        const u64 cut = sc.g.group_end[last_group];
        const u64 end = cut == PFB_NONE64 ? in_nbits : cut >> 2;
        u32 status = cut == PFB_NONE64 ? 0u : ((cut & 3u) == PFB_END_TRUNC ? SCL_ST_TRUNCATED : SCL_ST_SIZE);
        u64 consumed = end;
        // as the prefix-free block: bits left after out_cap values are SCL_ST_CAPACITY whatever they hold.
        // total > out_cap: ub_write stores `consumed` (0 for out_cap = 0)
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

__global__ void __launch_bounds__(PFB_THREADS, 4)
    ub_write_kernel(SclUintRule C, const u8 *__restrict__ in, u64 in_size_bytes, u64 in_bit_offset, u64 in_nbits, u64 n_sub,
                    PfbDecScratch sc, u32 *__restrict__ out, u64 out_cap, scl_uint_block_result *__restrict__ result) {
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

static int ub_encode(const char *what, const scl_uint_code *code, const u32 *d_val, u64 n, u8 *d_out, u64 out_cap_bytes,
                     u64 *d_nbits, u32 *d_status, void *d_scratch, u64 scratch_bytes, hipStream_t st) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(d_out && d_nbits && d_status && d_scratch && (d_val || n == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(n < (1ull << 32), "%s: %llu values: a block holds fewer than 2^32", what, (unsigned long long)n);
    SCL_REQUIRE(((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_nbits & 7) == 0 &&
                    ((uintptr_t)d_val & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                "%s: d_out, d_val and d_status must be 4-byte, d_scratch and d_nbits 8-byte aligned", what);
    SCL_REQUIRE(scratch_bytes >= pfb_enc_scratch(n), "%s: scratch of %llu bytes, scl_uint_block_scratch_bytes asks for %llu",
                what, (unsigned long long)scratch_bytes, (unsigned long long)pfb_enc_scratch(n));
    SCL_HIP_TRY(hipMemsetAsync(d_nbits, 0, 8, st));
    SCL_HIP_TRY(hipMemsetAsync(d_status, 0, 4, st));
    if (n == 0) return SCL_OK;
    PfbEncScratch *head = (PfbEncScratch *)d_scratch;
    u64 *tile_bits = (u64 *)((u8 *)d_scratch + 64);
    const u64 n_tiles = pfb_tiles(n);
    // the tiles OR their shared words in: zero what the longest possible stream can reach
    const u64 reach = n * (PFB_MAX_LEN / 8);
    const u64 zeroed = reach < out_cap_bytes ? reach : out_cap_bytes;
    if (zeroed) SCL_HIP_TRY(hipMemsetAsync(d_out, 0, zeroed, st));
    SCL_HIP_TRY(hipMemsetAsync(head, 0, 64, st));
    hipLaunchKernelGGL(ub_tile_bits_kernel, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, C, d_val, n, tile_bits, d_status);
    hipLaunchKernelGGL(ub_scan_tiles_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, tile_bits, n_tiles, out_cap_bytes, head,
                       d_nbits, d_status);
    const u64 tail_index = (out_cap_bytes & 3) ? out_cap_bytes >> 2 : PFB_NONE64;
    hipLaunchKernelGGL(ub_encode_tile_kernel, dim3((u32)n_tiles), dim3(PFB_THREADS), 0, st, C, d_val, n, (const u64 *)tile_bits,
                       head, (u32 *)d_out, tail_index);
    if (out_cap_bytes & 3)
        hipLaunchKernelGGL(ub_encode_tail_kernel, dim3(1), dim3(1), 0, st, (const PfbEncScratch *)head, (const u64 *)d_nbits,
                           d_out, out_cap_bytes);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

static int ub_decode(const char *what, const scl_uint_code *code, const u8 *d_in, u64 in_size_bytes, u64 in_bit_offset,
                     u64 in_nbits, u32 *d_out_val, u64 out_cap, scl_uint_block_result *d_result, void *d_scratch,
                     u64 scratch_bytes, hipStream_t st) {
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(d_in && d_result && d_scratch && (d_out_val || out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(in_nbits < (1ull << 46) && in_bit_offset < (1ull << 62), "%s: stream of %llu bits: 2^46 and more are not coded",
                what, (unsigned long long)in_nbits);
    SCL_REQUIRE(((uintptr_t)d_in & 3) == 0 && ((uintptr_t)d_scratch & 7) == 0 && ((uintptr_t)d_result & 7) == 0 &&
                    ((uintptr_t)d_out_val & 3) == 0,
                "%s: d_in and d_out_val must be 4-byte, d_scratch and d_result 8-byte aligned", what);
    SCL_REQUIRE(scratch_bytes >= pfb_dec_scratch(in_nbits), "%s: scratch of %llu bytes, scl_uint_block_scratch_bytes asks for %llu",
                what, (unsigned long long)scratch_bytes, (unsigned long long)pfb_dec_scratch(in_nbits));
    SCL_REQUIRE((in_bit_offset + in_nbits + 7) / 8 <= in_size_bytes, "%s: the stream ends behind in_size_bytes", what);
    if (in_nbits == 0) {  // an empty stream: zero values, nothing is launched
        SCL_HIP_TRY(hipMemsetAsync(d_result, 0, sizeof(scl_uint_block_result), st));
        return SCL_OK;
    }
    const u64 n_sub = pfb_subs(in_nbits), n_groups = pfb_groups(in_nbits);
    const PfbDecScratch sc = pfb_dec_carve(d_scratch, n_groups);
    SCL_HIP_TRY(hipMemsetAsync(sc.head, 0, 64, st));
    const dim3 grid((u32)n_groups), block(PFB_THREADS);
    u32 sync_passes = 0;
    const auto sync = [&](u32 pass) {
        hipLaunchKernelGGL(ub_sync_kernel, grid, block, 0, st, C, d_in, in_size_bytes, in_bit_offset, in_nbits, n_sub, n_groups, sc,
                           pass);
    };
    if (int rc = pfb_run_sync_passes(sync, sc.head, n_groups, st, &sync_passes)) return rc;
    hipLaunchKernelGGL(ub_scan_groups_kernel, dim3(1), dim3(PFB_SCAN_THREADS), 0, st, sc, n_groups, in_nbits, out_cap,
                       sync_passes, d_result);
    hipLaunchKernelGGL(ub_write_kernel, grid, block, 0, st, C, d_in, in_size_bytes, in_bit_offset, in_nbits, n_sub, sc, d_out_val,
                       out_cap, d_result);
    SCL_HIP_TRY(hipGetLastError());
    return SCL_OK;
}

extern "C" int scl_uint_encode_block(const scl_uint_code *code, const uint32_t *d_val, uint64_t n, uint8_t *d_out,
                                     uint64_t out_cap_bytes, uint64_t *d_nbits, uint32_t *d_status, void *d_scratch,
                                     uint64_t scratch_bytes, void *stream) {
    return ub_encode("uint_encode_block", code, d_val, n, d_out, out_cap_bytes, d_nbits, d_status, d_scratch, scratch_bytes,
                     (hipStream_t)stream);
}

extern "C" int scl_uint_decode_block(const scl_uint_code *code, const uint8_t *d_in, uint64_t in_size_bytes,
                                     uint64_t in_bit_offset, uint64_t in_nbits, uint32_t *d_out_val, uint64_t out_cap,
                                     scl_uint_block_result *d_result, void *d_scratch, uint64_t scratch_bytes, void *stream) {
    return ub_decode("uint_decode_block", code, d_in, in_size_bytes, in_bit_offset, in_nbits, d_out_val, out_cap, d_result,
                     d_scratch, scratch_bytes, (hipStream_t)stream);
}

// ---- one block in host memory ---------------------------------------------------------------------------------------------
extern "C" int scl_uint_encode_block_host(const scl_uint_code *code, const uint32_t *h_val, uint64_t n, uint8_t *h_out,
                                          uint64_t out_cap_bytes, uint64_t *nbits, uint32_t *status) {
    const char *what = "uint_encode_block_host";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(h_out && nbits && status && (h_val || n == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(n < (1ull << 32), "%s: %llu values: a block holds fewer than 2^32", what, (unsigned long long)n);
    const u64 reach = n * (PFB_MAX_LEN / 8);
    const u64 cap = reach < out_cap_bytes ? reach : out_cap_bytes;  // no stream of n values is longer than `reach`
    const u64 scratch_bytes = pfb_enc_scratch(n);
    ScratchDev d_val, d_out, d_meta, d_scr;
    int rc;
    if ((rc = d_val.alloc(n * 4)) || (rc = d_out.alloc(cap)) || (rc = d_meta.alloc(16)) || (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    if (n) SCL_HIP_TRY(hipMemcpy(d_val.p, h_val, n * 4, hipMemcpyHostToDevice));
    rc = ub_encode(what, code, (const u32 *)d_val.p, n, (u8 *)d_out.p, cap, (u64 *)d_meta.p, (u32 *)d_meta.p + 2, d_scr.p,
                   scratch_bytes, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    u64 meta[2];
    SCL_HIP_TRY(hipMemcpy(meta, d_meta.p, 16, hipMemcpyDeviceToHost));
    const u64 bytes = (meta[0] + 7) / 8;
    SCL_REQUIRE(bytes <= out_cap_bytes, "%s: output needs %llu bytes, capacity %llu", what, (unsigned long long)bytes,
                (unsigned long long)out_cap_bytes);
    *status = (u32)meta[1];
    *nbits = meta[0];
    if (*status == 0 && bytes) SCL_HIP_TRY(hipMemcpy(h_out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return SCL_OK;
}

extern "C" int scl_uint_decode_block_host(const scl_uint_code *code, const uint8_t *h_in, uint64_t in_nbits,
                                          uint32_t *h_out_val, uint64_t out_cap, uint64_t *n_out, uint64_t *consumed,
                                          uint32_t *status) {
    const char *what = "uint_decode_block_host";
    SclUintRule C;
    if (int rc = scl_uint_rule_checked(what, code, &C)) return rc;
    SCL_REQUIRE(h_in && n_out && consumed && status && (h_out_val || out_cap == 0), "%s: null pointer argument", what);
    SCL_REQUIRE(in_nbits < (1ull << 46), "%s: stream of %llu bits: 2^46 and more are not coded", what,
                (unsigned long long)in_nbits);
    const u64 in_bytes = (in_nbits + 7) / 8, in_size = scl_round_up(in_bytes, 4) + 4;
    const u64 scratch_bytes = pfb_dec_scratch(in_nbits);
    ScratchDev d_in, d_out, d_res, d_scr;
    int rc;
    if ((rc = d_in.alloc(in_size)) || (rc = d_out.alloc(out_cap * 4)) || (rc = d_res.alloc(sizeof(scl_uint_block_result))) ||
        (rc = d_scr.alloc(scratch_bytes)))
        return rc;
    SCL_HIP_TRY(hipMemset((u8 *)d_in.p + in_bytes, 0, in_size - in_bytes));  // every byte behind the stream that a word load reaches
    if (in_bytes) SCL_HIP_TRY(hipMemcpy(d_in.p, h_in, in_bytes, hipMemcpyHostToDevice));
    rc = ub_decode(what, code, (const u8 *)d_in.p, in_size, 0, in_nbits, (u32 *)d_out.p, out_cap, (scl_uint_block_result *)d_res.p,
                   d_scr.p, scratch_bytes, nullptr);
    if (rc) return rc;
    SCL_HIP_TRY(hipDeviceSynchronize());
    scl_uint_block_result res;
    SCL_HIP_TRY(hipMemcpy(&res, d_res.p, sizeof(res), hipMemcpyDeviceToHost));
    *n_out = res.n_out;
    *consumed = res.consumed;
    *status = res.status;
    if (res.n_out) SCL_HIP_TRY(hipMemcpy(h_out_val, d_out.p, res.n_out * 4, hipMemcpyDeviceToHost));
    return SCL_OK;
}
