// scl_aec_fast.hip -- adaptive arithmetic coding with per-lane context tables in LDS (BASELINE.json configs[3]),
// one wavefront lane per chunk.  Same streams, bit for bit, as scl_aec.hip and the reference:
//   ArithmeticEncoder.shrink_range / encode_block   scl/compressors/arithmetic_coding.py:58-78, :80-161
//   ArithmeticDecoder.decode_step_core / decode_block                               :177-201, :203-287
//   AdaptiveIIDFreqModel / AdaptiveOrderKFreqModel   scl/compressors/probability_models.py:70-92, :95-160
//
// Served models (aec_fast_ok): PRECISION = 32, adaptive IID or order-k model with
// alphabet 2..16 and at most 16 contexts (K^k <= 16: order-1 K <= 16, order-2 K <= 4, ...), totals that stay
// below 2^15 and below the model's rescale threshold for the whole chunk.  Everything else -> scl_aec.hip.
//
// What is different from the generic kernel (13.7 / 21.7 ms per 256 MiB of order-1 K = 16 data, now 1.9 / 2.6 ms):
//  * Model layout.  A context row is 16 u16 EXCLUSIVE cumulative counts X[j] = count[0] + .. + count[j-1]
//    (entries past the alphabet hold the total), 32 bytes per row, row `ctx` of thread t at LDS [ctx][t], plus a
//    u32 total per row: c = X[s], d = X[s+1] (or the total) are two 2-byte reads at one address, the update
//    `count[s] += 1` is X[j] += 1 for j > s = eight v_pk_add_u16 on the row with a mask row from a 512-byte LUT
//    and one ds_add_u32 on the total, and the decoder's search max{s : c[s] <= target} is a packed
//    compare-and-count over the 8 row registers.  16 contexts x 32 B x 256 lanes = 128 KiB (+ 16 KiB totals):
//    one workgroup of 256 lanes per CU, i.e. ONE wave per SIMD -- the kernels are bound by how fast a lone wave
//    issues instructions (~6 clk each, profiles/r01_ubench_dp_issue.txt), so every instruction counts.
//  * Arithmetic.  (rng*c)//T and ((state-low+1)*T-1)//rng are evaluated in binary64: every operand is an integer
//    below 2^47, q = trunc((num + 0.5) * x) with x = 1/den refined by two Newton steps from v_rcp_f32 is exact
//    because the quotient's error (< 2^-18 resp. 2^-35) is below the distance 0.5/den of (num + 0.5)/den from the
//    nearest integer (den < 2^15 resp. <= 2^32).  low and high-1 are kept as u32.
//  * Renormalisation in closed form.  With hm = high - 1: k = clz(low ^ hm) E1/E2 steps emit the k common leading
//    bits, then m = number of leading (1,0) bit pairs of (low, hm) below them E3 steps.  The reference's STRICT
//    comparisons (quirk Q1: `high < HALF`, `low > HALF`, `low > QTR and high < 3*QTR`) differ from this only when
//    low or high hits a power-of-two boundary inside the shifted-out prefix, i.e. when
//    ctz(low) + k + m + 1 >= 32 or ctz(high) + k + m + 1 >= 32; those symbols (rare after the first few of a
//    chunk) and runs of more than 32 - k pending bits take the literal loops of the reference.
//  * Encoder software pipeline: the model reads of symbol i+1 are in flight while symbol i is coded; words go
//    straight to the slot (4-byte stores, L2 merges them); symbols arrive four per 32-bit load, one word ahead,
//    the load unconditional so that it is not waited for at once.
#include <stdlib.h>

#include "scl_aec_internal.h"
#include "scl_aec_frame.h"

#define AF_THREADS 256
#define AF_CTX_BYTES (AF_THREADS * 32)      // one 32-byte row of every thread
#define AF_TABLE_BYTES (16 * AF_CTX_BYTES)  // 128 KiB
#define AF_TOT_BASE AF_TABLE_BYTES          // u32 totals [ctx][thread]
#define AF_TOT_BYTES (16 * AF_THREADS * 4)
#define AF_LUT_BASE (AF_TOT_BASE + AF_TOT_BYTES)
#define AF_LUT_BYTES 512
#define AF_LDS_BYTES (AF_LUT_BASE + AF_LUT_BYTES)

// LDS image of one workgroup: rows (exclusive cumulative counts, 32 bytes per context and thread), row totals,
// and the update masks LUT[s][j] = (j > s)
__device__ __forceinline__ void af_setup_tables(char *lds, const AecFastDev &P, u32 tid) {
    af_fill_mask_rows(lds + AF_LUT_BASE, tid, [](u32 j, u32 s) { return j > s; });
    const AfRow init = {make_uint4(P.initX[0], P.initX[1], P.initX[2], P.initX[3]),
                        make_uint4(P.initX[4], P.initX[5], P.initX[6], P.initX[7])};
    for (u32 c = 0; c < P.nctx; ++c) {
        af_row_store(lds, c * AF_CTX_BYTES + tid * 32, init);
        *reinterpret_cast<u32_lds *>(lds + AF_TOT_BASE + c * (AF_THREADS * 4) + tid * 4) = P.total0;
    }
    __syncthreads();
}

// The encoder's model stage (af_lane_encode), split in two so that the arithmetic of the previous symbol runs while the
// LDS reads are in flight: issue = freqs_current lookup for symbol s (loads only), finish = update_model (:118) and 1/T.
// Everything the arithmetic of a symbol needs (c, d, T, 1/T) is ready one iteration ahead.
template <bool ORDER1>
struct AfEncModel {
    const AecFastDev &P;
    char *lds;
    u32 tid;
    u32 ctx = 0;
    u32 c_nx = 0, d_nx = 1, T_nx = 1;
    double x_nx = 1.0;
    u32 m_rowbase = 0, m_totaddr = 0, m_s = 0, m_draw = 0;
    AfRow m_R, m_M;
    __device__ __forceinline__ AfEncModel(const AecFastDev &P_, char *lds_, u32 tid_) : P(P_), lds(lds_), tid(tid_) {}
    __device__ __forceinline__ void issue(u32 s) {
        m_rowbase = ctx * AF_CTX_BYTES + tid * 32;
        m_totaddr = AF_TOT_BASE + ctx * (AF_THREADS * 4) + tid * 4;
        m_s = s;
        const u32 ea = m_rowbase + 2 * s;
        c_nx = *reinterpret_cast<const u16_lds *>(lds + ea);
        m_draw = *reinterpret_cast<const u16_lds *>(lds + ea + 2);
        T_nx = *reinterpret_cast<const u32_lds *>(lds + m_totaddr);
        m_R = af_row_load(lds, m_rowbase);
        m_M = af_row_load(lds, AF_LUT_BASE + s * 32);
        ctx = af_next_ctx<ORDER1>(P, ctx, s);
    }
    __device__ __forceinline__ void finish() {
        // update_model: count[s] += 1  <=>  X[j] += 1 for j > s, total += 1
        af_row_store(lds, m_rowbase, af_row_add(m_R, m_M));
        __hip_atomic_fetch_add(reinterpret_cast<u32 *>(lds + m_totaddr), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        d_nx = (m_s == 15) ? T_nx : m_draw;
        x_nx = af_recip((double)T_nx);
    }
    // arithmetic stage: shrink_range (:58-78) and the renormalisation loops (:126-150) of one symbol, in the first forms
    // (af_shrink, af_renorm_counts): this kernel is the second implementation the tests compare the split encoder against
    template <class Emit>
    __device__ __forceinline__ void code(AfWriter &wr, u32 &low, u32 &hm, u32 &pending, u32 cc, u32 dd, u32 TT, double xx,
                                         Emit emit) {
        af_shrink(low, hm, cc, dd, TT, xx);
        u32 k, m;
        const bool edge = af_renorm_counts(low, hm, k, m);
        if (__builtin_expect(edge || (k + pending > 32), 0)) {
            af_renorm_literal_enc(low, hm, pending, emit);
        } else {
            af_put_common(wr, low, k, m, pending);
            const u32 kt = k + m;  // <= 31
            low = (low << kt) & 0x7FFFFFFFu;
            hm = (hm << kt) | ((1u << kt) - 1u) | AF_HALF;
        }
    }
};

template <bool ORDER1>
__global__ void __launch_bounds__(AF_THREADS)
    aec_fast_encode_kernel(AecFastDev P, const u8 *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens,
                           u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride,
                           u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[AF_LDS_BYTES];
    const u32 tid = threadIdx.x;
    af_setup_tables(lds, P, tid);
    const u64 chunk = (u64)blockIdx.x * AF_THREADS + tid;
    if (chunk >= n_chunks) return;
    AfWriter wr;
    wr.init(out + chunk * out_stride);
    AfEncModel<ORDER1> mdl(P, lds, tid);
    const AfEncoded e = af_lane_encode(mdl, wr, P.K, P.size_bits, sym, sym_stride, lens, chunk_len, chunk);
    af_encode_results(e.total, e.st, chunk, out_stride, out_bit_off, out_nbits, status);
}

// ---- decoder (round 4) ---------------------------------------------------------------------------------------------
// Its own table layout: a context row is 16 u16 INCLUSIVE cumulative counts Y[j] = count[0] + .. + count[j] (entries past
// the alphabet hold the total, so Y[15] IS the row total: no separate total array, no second LDS update, no clamp of the
// searched symbol).  c = Y[s-1] (0 for s = 0), d = Y[s]; update_model is Y[j] += 1 for j >= s = eight v_pk_add_u16 with a
// mask row from the 512-byte LUT; the search max{s : c[s] <= target} is 16 - #{j : Y[j] > target}.
// Symbols leave through 64 bytes of LDS per lane (the 16 KiB the totals used to take) as whole 64-byte sectors -- four
// back-to-back 16-byte stores every 64 symbols -- instead of one 4-byte store per four symbols, which the memory system
// did not merge at 262 144 open lines: 12.6 GB of HBM writes for 1 GiB of symbols (profiles/traffic.json, round 3).
#define AD_ROW_BASE 16                             // rows start 16 bytes in: the address "two bytes before a row" is never negative
#define AD_OUT_BASE (AD_ROW_BASE + AF_TABLE_BYTES)  // [thread][64 bytes]
#define AD_OUT_BYTES (AF_THREADS * 64)
#define AD_LDS_BYTES (AD_OUT_BASE + AD_OUT_BYTES)

__device__ __forceinline__ void ad_setup_tables(char *lds, const AecFastDev &P, u32 tid) {
    // inclusive from the exclusive initX: Y[j] = X[j + 1], Y[15] = total
    u32 y[8];
#pragma unroll
    for (u32 r = 0; r < 8; ++r) {
        const u32 lo = P.initX[r] >> 16;                                   // X[2r + 1]
        const u32 hi = (r < 7) ? (P.initX[r + 1] & 0xFFFFu) : P.total0;    // X[2r + 2]
        y[r] = lo | (hi << 16);
    }
    const AfRow init = {make_uint4(y[0], y[1], y[2], y[3]), make_uint4(y[4], y[5], y[6], y[7])};
    for (u32 c = 0; c < P.nctx; ++c) af_row_store(lds, AD_ROW_BASE + c * AF_CTX_BYTES + tid * 32, init);
    __syncthreads();
}

// One symbol of the decoder (af_lane_decode): decode_step_core (:177-201) and update_model.
template <bool ORDER1>
struct AdStep {
    const AecFastDev &P;
    char *lds;
    u32 lane_m2;  // two bytes before the lane's row of context 0
    u32 row_m2;   // the same for the current context: carried from symbol to symbol
    u32 ctx = 0;
    AfRow R;
    __device__ __forceinline__ AdStep(const AecFastDev &P_, char *lds_, u32 tid)
        : P(P_), lds(lds_), lane_m2(AD_ROW_BASE + tid * 32 - 2), row_m2(lane_m2), R(af_row_load(lds_, AD_ROW_BASE + tid * 32)) {}
    __device__ __forceinline__ u32 operator()(u32 &low, u32 &hm, u32 state) {
        // T = Y[15] < 2^15, as float (one SDWA conversion out of the packed pair) and as double (from the float): both exact
        float Tf;
        asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(Tf) : "v"(R.b.w));
        const double Td = (double)Tf;
        const double xr = af_recip((double)(hm - low) + 1.0);
        // target = ((state - low + 1) * T - 1) // rng  (see scl_aec.hip).  low <= state <= hm holds for ANY input bits (the
        // symbol chosen is the one whose interval holds the state), so target <= T - 1; the guard is on s below.
        const double num = __builtin_fma((double)(state - low) + 1.0, Td, -0.5);
        const u32 tgt = (u32)(num * xr);
        // s = #{j : Y[j] <= target}; Y[15] = T > target, so s <= 15, and entries past the alphabet hold T as well, so
        // s <= K - 1
        AfRow M;
        const u32 s = min(af_row_search(R, tgt, M), P.K - 1);
        // c = Y[s - 1], d = Y[s]: two u16 reads, issued before the row is rewritten; s = 0 reads the two bytes in front of
        // the row, masked away below.  All addresses of the step hang off "row - 2": one add fewer than with "row" and "- 2".
        const u32 ea_m2 = row_m2 + 2 * s;
        u32 c_raw = *reinterpret_cast<const u16_lds *>(lds + ea_m2);
        u32 ea_d = ea_m2;
        asm("" : "+v"(ea_d));  // hides that the two reads are adjacent (the compiler would merge them into one unaligned read)
        u32 d_raw = *reinterpret_cast<const u16_lds *>(lds + ea_d + 2);
        // update_model: Y[j] += 1 for j >= s, i.e. minus the search's masks
        af_row_store(lds, row_m2 + 2, af_row_sub(R, M));
        ctx = af_next_ctx<ORDER1>(P, ctx, s);
        // next symbol's row: issued now, needed only after the arithmetic below
        asm("v_lshl_add_u32 %0, %1, 13, %2" : "=v"(row_m2) : "v"(ctx), "v"(lane_m2));  // ctx * AF_CTX_BYTES + lane_m2, one op
        R = af_row_load(lds, row_m2 + 2);
        // (the empty asm statements around 1/T place its seven instructions after the search and before the wait for c, d)
        float T2 = Tf;
        asm volatile("" : "+v"(T2) : "v"(s));
        double xT = af_recip_fd(T2, Td);
        asm volatile("" : "+v"(xT));
        asm volatile("" : "+v"(c_raw), "+v"(d_raw));
        const u32 c = c_raw & ~M.a.x;
        af_shrink2_d(low, hm, (double)c, (double)d_raw, xT);
        return s;
    }
};

template <bool ORDER1>
__global__ void __launch_bounds__(AF_THREADS)
    aec_fast_decode_kernel(AecFastDev P, const u8 *__restrict__ in, u64 in_size_bytes,
                           const u64 *__restrict__ bit_off, const u32 *__restrict__ in_nbits, u64 n_chunks,
                           u8 *__restrict__ out_sym, u64 out_stride, u32 out_cap, u32 *__restrict__ out_lens,
                           u32 *__restrict__ consumed, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[AD_LDS_BYTES];
    ad_setup_tables(lds, P, threadIdx.x);
    AfLaneDec f;
    if (af_lane_dec_done<AF_THREADS>(f, P.size_bits, in, in_size_bytes, bit_off, in_nbits, n_chunks, out_cap, out_lens, consumed,
                                     status))
        return;
    AdStep<ORDER1> step(P, lds, threadIdx.x);
    af_lane_decode(step, f, lds + AD_OUT_BASE, out_sym + f.chunk * out_stride, consumed, status);
}

// ---- host side ----------------------------------------------------------------------------------------------
bool aec_fast_ok(const scl_aec_model *m, u64 max_symbols) {
    const AecDev &d = m->dev;
    if (d.kind != SCL_MODEL_IID && d.kind != SCL_MODEL_ORDERK) return false;
    if (d.K < 2 || d.K > 16 || d.ctx_mod > 16 || d.P != 32) return false;
    const u64 total_max = (u64)d.total0 + max_symbols;  // IID: total; ORDERK: bound on a row total and on any count
    if (total_max >= 32768 || total_max >= d.max_total) return false;
    return true;
}

void aec_fast_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *) {
    // round 3: the two-role encoder (scl_aec_split.hip) serves every batch; SCL_AEC_ENC=lane keeps the one-lane-per-
    // chunk kernel below for A/B timing and as a second implementation the tests compare against
    const char *enc_env = getenv("SCL_AEC_ENC");  // read at every call, like the other switches
    const bool lane_kernel = enc_env && (enc_env[0] == 'l' || enc_env[0] == 'L');
    if (!lane_kernel) {
        aec_split_encode_launch(m, a, st);
        return;
    }
    AEC_LAUNCH_ORDER1(m, scl_launch_encode, aec_fast_encode_kernel, aec_grid(a.n_chunks, AF_THREADS), st, aec_fast_dev(m), a);
}

void aec_fast_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *) {
    AEC_LAUNCH_ORDER1(m, scl_launch_decode, aec_fast_decode_kernel, aec_grid(a.n_chunks, AF_THREADS), st, aec_fast_dev(m), a);
}
