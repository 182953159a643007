// scl_aec_iid.hip -- adaptive i.i.d. arithmetic coding (AdaptiveIIDFreqModel) for alphabets up to 256 symbols
// with the lane's whole model in LDS, one wavefront lane per chunk.  Same streams, bit for bit, as scl_aec.hip
// and the reference:
//   ArithmeticEncoder / ArithmeticDecoder   scl/compressors/arithmetic_coding.py:58-161, :177-287
//   AdaptiveIIDFreqModel                     scl/compressors/probability_models.py:70-92
//
// Served models (aec_iid_ok): kind IID, alphabet 17..256 (smaller ones are a single row of scl_aec_fast.hip),
// PRECISION = 32, initial total + chunk length < 2^15 and below the model's rescale
// threshold (so the halving rule :86-92 cannot fire inside a chunk).
//
// Model layout: two levels of cumulative counts, all u16, 32-byte rows [row][thread] in LDS:
//   XB[16]      exclusive cumulative totals of the 16 blocks of 16 symbols   (XB[b] = count of all symbols < 16 b)
//   IC[b][16]   inclusive cumulative counts inside block b                   (IC[b][w] = sum of block b up to w)
// c[s] = XB[b] + IC[b][w-1], c[s] + f[s] = XB[b] + IC[b][w]  (b = s >> 4, w = s & 15): three 2-byte reads;
// count[s] += 1 is IC[b][j] += 1 for j >= w and XB[j] += 1 for j > b: sixteen v_pk_add_u16 with two mask rows;
// the decoder's search is two packed compare-and-counts (block, then symbol) with one dependent row read between.
// 17 rows x 32 B x 256 lanes = 136 KiB: one workgroup per CU, one wave per SIMD, like scl_aec_fast.hip, whose
// arithmetic (exact binary64 division, closed-form renormalisation) and per-lane I/O are reused unchanged.
// The generic kernel scans the 256 counts twice per symbol: 0.38 GB/s round trip on bytes.
#include "scl_aec_internal.h"
#include "scl_aec_frame.h"

#define AI_THREADS 256
#define AI_ROW_BYTES (AI_THREADS * 32)          // one 32-byte row of every thread
#define AI_IC_BASE AI_ROW_BYTES                 // XB row first, then 16 block rows
#define AI_LUT_GE_BASE (17 * AI_ROW_BYTES)      // mask rows (j >= w)
#define AI_LUT_GT_BASE (AI_LUT_GE_BASE + 512)   // mask rows (j > b)
#define AI_OUT_BASE (AI_LUT_GT_BASE + 512)      // decoder: 64 bytes of symbol staging per lane (AfSymOut)
#define AI_LDS_BYTES (AI_LUT_GT_BASE + 512)
#define AI_DEC_LDS_BYTES (AI_OUT_BASE + AI_THREADS * 64)

struct AecIidDev {
    u32 K, total0;
    u32 size_bits;  // DATA_BLOCK_SIZE_BITS (1..32)
    const u32 *d_init;  // 17 rows x 8 packed u32: XB, then IC[0..15], built from the initial frequencies
};

__device__ __forceinline__ void ai_setup_tables(char *lds, const AecIidDev &P, u32 tid) {
    af_fill_mask_rows(lds + AI_LUT_GE_BASE, tid, [](u32 j, u32 s) { return j >= s; });
    af_fill_mask_rows(lds + AI_LUT_GT_BASE, tid, [](u32 j, u32 s) { return j > s; });
    const uint4 *init = reinterpret_cast<const uint4 *>(P.d_init);
    for (u32 row = 0; row < 17; ++row) af_row_store(lds, row * AI_ROW_BYTES + tid * 32, AfRow{init[2 * row], init[2 * row + 1]});
    __syncthreads();
}

// The encoder's model stage (af_lane_encode), split as in scl_aec_fast.hip: loads first, update and 1/T after the previous
// symbol is coded.
struct AiEncModel {
    char *lds;
    u32 tid;
    u32 T;  // the total of an i.i.d. model is its initial total plus the symbols seen
    u32 c_nx = 0, d_nx = 1, T_nx = 1;
    double x_nx = 1.0;
    AfRow XB;  // the block-level row also lives in registers (one context: it is never re-read)
    u32 m_rowaddr = 0, m_xb = 0, m_ic = 0, m_icm1 = 0, m_w = 0;
    AfRow m_IC, m_ge, m_gt;
    __device__ __forceinline__ AiEncModel(const AecIidDev &P, char *lds_, u32 tid_)
        : lds(lds_), tid(tid_), T(P.total0), XB(af_row_load(lds_, tid_ * 32)) {}
    __device__ __forceinline__ void issue(u32 s) {
        const u32 b = s >> 4, w = s & 15u;
        m_w = w;
        m_rowaddr = AI_IC_BASE + b * AI_ROW_BYTES + tid * 32;
        m_xb = *reinterpret_cast<const u16_lds *>(lds + tid * 32 + 2 * b);
        m_ic = *reinterpret_cast<const u16_lds *>(lds + m_rowaddr + 2 * w);
        m_icm1 = *reinterpret_cast<const u16_lds *>(lds + m_rowaddr + 2 * w - 2);  // unused when w == 0
        m_IC = af_row_load(lds, m_rowaddr);
        m_ge = af_row_load(lds, AI_LUT_GE_BASE + w * 32);
        m_gt = af_row_load(lds, AI_LUT_GT_BASE + b * 32);
    }
    __device__ __forceinline__ void finish() {
        c_nx = m_xb + (m_w ? m_icm1 : 0u);
        d_nx = m_xb + m_ic;
        T_nx = T;
        x_nx = af_recip((double)T);
        // update_model (:83-85): count[s] += 1
        af_row_store(lds, m_rowaddr, af_row_add(m_IC, m_ge));
        XB = af_row_add(XB, m_gt);
        af_row_store(lds, tid * 32, XB);
        T += 1;
    }
    template <class W, class Emit>
    __device__ __forceinline__ void code(W &wr, u32 &low, u32 &hm, u32 &pending, u32 cc, u32 dd, u32, double xx, Emit emit) {
        af_shrink2(low, hm, cc, dd, xx);
        u32 k, m, nlow, nhm;
        const bool edge = af_renorm2_dec(low, hm, k, m, nlow, nhm);  // the conservative corner test: two compares fewer
        const bool rare = edge | (k + pending > 32);  // one condition, one branch
        if (__builtin_expect(rare, 0)) {
            af_renorm_literal_enc(low, hm, pending, emit);
        } else {
            af_put_common_flat(wr, low, k, m, pending);
            low = nlow;
            hm = nhm;
        }
    }
};

__global__ void __launch_bounds__(AI_THREADS)
    aec_iid_encode_kernel(AecIidDev P, const u8 *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens,
                          u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride,
                          u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[AI_DEC_LDS_BYTES];  // tables + 64 bytes of stream staging per lane
    const u32 tid = threadIdx.x;
    ai_setup_tables(lds, P, tid);
    const u64 chunk = (u64)blockIdx.x * AI_THREADS + tid;
    if (chunk >= n_chunks) return;
    AfWriterT<true> wr;
    wr.init(out + chunk * out_stride, lds + AI_OUT_BASE, tid);
    AiEncModel mdl(P, lds, tid);
    const AfEncoded e = af_lane_encode(mdl, wr, P.K, P.size_bits, sym, sym_stride, lens, chunk_len, chunk);
    // The stores written out: behind af_encode_results this kernel measured 0.85 % slower (profiles/aec_frame_timing.txt).
    out_bit_off[chunk] = chunk * out_stride * 8;
    out_nbits[chunk] = (u32)e.total;
    if (status) status[chunk] = e.st;
}

// One symbol of the decoder (af_lane_decode): decode_step_core (:177-201) and update_model.
// low <= state <= hm holds for ANY input bits (the symbol chosen is the one whose interval holds the state), so
// target <= T - 1, and with it b <= last block (XB of the blocks past the alphabet is T) and w <= the last symbol of the
// block (its sums stay at the block total past the alphabet): the searches need no clamps.  b <= 15 structurally
// (XB[0] = 0 <= target), which is what the addresses need; the guard on s is for the symbol written.
struct AiDecStep {
    char *lds;
    u32 tid, K, T;
    AfRow XB;
    __device__ __forceinline__ AiDecStep(const AecIidDev &P, char *lds_, u32 tid_)
        : lds(lds_), tid(tid_), K(P.K), T(P.total0), XB(af_row_load(lds_, tid_ * 32)) {}
    __device__ __forceinline__ u32 operator()(u32 &low, u32 &hm, u32 state) {
        const double xr = af_recip((double)(hm - low) + 1.0);
        const double num = __builtin_fma((double)(state - low) + 1.0, (double)T, -0.5);
        const u32 tgt = (u32)(num * xr);  // ((state - low + 1) * T - 1) // rng, see scl_aec.hip
        // block: largest b with XB[b] <= target  (XB[0] = 0 always counts).  Both searches hand back their compare masks:
        // the rows are sorted, so "entry > target" is exactly the set update_model increments (af_pk_search16)
        AfRow xbm, icm;
        const u32 b = (af_row_search(XB, tgt, xbm) - 1u) & 15u;
        const u32 rowaddr = AI_IC_BASE + b * AI_ROW_BYTES + tid * 32;
        u32 xb = *reinterpret_cast<const u16_lds *>(lds + tid * 32 + 2 * b);
        const AfRow IC = af_row_load(lds, rowaddr);
        // 1/T: its seven instructions go here, while the row is in flight (the empty asm statements pin it between the block
        // search and the first use of the row; they also keep the 16-bit reads 32 bits wide -- narrowed to 16-bit operations
        // each costs a v_and 0xffff)
        u32 T2 = T;
        asm volatile("" : "+v"(T2) : "v"(b));
        double xT = af_recip((double)T2);
        asm volatile("" : "+v"(xT));
        asm volatile("" : "+v"(xb));
        // symbol inside the block: number of inclusive sums <= target - XB[b]
        const u32 w = af_row_search(IC, tgt - xb, icm);
        const u32 s = min(16 * b + w, K - 1);
        u32 ic = *reinterpret_cast<const u16_lds *>(lds + rowaddr + 2 * w);
        u32 icm1 = *reinterpret_cast<const u16_lds *>(lds + rowaddr + 2 * w - 2);
        // update_model
        af_row_store(lds, rowaddr, af_row_sub(IC, icm));
        XB = af_row_sub(XB, xbm);
        af_row_store(lds, tid * 32, XB);
        asm volatile("" : "+v"(ic), "+v"(icm1));
        // w = 0 <=> IC[0] > target - XB[b] <=> the low half of icm's first word is all ones
        const u32 c = xb + (icm1 & ~icm.a.x), d = xb + ic;
        af_shrink2(low, hm, c, d, xT);
        T += 1;
        return s;
    }
};

__global__ void __launch_bounds__(AI_THREADS)
    aec_iid_decode_kernel(AecIidDev P, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                          const u32 *__restrict__ in_nbits, u64 n_chunks, u8 *__restrict__ out_sym, u64 out_stride,
                          u32 out_cap, u32 *__restrict__ out_lens, u32 *__restrict__ consumed,
                          u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[AI_DEC_LDS_BYTES];
    ai_setup_tables(lds, P, threadIdx.x);
    AfLaneDec f;
    if (af_lane_dec_done<AI_THREADS>(f, P.size_bits, in, in_size_bytes, bit_off, in_nbits, n_chunks, out_cap, out_lens, consumed,
                                     status))
        return;
    AiDecStep step(P, lds, threadIdx.x);
    af_lane_decode(step, f, lds + AI_OUT_BASE, out_sym + f.chunk * out_stride, consumed, status);
}

// ---- host side ----------------------------------------------------------------------------------------------
bool aec_iid_ok(const scl_aec_model *m, u64 max_symbols) {
    const AecDev &d = m->dev;
    if (d.kind != SCL_MODEL_IID || d.K < 17 || d.K > 256 || d.P != 32 || !m->d_iid_init)
        return false;
    const u64 total_max = (u64)d.total0 + max_symbols;
    return total_max < 32768 && total_max < d.max_total;
}

// 17 rows of 16 u16 (packed in u32 pairs) from the initial frequencies: XB, then IC[0..15]
void aec_iid_build_init(const u32 *h_freq, u32 K, u32 *out136) {
    u32 rows[17][16];
    u32 acc = 0;
    for (u32 b = 0; b < 16; ++b) {
        rows[0][b] = acc;
        u32 in_block = 0;
        for (u32 w = 0; w < 16; ++w) {
            const u32 s = 16 * b + w;
            if (s < K) in_block += h_freq[s];
            rows[1 + b][w] = in_block;
        }
        acc += in_block;
    }
    for (u32 r = 0; r < 17; ++r)
        for (u32 j = 0; j < 8; ++j) out136[r * 8 + j] = rows[r][2 * j] | (rows[r][2 * j + 1] << 16);
}

static AecIidDev aec_iid_dev(const scl_aec_model *m) {
    AecIidDev f;
    f.K = m->dev.K;
    f.total0 = m->dev.total0;
    f.size_bits = m->dev.size_bits;
    f.d_init = m->d_iid_init;
    return f;
}

void aec_iid_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *) {
    scl_launch_encode(aec_iid_encode_kernel, aec_grid(a.n_chunks, AI_THREADS), st, aec_iid_dev(m), a);
}

void aec_iid_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *) {
    scl_launch_decode(aec_iid_decode_kernel, aec_grid(a.n_chunks, AI_THREADS), st, aec_iid_dev(m), a);
}
