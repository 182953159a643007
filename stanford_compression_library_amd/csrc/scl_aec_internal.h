// scl_aec_internal.h -- model handle of the arithmetic coder and the launch entry points of its tuned kernel families,
// shared by scl_aec.hip (any parameters, the table of families) and scl_aec_{fast,split,iid,static,wide,sparse}.hip;
// the kernel parameters of the small-alphabet adaptive models, which two of those files code.  Internal to csrc/.
#pragma once
#include "scl_common.h"

struct AecDev {
    int kind;
    u32 K, k;
    u32 P, size_bits;
    u64 max_total;
    u64 cells;  // per-chunk scratch cells (u32)
    u64 ctx_mod;  // K^k
    const u32 *d_freq;  // [K] initial frequencies (FIXED / IID)
    const u32 *d_cum;   // [K] exclusive cumulative of d_freq (FIXED)
    u32 total0;         // sum of initial frequencies
    u32 fenwick;        // ORDERK with a large alphabet: two-level rows of (count - 1), see scl_aec.hip
    u32 row_cells;      // two-level rows: 16 block totals + 16 * ceil(K / 16) counts
};

struct scl_aec_model {
    int device;  // hipGetDevice() at create: the tables live there (scl_check_device)
    AecDev dev;
    u32 *d_freq, *d_cum;
    u32 h_freq[256];  // host copy of the initial frequencies (all ones for ORDERK)
    u32 *d_iid_init;  // IID, alphabet > 16: the two-level cumulative table of scl_aec_iid.hip (17 rows x 8 u32)
};

// The tuned kernel families.  Every launch takes (model, the batch call's arguments, stream, the call's scratch): the
// scratch is used by the order-k families on large alphabets only (scl_aec.hip holds the table of families).
// scl_aec_fast.hip
bool aec_fast_ok(const scl_aec_model *m, u64 max_symbols);
void aec_fast_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
void aec_fast_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
// scl_aec_split.hip: the encoder of the same models with the model side and the coder side of a chunk in two waves
void aec_split_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st);
// scl_aec_wide.hip: order-k models in the two-level row layout (large alphabets), tuned arithmetic over device-memory rows
bool aec_wide_ok(const scl_aec_model *m, u64 max_symbols);
u64 aec_wide_scratch_bytes(const scl_aec_model *m, u64 n_chunks);
void aec_wide_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
void aec_wide_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
// scl_aec_sparse.hip: the same models with one 64-byte line per context (the symbols seen in it) until it has been seen 28
// times, then its dense row: one table piece read and written per symbol instead of two
u64 aec_sparse_zero_bytes(const scl_aec_model *m, u64 n_chunks);
void aec_sparse_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
void aec_sparse_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
// scl_aec_static.hip
bool aec_static_ok(const scl_aec_model *m);
void aec_static_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
void aec_static_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
// scl_aec_iid.hip
bool aec_iid_ok(const scl_aec_model *m, u64 max_symbols);
void aec_iid_build_init(const u32 *h_freq, u32 K, u32 *out136);
void aec_iid_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);
void aec_iid_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch);

// ---- launch shapes of the tuned families ------------------------------------------------------------------------------
// one lane per chunk, workgroups of `threads` lanes; the split encoder: `per_group` chunks to a workgroup of `threads`
static inline SclGrid aec_grid(u64 n_chunks, u32 threads) { return {(u32)((n_chunks + threads - 1) / threads), threads}; }
static inline SclGrid aec_grid_groups(u64 n_chunks, u32 per_group, u32 threads) { return {aec_grid(n_chunks, per_group).blocks, threads}; }
// kernels templated on ORDER1 (the context of an order-1 model is the previous symbol: no multiply, no modulo)
#define AEC_LAUNCH_ORDER1(m, LAUNCH, KERNEL, ...)                   \
    do {                                                            \
        if ((m)->dev.k == 1) LAUNCH(KERNEL<true>, __VA_ARGS__);     \
        else LAUNCH(KERNEL<false>, __VA_ARGS__);                    \
    } while (0)

// ---- small-alphabet adaptive models (aec_fast_ok): what scl_aec_fast.hip's and scl_aec_split.hip's kernels take ----------
struct AecFastDev {
    u32 K;          // alphabet size 2..16
    u32 nctx;       // K^k <= 16
    u32 ctx_magic;  // ceil(2^16 / nctx): (v * magic) >> 16 == v / nctx for v < 272
    u32 total0;     // initial total of a row
    u32 size_bits;  // DATA_BLOCK_SIZE_BITS (1..32)
    u32 initX[8];   // 16 packed u16: EXCLUSIVE cumulative initial counts X[j] = sum_{i<j}, padded with the total
};

template <bool ORDER1>
__device__ __forceinline__ u32 af_next_ctx(const AecFastDev &P, u32 ctx, u32 s) {  // past_k[1:] + [s], :146-151
    if (ORDER1) return s;
    // (24-bit multiplies: v < 272, magic <= 2^15, nctx <= 16 -- the 32-bit v_mul_lo_u32 is a quarter-rate instruction)
    const u32 v = __umul24(ctx, P.K) + s;
    return v - __umul24(__umul24(v, P.ctx_magic) >> 16, P.nctx);
}

static inline AecFastDev aec_fast_dev(const scl_aec_model *m) {
    AecFastDev f;
    f.K = m->dev.K;
    f.nctx = (u32)m->dev.ctx_mod;
    f.ctx_magic = (65536u + f.nctx - 1) / f.nctx;
    u32 X[16], acc = 0;
    for (u32 j = 0; j < 16; ++j) {
        X[j] = acc;  // exclusive; entries past the alphabet hold the total
        if (j < f.K) acc += m->h_freq[j];
    }
    f.total0 = acc;
    f.size_bits = m->dev.size_bits;
    for (u32 r = 0; r < 8; ++r) f.initX[r] = X[2 * r] | (X[2 * r + 1] << 16);
    return f;
}
