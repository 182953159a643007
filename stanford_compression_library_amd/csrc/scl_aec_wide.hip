// scl_aec_wide.hip -- adaptive order-k arithmetic coding on LARGE alphabets (BASELINE.json configs[3], second point:
// order-1 on bytes, K = 256), one wavefront lane per chunk, per-lane two-level count rows in device memory.  Round 3:
// the tuned arithmetic of scl_aec_fast.hip over the tables of scl_aec.hip.  Same streams, bit for bit, as scl_aec.hip and
//   ArithmeticEncoder.shrink_range / encode_block   scl/compressors/arithmetic_coding.py:58-78, :80-161
//   ArithmeticDecoder.decode_step_core / decode_block                               :177-201, :203-287
//   AdaptiveOrderKFreqModel                          scl/compressors/probability_models.py:95-160
//
// Served models (aec_wide_ok): AdaptiveOrderKFreqModel in the two-level row layout of scl_aec.hip (alphabet 17..256, more
// than 256 cells per chunk: 16 block totals + counts in blocks of 16, all stored as count - 1 in zero-filled scratch),
// PRECISION = 32, row totals that stay below 2^15 and below the model's rescale threshold for the whole chunk.
//
// Why it exists.  profiles/r03_aec_k256_pmc_summary.txt: the any-parameter kernels spend 830 (encode) / 1116 (decode)
// vector instructions per symbol on this model -- 64-bit divisions, literal renormalisation loops, a bit reader / writer
// that handles any width -- on top of one (encode) or two (decode) dependent round trips to a table that cannot be
// cached (272 KiB per lane).  Here the arithmetic is that of scl_aec_fast.hip (exact binary64 quotients with one
// reciprocal, closed-form renormalisation with the literal loops on the strict-comparison corners, 32-bit word I/O,
// ~150 instructions per symbol), and the ENCODER issues the two row reads of symbol i + 1 before it codes symbol i:
// its lookups do not depend on the coder state, only on the counts, so what symbol i adds to the rows that are already
// in flight is patched into the results (same context: total + 1; same context and a smaller / the same symbol:
// cumulative + 1 / frequency + 1).  The decoder learns its context from the symbol it has just decoded: two dependent
// round trips per symbol remain (block totals, then the block of counts the search lands in).
#include "scl_aec_internal.h"
#include "scl_aec_frame.h"

#define AW_THREADS 256

struct AecWideDev {
    u32 K;          // alphabet size 17..256
    u32 k;          // order 0..3
    u32 ctx_mod;    // K^k
    u32 row_cells;  // 16 + 16 * ceil(K / 16)
    u32 size_bits;  // DATA_BLOCK_SIZE_BITS (1..32)
    u64 cells;      // per chunk: ctx_mod * row_cells
};

// Cells are u16 here (the any-parameter kernels keep u32 cells in the same scratch: these kernels own their zero-filled
// scratch for one launch and use the first half of it): every count and block total stays below 2^15 (aec_wide_ok), and a
// group of 16 cells is 32 bytes -- the kernels are bound by the number of bytes their scattered row accesses move.
typedef u16 aw_cell;

__global__ void __launch_bounds__(AW_THREADS)
    aec_wide_encode_kernel(AecWideDev P, const u8 *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens,
                           u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride,
                           u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits, u32 *__restrict__ status,
                           u32 *__restrict__ scratch) {
    const u64 chunk = (u64)blockIdx.x * AW_THREADS + threadIdx.x;
    if (chunk >= n_chunks) return;
    const u32 n = lens ? lens[chunk] : chunk_len;
    aw_cell *cnt = reinterpret_cast<aw_cell *>(scratch) + chunk * P.cells;
    AfWriter wr;
    wr.init(out + chunk * out_stride);
    wr.put(af_header_value(n, P.size_bits), P.size_bits);  // :92-99
    u32 st = af_header_status(n, P.size_bits);
    u32 low = 0, hm = 0xFFFFFFFFu;
    u32 pending = 0;  // E3 steps not yet resolved

    // symbol i's rows are in flight since the previous iteration; what symbol i - 1 added to them (it was counted
    // after they were issued) is patched into the results.
    AfSymFeed feed;
    u32 s_cur = feed.first(sym + chunk * sym_stride, n, P.K, st);
    u32 ctx = 0;
    AfCells16 bt = af_load16(cnt);
    AfCells16 cb = af_load16(cnt + 16 + (s_cur & ~15u));
    u32 p_ctx = 0xFFFFFFFFu, p_s = 0;  // the symbol counted while these rows were in flight (none yet)
    u32 c_pv = 0, d_pv = 1;            // (c, d, T) = (0, 1, 1): the arithmetic stage is a no-op before the first symbol
    double x_pv = 1.0;
    for (u32 i = 0; i < n; ++i) {
        const u32 s = s_cur, b = s >> 4;
        const u64 rb = (u64)ctx * P.row_cells;
        // next symbol: its rows are issued now, before this symbol is counted
        const u32 s_nx = feed.next(i + 1, n, P.K, st);
        const u32 ctx_nx = af_next_ctx_k(P, ctx, s);
        const AfCells16 bt_nx = af_load16(cnt + (u64)ctx_nx * P.row_cells);
        const AfCells16 cb_nx = af_load16(cnt + (u64)ctx_nx * P.row_cells + 16 + (s_nx & ~15u));
        // meanwhile: the arithmetic of the previous symbol
        af_code_symbol(wr, low, hm, pending, c_pv, d_pv, x_pv);
        // freqs_current of this symbol (:118) from its rows (count[j] = 1 + cell)
        // This kernel's own text of af_row_counts (scl_aec_frame.h): through the helper it came out with 114 VGPRs for the
        // parent's 85, a wave less per SIMD (profiles/aec_frame_codegen.txt).  Keep the copy in step with the helper.
        AfRowCounts r = {0, 0, 0, 0};
        const u32 w = s & 15u;
#pragma unroll
        for (u32 j = 0; j < 16; ++j) {
            r.tot += bt.v[j];
            r.below += (j < b) ? bt.v[j] : 0u;
            r.below += (j < w) ? cb.v[j] : 0u;
            r.fs = (j == w) ? cb.v[j] : r.fs;
            r.fb = (j == b) ? bt.v[j] : r.fb;
        }
        if (p_ctx == ctx) {  // symbol i - 1 had the same context: its count is missing from the rows read above
            const u32 pb = p_s >> 4;
            r.tot += 1;
            r.below += (p_s < s) ? 1u : 0u;
            r.fs += (p_s == s) ? 1u : 0u;
            r.fb += (pb == b) ? 1u : 0u;
        }
        c_pv = s + r.below;
        d_pv = c_pv + 1 + r.fs;
        x_pv = af_recip((double)(P.K + r.tot));
        // update_model (:143-160): count[s] += 1, block total += 1 (cells hold count - 1)
        cnt[rb + 16 + s] = (aw_cell)(r.fs + 1);
        cnt[rb + b] = (aw_cell)(r.fb + 1);
        p_ctx = ctx;
        p_s = s;
        ctx = ctx_nx;
        s_cur = s_nx;
        bt = bt_nx;
        cb = cb_nx;
    }
    af_code_symbol(wr, low, hm, pending, c_pv, d_pv, x_pv);
    af_terminate(low, pending, [&](u32 bit) { af_emit(wr, bit, pending); });  // :153-159
    af_encode_results(wr.finish(), st, chunk, out_stride, out_bit_off, out_nbits, status);
}

__global__ void __launch_bounds__(AW_THREADS)
    aec_wide_decode_kernel(AecWideDev P, const u8 *__restrict__ in, u64 in_size_bytes, const u64 *__restrict__ bit_off,
                           const u32 *__restrict__ in_nbits, u64 n_chunks, u8 *__restrict__ out_sym, u64 out_stride,
                           u32 out_cap, u32 *__restrict__ out_lens, u32 *__restrict__ consumed,
                           u32 *__restrict__ status, u32 *__restrict__ scratch) {
    AfLaneDec f;
    if (af_lane_dec_done<AW_THREADS>(f, P.size_bits, in, in_size_bytes, bit_off, in_nbits, n_chunks, out_cap, out_lens, consumed,
                                     status))
        return;
    AfReader &rd = f.rd;
    const u32 n = f.n;
    aw_cell *cnt = reinterpret_cast<aw_cell *>(scratch) + f.chunk * P.cells;
    AfSymWord so;
    so.init(out_sym + f.chunk * out_stride);
    u64 used = 32;
    u32 state = rd.get(32);
    u32 low = 0, hm = 0xFFFFFFFFu;
    u32 ctx = 0;
    const u32 nblk = (P.K + 15) >> 4;
    AfCells16 bt = af_load16(cnt);
    for (u32 i = 0;; ++i) {
        const u64 rb = (u64)ctx * P.row_cells;
        // ---- decode_step_core, :177-201: block totals (in hand), then the block of counts the search lands in ----
        const double xr = af_recip((double)(hm - low) + 1.0);  // issued before the row arrives
        const AfRowFound r = af_row_find(bt, cnt + rb, P.K, nblk, state, low, xr);
        const double xT = af_recip((double)r.T);
        // update_model, then the next symbol's block totals: issued now, needed after the arithmetic below
        cnt[rb + 16 + r.s] = (aw_cell)(r.fs + 1);
        cnt[rb + r.b] = (aw_cell)(r.fb + 1);
        ctx = af_next_ctx_k(P, ctx, r.s);
        bt = af_load16(cnt + (u64)ctx * P.row_cells);
        af_shrink2(low, hm, r.c, r.c + 1 + r.fs, xT);
        so.put(r.s, i);
        if (i + 1 == n) break;  // before the renormalisation, :242-243
        // ---- renormalisation, :245-275 ----
        u32 k, m, nlow, nhm;
        const bool edge = af_renorm2(low, hm, k, m, nlow, nhm);
        if (__builtin_expect(edge, 0)) {
            af_renorm_literal_dec(low, hm, state, [&] {
                used++;
                return rd.get(1);
            });
        } else {
            const u32 kt = k + m;  // <= 31
            state = af_state_shift_in(rd, state, k, kt);
            low = nlow;
            hm = nhm;
            used += kt;
        }
    }
    so.finish(n);
    consumed[f.chunk] = af_consumed_bits(low, hm, state, used + P.size_bits);  // :277-282
    if (status) status[f.chunk] = f.st;
}

// ---- host side ----------------------------------------------------------------------------------------------
bool aec_wide_ok(const scl_aec_model *m, u64 max_symbols) {
    const AecDev &d = m->dev;
    if (d.kind != SCL_MODEL_ORDERK || !d.fenwick || d.P != 32) return false;
    const u64 total_max = (u64)d.K + max_symbols;  // bound on a row total and on any count
    return total_max < 32768 && total_max < d.max_total;
}

static AecWideDev aec_wide_dev(const scl_aec_model *m) {
    AecWideDev f;
    f.K = m->dev.K;
    f.k = m->dev.k;
    f.ctx_mod = (u32)m->dev.ctx_mod;
    f.row_cells = m->dev.row_cells;
    f.size_bits = m->dev.size_bits;
    f.cells = m->dev.cells;
    return f;
}

// bytes of the scratch these kernels use (and need zero-filled) for n_chunks chunks
u64 aec_wide_scratch_bytes(const scl_aec_model *m, u64 n_chunks) { return m->dev.cells * n_chunks * sizeof(aw_cell); }

void aec_wide_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *d_scratch) {
    scl_launch_encode(aec_wide_encode_kernel, aec_grid(a.n_chunks, AW_THREADS), st, aec_wide_dev(m), a, d_scratch);
}

void aec_wide_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *d_scratch) {
    scl_launch_decode(aec_wide_decode_kernel, aec_grid(a.n_chunks, AW_THREADS), st, aec_wide_dev(m), a, d_scratch);
}
