// scl_aec_frame.h -- what stands around the per-symbol work of the tuned arithmetic-coder kernels, one copy each.
// Internal to csrc/.  (Arithmetic and the rare paths: scl_aec_math.h; readers, writers and packed rows: scl_aec_lane_io.h.)
//
// Who uses what:
//   scl_aec_fast.hip, scl_aec_iid.hip (a lane's model in LDS)
//       decoders: af_lane_dec_done, af_lane_decode<STEP>          encoders: af_lane_encode<MODEL>
//   scl_aec_wide.hip, scl_aec_sparse.hip (a lane's model in device memory)
//       encoders: af_code_symbol, AfSymFeed, AfCells16 / af_load16, af_row_counts (sparse), af_next_ctx_k
//       the wide decoder: af_lane_dec_done, af_row_find, AfSymWord
//   every encoder: af_emit; af_put_common (fast, wide, sparse) or af_put_common_flat (iid, static); af_encode_results (all
//   but the iid encoder)
// NOT the split encoder's three roles, nor the static kernels' line I/O.  Kernels that keep their own text of a piece, for a
// measured reason given at the site: aec_iid_encode_kernel (result stores), aec_sparse_decode_kernel (start, literal loops,
// af_row_find, AfSymWord), aec_wide_encode_kernel (af_row_counts).
//
// A decoder's STEP carries its model state (rows in registers, context, addresses) and provides
//   u32 operator()(u32 &low, u32 &hm, u32 state)     decode_step_core and update_model of one symbol: the symbol
// An encoder's MODEL carries c_nx, d_nx, T_nx, x_nx -- (c, d, T, 1 / T) of the symbol issued last, (0, 1, 1, 1.0) at the
// start -- and provides
//   void issue(u32 s)     freqs_current of symbol s: loads only
//   void finish()         update_model, c_nx .. x_nx
//   void code(wr, low, hm, pending, c, d, T, x)     shrink_range and the renormalisation of one symbol
// Both are built in the kernel and come by reference: by value the rows inside them were copied through memory-shaped
// slices (profiles/aec_frame_codegen.txt).
#pragma once
#include <type_traits>

#include "scl_aec_lane_io.h"
#include "scl_aec_math.h"

// ---- encoders: stream bits ------------------------------------------------------------------------------------------
// One step of the literal loops, and the termination: `bit`, then `pending` copies of its inverse.  `lds`: nothing, or the
// ring argument of the line-granular writer (scl_aec_static.hip).
template <class W, class... LDS>
__device__ __forceinline__ void af_emit(W &wr, u32 bit, u32 pending, LDS... lds) {
    wr.put(lds..., bit, 1);
    wr.put_run(lds..., bit ^ 1u, pending);
}

// The field of a closed-form renormalisation, k E1/E2 steps then m E3 steps: b0, then `pending` copies of !b0, then the
// other k - 1 common bits of (low, hm); k + pending <= 32.  Branching form: nothing is put for k = 0.
template <class W>
__device__ __forceinline__ void af_put_common(W &wr, u32 low, u32 k, u32 m, u32 &pending) {
    if (k > 0) {
        const u32 top = low >> (32 - k);
        const u32 b0 = top >> (k - 1);
        const u32 rest = top & ((1u << (k - 1)) - 1u);
        const u32 pat = (1u << pending) - (b0 ^ 1u);  // pending <= 31 here
        wr.put((pat << (k - 1)) | rest, k + pending);
        pending = 0;
    }
    pending += m;
}
// Branch-free form: for k = 0 the field is empty (v = 0, nb = 0) and the pending count just grows.
template <class W, class... LDS>
__device__ __forceinline__ void af_put_common_flat(W &wr, u32 low, u32 k, u32 m, u32 &pending, LDS... lds) {
    const bool any = k != 0;
    const u32 km1 = (k - 1u) & 31u;
    const u32 b0 = low >> 31;
    const u32 rest = __builtin_amdgcn_ubfe(low, (32u - k) & 31u, km1);  // bits 30 .. 32-k of low
    const u32 pat = (1u << pending) - (b0 ^ 1u);                       // pending <= 31 here
    u32 fv = (pat << km1) | rest, fn = k + pending;
    asm volatile("" : "+v"(fv), "+v"(fn));  // computed for every lane: the compiler would turn the selects into a branch
    wr.put_field(lds..., any ? fv : 0u, any ? fn : 0u);
    pending = (any ? 0u : pending) + m;
}

// Arithmetic stage of one symbol, shrink_range (:58-78) and the renormalisation loops (:126-150), in the round-3 forms.
template <class W>
__device__ __forceinline__ void af_code_symbol(W &wr, u32 &low, u32 &hm, u32 &pending, u32 c, u32 d, double x) {
    af_shrink2(low, hm, c, d, x);
    u32 k, m, nlow, nhm;
    const bool edge = af_renorm2(low, hm, k, m, nlow, nhm);
    if (__builtin_expect(edge || (k + pending > 32), 0)) {
        af_renorm_literal_enc(low, hm, pending, [&](u32 bit) { af_emit(wr, bit, pending); });
    } else {
        af_put_common(wr, low, k, m, pending);
        low = nlow;
        hm = nhm;
    }
}

// The stores behind a forward writer's finish(): the stream starts at the start of slot `chunk` and is `total` bits long.
__device__ __forceinline__ void af_encode_results(u64 total, u32 st, u64 chunk, u64 out_stride, u64 *out_bit_off,
                                                  u32 *out_nbits, u32 *status) {
    out_bit_off[chunk] = chunk * out_stride * 8;
    out_nbits[chunk] = (u32)total;
    if (status) status[chunk] = st;
}

// ---- lane encode frame ----------------------------------------------------------------------------------------------
// Header (:92-99), the symbols four per 32-bit load and one word ahead, the software pipeline -- the model reads of a
// symbol are in flight while the previous one is coded --, the drain and the termination (:153-159).  `wr`: the kernel's
// writer, opened on the chunk's slot.  The kernel stores what comes back (af_encode_results, or written out).
struct AfEncoded {
    u64 total;  // stream bits
    u32 st;
};
template <class MODEL, class W>
__device__ __forceinline__ AfEncoded af_lane_encode(MODEL &mdl, W &wr, u32 K, u32 size_bits, const u8 *sym, u64 sym_stride,
                                                    const u32 *lens, u32 chunk_len, u64 chunk) {
    const u32 n = lens ? lens[chunk] : chunk_len;
    const u32 *src = reinterpret_cast<const u32 *>(sym + chunk * sym_stride);
    wr.put(af_header_value(n, size_bits), size_bits);
    u32 st = af_header_status(n, size_bits);
    u32 low = 0, hm = 0xFFFFFFFFu;
    u32 pending = 0;  // E3 steps not yet resolved (<= 32 * n < 2^20)
    // Before the first symbol (c, d, T, 1/T) = (0, 1, 1, 1.0) makes the arithmetic stage a no-op (d == T keeps high,
    // low += 0, nothing to renormalise), so every symbol runs the same body and one more `code` drains it.
    auto emit = [&](u32 bit) { af_emit(wr, bit, pending); };
    u32 nextw = 0;
    const u32 last_word = n ? (n - 1) >> 2 : 0;
    const u32 n_words = (n + 3) >> 2;
    if (n > 0) nextw = src[0];
    for (u32 w = 0; w < n_words; ++w) {
        // The load is unconditional with its index clamped into the chunk and sits where nothing has to be merged with
        // it: a load under a lane-dependent or periodic condition is copied into the loop-carried register at once,
        // i.e. waited for at once (~1 us each).
        u32 word = nextw;
        nextw = src[min(w + 1, last_word)];
        const u32 cnt = min(4u, n - 4 * w);
#pragma unroll 1
        for (u32 j = 0; j < cnt; ++j) {
            u32 s = word & 0xFFu;
            word >>= 8;
            if (s >= K) {
                st |= SCL_ST_SYMBOL;
                s = 0;
            }
            const u32 cc = mdl.c_nx, dd = mdl.d_nx, TT = mdl.T_nx;
            const double xx = mdl.x_nx;
            mdl.issue(s);                                   // this symbol: LDS reads in flight ...
            mdl.code(wr, low, hm, pending, cc, dd, TT, xx, emit);  // ... while the previous symbol is coded
            mdl.finish();
        }
    }
    mdl.code(wr, low, hm, pending, mdl.c_nx, mdl.d_nx, mdl.T_nx, mdl.x_nx, emit);
    af_terminate(low, pending, emit);
    return {wr.finish(), st};
}

// ---- lane decode frame ----------------------------------------------------------------------------------------------
struct AfLaneDec {
    u64 chunk;
    u32 n, st;  // symbols to decode, status as the header left it
    AfReader rd;
};
// The decoders' start (:203-240).  True: this lane is done -- it has no chunk, or the header settled the chunk (its results
// are written, af_decode_length).  Else the reader stands behind the header.  Its own function, `if (..) return;` in the
// kernel, as in scl_ans_frame.h.
template <u32 THREADS>
__device__ __forceinline__ bool af_lane_dec_done(AfLaneDec &f, u32 size_bits, const u8 *in, u64 in_size_bytes,
                                                 const u64 *bit_off, const u32 *in_nbits, u64 n_chunks, u32 out_cap,
                                                 u32 *out_lens, u32 *consumed, u32 *status) {
    f.chunk = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (f.chunk >= n_chunks) return true;
    const u32 nbits = in_nbits[f.chunk];
    f.rd.init(in, in_size_bytes, bit_off[f.chunk], nbits);
    f.n = af_decode_length(f.rd.get(size_bits), f.st, nbits, size_bits, out_cap, f.chunk, out_lens, consumed, status);
    return f.n == 0;
}

// Everything behind the header: the first state, all symbols through `step` and AfSymOut (its 64 bytes per lane at
// `lds_out`), the renormalisation between them (:245-275), consumed bits (:277-282) and status.
template <class STEP>
__device__ __forceinline__ void af_lane_decode(STEP &step, AfLaneDec &f, char *lds_out, u8 *out_row, u32 *consumed,
                                               u32 *status) {
    AfReader &rd = f.rd;
    const u32 n = f.n;
    AfSymOut so;
    so.init(lds_out, threadIdx.x, out_row);
    u32 state = rd.get(32);
    u32 low = 0, hm = 0xFFFFFFFFu;
    // One symbol: the loops run it for all but the last symbol of the chunk, the last one follows them without a
    // renormalisation (the reference breaks before it, :242-243): a single exit test per iteration.
    auto symbol = [&](u32 i) { so.put(step(low, hm, state), i); };  // four to a word, sixteen words to a sector
    // UNCHECKED selects the reader's refill (AfReader::next_word)
    auto renorm = [&](auto unchecked) {
        constexpr bool UC = decltype(unchecked)::value;
        u32 k, m, nlow, nhm;
        const bool edge = af_renorm2_dec(low, hm, k, m, nlow, nhm);
        if (__builtin_expect(edge, 0)) {
            af_renorm_literal_dec(low, hm, state, [&] { return rd.get<UC>(1); });
        } else {
            const u32 kt = k + m;  // <= 31
            state = af_state_shift_in<UC>(rd, state, k, kt);
            low = nlow;
            hm = nhm;
        }
    };
    // The symbol index i is the same for every lane still at work (they start together and only drop out), so it lives in a
    // scalar register.  Stretches: as many symbols as EVERY working lane can decode without reaching the last word of its
    // stream (and has left to decode) run with the unchecked refill and a scalar trip count; the last symbols of the chunks
    // -- and everything, in a wave that holds a very short stream -- run in the checked loop below.
    u32 i = 0;
    for (;;) {
        const bool at_work = i + 1 < n;
        const u32 mine = at_work ? min(rd.safe_symbols(), n - 1 - i) : 0xFFFFFFFFu;
        const u32 cnt = __builtin_amdgcn_readfirstlane(af_wave_min(mine));
        if (cnt == 0xFFFFFFFFu || cnt < 16) break;
        if (at_work) {
            const u32 *before = rd.ptr;
            // four symbols per trip once the index is a multiple of four: which byte of the output word a symbol fills, and
            // when the word is complete, are then known at compile time (AfSymOut::put: no scalar compare-and-branch per
            // symbol), and the trip count is tested once per four
            u32 u = 0;
            for (; u < cnt && ((i + u) & 3u); ++u) {
                symbol(i + u);
                renorm(std::true_type{});
            }
            for (; u + 4 <= cnt; u += 4) {
                const u32 base = i + u;
                __builtin_assume((base & 3u) == 0);
#pragma unroll
                for (u32 q = 0; q < 4; ++q) {
                    symbol(base + q);
                    renorm(std::true_type{});
                }
            }
            for (; u < cnt; ++u) {
                symbol(i + u);
                renorm(std::true_type{});
            }
            rd.settle(before);
        }
        i += cnt;
    }
    for (; i + 1 < n; ++i) {
        symbol(i);
        renorm(std::false_type{});
    }
    symbol(n - 1);
    so.finish(n);
    consumed[f.chunk] = af_consumed_bits(low, hm, state, rd.position());
    if (status) status[f.chunk] = f.st;
}

// ---- order-k models on large alphabets: two-level rows of u16 cells in device memory (scl_aec_wide.hip; the dense rows of
// scl_aec_sparse.hip).  A row is 16 block totals, then the counts in blocks of 16; cells hold count - 1. --------------------
template <class DEV>
__device__ __forceinline__ u32 af_next_ctx_k(const DEV &P, u32 ctx, u32 s) {  // past_k[1:] + [s], :146-151
    if (P.k == 0) return 0;
    if (P.k == 1) return s;
    return (u32)(((u64)ctx * P.K + s) % P.ctx_mod);
}

struct AfCells16 {  // 16 consecutive cells
    u32 v[16];
};
// 16 cells, aligned to their size, as 16-byte loads issued back to back
template <class CELL>
__device__ __forceinline__ AfCells16 af_load16(const CELL *p) {
    static_assert(sizeof(CELL) == 2, "two cells to a 32-bit word");
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    AfCells16 r;
    const uint4 a = q[0], b = q[1];
    const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (u32 j = 0; j < 8; ++j) {
        r.v[2 * j] = w[j] & 0xFFFFu;
        r.v[2 * j + 1] = w[j] >> 16;
    }
    return r;
}

// freqs_current of symbol s (:118) from its row's block totals `bt` and its block of counts `cb`, in cell units
struct AfRowCounts {
    u32 below, tot, fs, fb;  // cells below s, all cells, the symbol's cell, its block's total
};
__device__ __forceinline__ AfRowCounts af_row_counts(const AfCells16 &bt, const AfCells16 &cb, u32 s) {
    const u32 b = s >> 4, w = s & 15u;
    AfRowCounts r = {0, 0, 0, 0};
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        r.tot += bt.v[j];
        r.below += (j < b) ? bt.v[j] : 0u;
        r.below += (j < w) ? cb.v[j] : 0u;
        r.fs = (j == w) ? cb.v[j] : r.fs;
        r.fb = (j == b) ? bt.v[j] : r.fb;
    }
    return r;
}

// The decoder's side: target = ((state - low + 1) * T - 1) // rng (see scl_aec.hip; xr = 1 / rng), clamped for corrupt
// streams, then the largest s with c[s] = s + cells below s <= target -- the block first (c[16 j] = 16 j + totals below),
// a dependent read of that block, then the symbol inside it.
struct AfRowFound {
    u32 s, b, c, fs, fb, T;  // symbol, its block, c[s], the two cells update_model counts up, the row total
};
template <class CELL>
__device__ __forceinline__ AfRowFound af_row_find(const AfCells16 &bt, const CELL *row, u32 K, u32 nblk, u32 state, u32 low,
                                                  double xr) {
    AfRowFound r;
    u32 tot = 0;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) tot += bt.v[j];
    r.T = K + tot;
    const double num = __builtin_fma((double)(state - low) + 1.0, (double)r.T, -0.5);
    u32 tgt = (u32)(num * xr);
    tgt = min(tgt, r.T - 1);
    u32 b = 0, g = 0, run = 0, fb = bt.v[0];
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        const bool take = j < nblk && run <= tgt;
        b = take ? j : b;
        g = take ? run : g;
        fb = take ? bt.v[j] : fb;
        run += 16 + bt.v[j];
    }
    const AfCells16 cb = af_load16(row + 16 + 16 * b);
    const u32 wmax = min(15u, K - 1 - 16 * b);
    u32 w = 0, c = g, fs = cb.v[0];
    run = g;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        const bool take = j <= wmax && run <= tgt;
        w = take ? j : w;
        c = take ? run : c;
        fs = take ? cb.v[j] : fs;
        run += 1 + cb.v[j];
    }
    r.s = 16 * b + w;
    r.b = b;
    r.c = c;
    r.fs = fs;
    r.fb = fb;
    return r;
}

// The encoders' symbols: four per 32-bit load, two words ahead (the rows of symbol i + 1 are issued before symbol i is
// counted).  A symbol outside the alphabet is reported and coded as 0.
struct AfSymFeed {
    const u32 *src;
    u32 last_word, word_a, word_b;
    __device__ __forceinline__ u32 first(const u8 *row, u32 n, u32 K, u32 &st) {
        src = reinterpret_cast<const u32 *>(row);
        last_word = n ? (n - 1) >> 2 : 0;
        word_a = src[0];
        word_b = src[min(1u, last_word)];
        const u32 s = word_a & 0xFFu;
        if (n > 0 && s >= K) st |= SCL_ST_SYMBOL;
        return (s >= K) ? 0u : s;
    }
    // symbol inx = 1, 2, ... in turn; also past the end of the chunk (what is read for it is never used)
    __device__ __forceinline__ u32 next(u32 inx, u32 n, u32 K, u32 &st) {
        if ((inx & 3u) == 0) {
            word_a = word_b;
            word_b = src[min((inx >> 2) + 1, last_word)];
        }
        const u32 s = (word_a >> (8 * (inx & 3u))) & 0xFFu;
        if (inx < n && s >= K) st |= SCL_ST_SYMBOL;
        return (s >= K) ? 0u : s;
    }
};

// The decoders' symbols: four to a word, one 4-byte store per word (these kernels wait on their tables, not on this).
struct AfSymWord {
    u32 *dst;
    u32 oword;
    __device__ __forceinline__ void init(u8 *row) {
        dst = reinterpret_cast<u32 *>(row);
        oword = 0;
    }
    __device__ __forceinline__ void put(u32 s, u32 i) {
        oword |= s << (8 * (i & 3));
        if ((i & 3) == 3) {
            dst[i >> 2] = oword;
            oword = 0;
        }
    }
    __device__ __forceinline__ void finish(u32 n) {  // last, partial word (zero-padded inside the row)
        if ((n & 3) != 0) dst[(n - 1) >> 2] = oword;
    }
};
