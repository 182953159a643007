// scl_aec_static.hip -- arithmetic coding with a STATIC frequency model (FixedFreqModel) for gfx950, one wavefront
// lane per chunk.  Same streams, bit for bit, as scl_aec.hip and the reference:
//   ArithmeticEncoder.shrink_range / encode_block   scl/compressors/arithmetic_coding.py:58-78, :80-161
//   ArithmeticDecoder.decode_step_core / decode_block                               :177-201, :203-287
//   FixedFreqModel                                   scl/compressors/probability_models.py:57-67
//
// Served models (aec_static_ok): PRECISION = 32, alphabet 2..256, total <= 2^16.
// The model is read-only, so nothing is private to a lane but its interval: the {c, c + f} table (and, for totals
// up to 4096, a slot -> symbol table for the decoder) sits in LDS once per workgroup, and the kernels run at the
// occupancy of the rANS fast kernels with their line-granular I/O (scl_ans_fast_io.h): symbols arrive as whole
// 128-byte lines, stream words pass through a per-lane LDS ring and leave / arrive as whole lines.
// Arithmetic as in scl_aec_fast.hip (scl_aec_math.h): (rng*c)//T in exact binary64 with ONE reciprocal of T per
// launch, closed-form renormalisation, literal loops of the reference on its strict-comparison corners.
#include "scl_aec_internal.h"
#include "scl_aec_frame.h"
#include "scl_ans_fast_io.h"

#define AS_THREADS 256
#define AS_RING_BYTES (32 * AS_THREADS * 4)
#define AS_TAB_BASE AS_RING_BYTES         // uint2 {c, c + f} per symbol
#define AS_LUT_BASE (AS_TAB_BASE + 2048)  // u8 symbol per slot (totals <= 4096)
#define AS_LDS_BYTES (AS_LUT_BASE + 4096)

struct AecStaticDev {
    u32 K, T;
    u32 t;          // log2(T) when T is a power of two (the POW2 kernels), else unused
    u32 size_bits;  // DATA_BLOCK_SIZE_BITS (1..32)
    const u32 *d_freq, *d_cum;
};

__device__ __forceinline__ void as_setup_tables(char *lds, const AecStaticDev &P, u32 tid, bool with_lut) {
    if (tid < P.K) {
        const u32 c = P.d_cum[tid], f = P.d_freq[tid];
        *reinterpret_cast<uint2 *>(lds + AS_TAB_BASE + tid * 8) = make_uint2(c, c + f);
        if (with_lut)
            for (u32 j = 0; j < f; ++j) *reinterpret_cast<u8 *>(lds + AS_LUT_BASE + c + j) = (u8)tid;
    } else if (tid < 256) {
        *reinterpret_cast<uint2 *>(lds + AS_TAB_BASE + tid * 8) = make_uint2(0, 1);  // never selected
    }
    __syncthreads();
}

// The ENCODER's table for power-of-two totals: 16-byte entries {c, 0, d, 0} -- both counts arrive zero-extended to 64 bits in
// aligned register pairs, which is how v_mad_u64_u32 (af_shrink_pow2_wide) takes its addend: four register copies per symbol
// otherwise.  (36 KiB of LDS per workgroup: still four per CU.  The decoder has no room for it next to its slot table.)
__device__ __forceinline__ void as_setup_table16(char *lds, const AecStaticDev &P, u32 tid) {
    if (tid < P.K) {
        const u32 c = P.d_cum[tid], f = P.d_freq[tid];
        *reinterpret_cast<uint4 *>(lds + AS_TAB_BASE + tid * 16) = make_uint4(c, 0u, c + f, 0u);
    } else if (tid < 256) {
        *reinterpret_cast<uint4 *>(lds + AS_TAB_BASE + tid * 16) = make_uint4(0u, 0u, 1u, 0u);  // never selected
    }
    __syncthreads();
}
typedef AnsFwdWriter<AS_THREADS> AsOut;
typedef AnsBitReader<AS_THREADS, true> AsIn;

// one symbol of the encoder: shrink_range, then the renormalisation loops (:126-150)
template <bool POW2>
__device__ __forceinline__ void as_encode_symbol(u32 &low, u32 &hm, u32 &pending, u64 c, u64 d, u32 t, double xT,
                                                 AsOut &wr, char *lds) {
    if (POW2)
        af_shrink_pow2_wide(low, hm, c, d, t);
    else
        af_shrink2(low, hm, (u32)c, (u32)d, xT);
    u32 k, m, nlow, nhm;
    const bool edge = af_renorm2_dec(low, hm, k, m, nlow, nhm);  // the conservative corner test: two compares fewer
    const bool rare = edge | (k + pending > 32);                 // one condition, one branch
    if (__builtin_expect(rare, 0)) {
        af_renorm_literal_enc(low, hm, pending, [&](u32 bit) {
            af_emit(wr, bit, pending, lds);
            wr.maybe_flush(lds);
        });
    } else {
        af_put_common_flat(wr, low, k, m, pending, lds);
        low = nlow;
        hm = nhm;
    }
}

// POW2: the total is a power of two, shrink_range in integers (af_shrink_pow2)
template <bool POW2>
__global__ void __launch_bounds__(AS_THREADS, 4)
    aec_static_encode_kernel(AecStaticDev P, const u8 *__restrict__ sym, u64 sym_stride, const u32 *__restrict__ lens,
                             u32 chunk_len, u64 n_chunks, u8 *__restrict__ out, u64 out_stride,
                             u64 *__restrict__ out_bit_off, u32 *__restrict__ out_nbits, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[AS_TAB_BASE + (POW2 ? 4096 : 2048)];
    const u32 tid = threadIdx.x;
    if (POW2)
        as_setup_table16(lds, P, tid);
    else
        as_setup_tables(lds, P, tid, false);
    const u64 chunk = (u64)blockIdx.x * AS_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 n = lens ? lens[chunk] : chunk_len;
    const u8 *src = sym + chunk * sym_stride;
    const double xT = af_recip((double)P.T);
    AsOut wr;
    wr.init(tid, out + chunk * out_stride);
    wr.put(lds, af_header_value(n, P.size_bits), P.size_bits);  // :92-99
    u32 low = 0, hm = 0xFFFFFFFFu, pending = 0, bad = 0;

    auto code_word = [&](u32 w, u32 cnt) {  // up to four symbols, first symbol in the low byte
#pragma unroll 1
        for (u32 j = 0; j < cnt; ++j) {
            u32 s = w & 0xFFu;
            w >>= 8;
            bad = max(bad, s);
            s = (s < P.K) ? s : 0u;
            if (POW2) {
                const uint4 e = *reinterpret_cast<const uint4 *>(lds + AS_TAB_BASE + s * 16);  // {c, 0, d, 0}
                as_encode_symbol<POW2>(low, hm, pending, e.x | ((u64)e.y << 32), e.z | ((u64)e.w << 32), P.t, xT, wr, lds);
            } else {
                const uint2 e = *reinterpret_cast<const uint2 *>(lds + AS_TAB_BASE + s * 8);
                as_encode_symbol<POW2>(low, hm, pending, e.x, e.y, P.t, xT, wr, lds);
            }
        }
        wr.maybe_flush(lds);  // <= 4 new words per fast-path call on top of <= 15 pending (ring of 32)
    };

    const u32 n_lines = n >> 7;
    const uint4 *src16 = reinterpret_cast<const uint4 *>(src);
    Line128 cur;  // no second buffer: with it the kernel needs more than its 128 registers (4 waves per SIMD hide the load)
#pragma nounroll
    for (u32 t = 0; t < n_lines; ++t) {
        cur.load(src16 + 8 * t);
#pragma unroll 1
        for (u32 q = 0; q < 8; ++q) {
            const uint4 v = cur.v[0];
#pragma unroll
            for (int i = 0; i < 7; ++i) cur.v[i] = cur.v[i + 1];
            code_word(v.x, 4);
            code_word(v.y, 4);
            code_word(v.z, 4);
            code_word(v.w, 4);
        }
    }
    u32 i = n_lines << 7;
    for (; i + 4 <= n; i += 4) code_word(*reinterpret_cast<const u32 *>(src + i), 4);  // ragged tail
    if (i < n) {
        u32 w = 0;
        for (u32 j = 0; i + j < n; ++j) w |= (u32)src[i + j] << (8 * j);
        code_word(w, n - i);
    }
    af_terminate(low, pending, [&](u32 bit) { af_emit(wr, bit, pending, lds); });  // :153-159
    af_encode_results(wr.finish(lds), ((bad >= P.K) ? SCL_ST_SYMBOL : 0u) | af_header_status(n, P.size_bits), chunk, out_stride,
                      out_bit_off, out_nbits, status);
}

// LUT = true: total <= 4096, the decoder's search is one byte read by target slot; else a binary search on c
template <bool LUT, bool POW2>
__global__ void __launch_bounds__(AS_THREADS, 4)
    aec_static_decode_kernel(AecStaticDev P, const u8 *__restrict__ in, u64 in_size_bytes,
                             const u64 *__restrict__ bit_off, const u32 *__restrict__ in_nbits, u64 n_chunks,
                             u8 *__restrict__ out_sym, u64 out_stride, u32 out_cap, u32 *__restrict__ out_lens,
                             u32 *__restrict__ consumed, u32 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char lds[LUT ? AS_LDS_BYTES : AS_TAB_BASE + 2048];
    const u32 tid = threadIdx.x;
    as_setup_tables(lds, P, tid, LUT);
    const u64 chunk = (u64)blockIdx.x * AS_THREADS + tid;
    if (chunk >= n_chunks) return;
    const u32 nbits = in_nbits[chunk];
    u32 st;
    if (nbits < P.size_bits) {  // refused without opening the stream (af_decode_length's first test, ahead of rd.init)
        out_lens[chunk] = 0;
        consumed[chunk] = 0;
        if (status) status[chunk] = SCL_ST_TRUNCATED;
        return;
    }
    AsIn rd;
    rd.init(in, in_size_bytes, bit_off[chunk], lds, tid, nbits);
    const u32 n = af_decode_length(rd.get(lds, P.size_bits), st, nbits, P.size_bits, out_cap, chunk, out_lens, consumed,
                                   status);
    if (n == 0) return;
    rd.maybe_refill(lds);
    const double xT = af_recip((double)P.T), Td = (double)P.T;
    u8 *dst = out_sym + chunk * out_stride;
    u32 used = 32;
    u32 state = rd.get(lds, 32);
    u32 low = 0, hm = 0xFFFFFFFFu;

    // one symbol: decode_step_core (:177-201) and, unless it is the last one, the renormalisation (:245-275)
    auto decode_symbol = [&](bool last) -> u32 {
        const double xr = af_recip((double)(hm - low) + 1.0);
        const double num = __builtin_fma((double)(state - low) + 1.0, Td, -0.5);
        // ((state - low + 1) * T - 1) // rng, see scl_aec.hip.  low <= state <= hm holds for ANY input bits (the symbol chosen
        // is the one whose interval holds the state), so target <= T - 1: no clamp
        const u32 tgt = (u32)(num * xr);
        u32 s;
        if (LUT) {
            s = *reinterpret_cast<const u8 *>(lds + AS_LUT_BASE + tgt);
        } else {  // largest s with c[s] <= tgt
            s = 0;
#pragma unroll
            for (u32 b = 128; b > 0; b >>= 1) {
                const u32 t = s + b;
                const u32 ct = *reinterpret_cast<const u32 *>(lds + AS_TAB_BASE + min(t, 255u) * 8);
                s = (t < P.K && ct <= tgt) ? t : s;
            }
        }
        const uint2 e = *reinterpret_cast<const uint2 *>(lds + AS_TAB_BASE + s * 8);
        if (POW2)
            af_shrink_pow2(low, hm, e.x, e.y, P.t);
        else
            af_shrink2(low, hm, e.x, e.y, xT);
        if (last) return s;
        u32 k, m, nlow, nhm;
        const bool edge = af_renorm2_dec(low, hm, k, m, nlow, nhm);
        if (__builtin_expect(edge, 0)) {
            af_renorm_literal_dec(low, hm, state, [&] {
                used++;
                return rd.get(lds, 1);
            });
            rd.maybe_refill(lds);
        } else {
            const u32 kt = k + m;  // <= 31
            // kt bits come in from the stream: {state, look} << kt in one 64-bit shift (kt may be 0)
            const u64 both = (((u64)state << 32) | rd.look()) << kt;
            const u32 keep = (state << k) & AF_HALF;
            rd.advance(lds, kt);
            state = ((u32)(both >> 32) & 0x7FFFFFFFu) | keep;
            low = nlow;
            hm = nhm;
            used += kt;
        }
        return s;
    };

    // whole 128-byte lines of output (eight registers, one burst), then the ragged tail byte by byte
    u32 i = 0;
    const u32 n_full = n & ~127u;
#pragma nounroll
    for (; i < n_full; i += 128) {
        uint4 a[8];
#pragma unroll 1
        for (u32 q = 0; q < 8; ++q) {
            u32 w4[4];
#pragma unroll 1
            for (u32 g = 0; g < 4; ++g) {
                u32 w = 0;
#pragma unroll 1
                for (u32 j = 0; j < 4; ++j) {
                    const bool last = (i + 16 * q + 4 * g + j + 1 == n);
                    w |= decode_symbol(last) << (8 * j);
                }
                rd.maybe_refill(lds);  // <= 4 words consumed by four fast-path symbols
                // rotate instead of indexing: w4[g] with a run-time g would go through scratch
                w4[0] = w4[1], w4[1] = w4[2], w4[2] = w4[3], w4[3] = w;
            }
#pragma unroll
            for (int r = 0; r < 7; ++r) a[r] = a[r + 1];
            a[7] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
        uint4 *p = reinterpret_cast<uint4 *>(dst + i);
#pragma unroll
        for (int b = 0; b < 8; ++b) p[b] = a[b];
    }
    for (; i < n; ++i) {
        dst[i] = (u8)decode_symbol(i + 1 == n);
        if ((i & 3u) == 3u) rd.maybe_refill(lds);
    }
    consumed[chunk] = af_consumed_bits(low, hm, state, (u64)used + P.size_bits);  // :277-282
    if (status) status[chunk] = st;
}

// ---- host side ----------------------------------------------------------------------------------------------
bool aec_static_ok(const scl_aec_model *m) {
    const AecDev &d = m->dev;
    return d.kind == SCL_MODEL_FIXED && d.K >= 2 && d.K <= 256 && d.P == 32 &&
           d.total0 <= 65536 && (u64)d.total0 < d.max_total;
}

static AecStaticDev aec_static_dev(const scl_aec_model *m) {
    AecStaticDev f;
    f.K = m->dev.K;
    f.T = m->dev.total0;
    f.t = (f.T & (f.T - 1)) == 0 ? scl_bit_width_u64(f.T) - 1 : 0xFFFFFFFFu;
    f.size_bits = m->dev.size_bits;
    f.d_freq = m->dev.d_freq;
    f.d_cum = m->dev.d_cum;
    return f;
}

void aec_static_encode_launch(const scl_aec_model *m, const SclEncodeArgs<u8> &a, hipStream_t st, u32 *) {
    const SclGrid g = aec_grid(a.n_chunks, AS_THREADS);
    const AecStaticDev dev = aec_static_dev(m);
    if (dev.t != 0xFFFFFFFFu)
        scl_launch_encode(aec_static_encode_kernel<true>, g, st, dev, a);
    else
        scl_launch_encode(aec_static_encode_kernel<false>, g, st, dev, a);
}

void aec_static_decode_launch(const scl_aec_model *m, const SclDecodeArgs<u8> &a, hipStream_t st, u32 *) {
    const SclGrid g = aec_grid(a.n_chunks, AS_THREADS);
    const AecStaticDev dev = aec_static_dev(m);
    const bool pow2 = dev.t != 0xFFFFFFFFu;
#define AS_LAUNCH_DEC(LUT, POW2) scl_launch_decode(aec_static_decode_kernel<LUT, POW2>, g, st, dev, a)
    if (m->dev.total0 <= 4096) {
        if (pow2)
            AS_LAUNCH_DEC(true, true);
        else
            AS_LAUNCH_DEC(true, false);
    } else {
        if (pow2)
            AS_LAUNCH_DEC(false, true);
        else
            AS_LAUNCH_DEC(false, false);
    }
#undef AS_LAUNCH_DEC
}
