// scl_ans_frame.h -- what stands around the per-symbol step of the lane-per-chunk ANS kernels.  Internal to csrc/.
//
// Who uses what:
//   rANS (scl_rans_fast.hip), rANS-b (scl_rans_fast_b.hip), tANS tables (scl_tans_fast.hip)
//       decoders: ans_decode_refuse, ans_decode_open, ans_decode_rows<STEP>, ans_decode_close
//       host: ans_fill_dec_slots, ans_release_groups (the two rANS units), ans_wide_workgroups / ans_grid
//   encoders of scl_rans_fast.hip and the any-parameter kernels (scl_rans.hip, scl_tans.hip)   ans_encode_results
// NOT the range decoder's frame (scl_range_fast.hip): its symbols come out forwards, its header is a fixed 64 bits and it
// rejects the cooperative store; nor the arithmetic coders'.  NOT the encoders' header puts either: the three tuned
// encoders write state and size through two put32 signatures, and the AnsBackWriter encoders (scl_rans_fast_b.hip,
// scl_tans_fast.hip) keep even their result stores -- a function around them measured slower there
// (profiles/ans_frame_codegen.txt).
//
// The pieces, each defined once:
//   ans_decode_refuse   header-does-not-fit exit
//   ans_decode_open     reader init (linear or striped), n and x from the header, out_lens, capacity
//   ans_decode_rows     symbols last-first: ragged head in single symbols, 16-byte blocks up to a line boundary, then whole
//                       128-byte lines through CoopLineStore
//   ans_decode_close    consumed / status, with the truncated-before-state rule
//   ans_encode_results  the three stores behind a back writer's finish()
// A decoder's STEP holds the constants of its symbol step and provides
//   u8 symbol(x, r, lds)                     one symbol, the reader advanced
//   uint4 block16<REFILL>(x, r, lds)         16 symbols, last first, byte i = symbol i; REFILL: top the ring up afterwards
//   static constexpr bool SPARSE_REFILL      the line loop asks for a refill after every second block only
#pragma once
#include "scl_ans_fast_io.h"

#ifdef __HIPCC__
// True: the header does not fit in the chunk's `avail` bits; the chunk's three results are written and the lane is done.
// (Its own function, `if (ans_decode_refuse(..)) return;` in the kernel: as the false branch of a bool ans_decode_open the
// exit cost every decoder registers -- profiles/ans_frame_codegen.txt.)
template <class DEV>
__device__ __forceinline__ bool ans_decode_refuse(const DEV &P, u32 avail, u64 c, u32 *out_lens, u32 *consumed, u32 *status) {
    if (avail >= P.size_bits + P.nsb) return false;
    out_lens[c] = 0;
    consumed[c] = P.size_bits + P.nsb;
    if (status) status[c] = SCL_ST_TRUNCATED;
    return true;
}

// `r` stands behind the header afterwards; n symbols are to be decoded (0 when they exceed out_cap: st = SCL_ST_CAPACITY,
// else st = 0) from state x.
template <bool STRIPED, class DEV, class DecIn>
__device__ __forceinline__ void ans_decode_open(const DEV &P, DecIn &r, char *lds, const u8 *in, u64 in_size_bytes,
                                                const u64 *bit_off, u64 c, u32 out_cap, u32 &n, u32 &x, u32 &st,
                                                u32 *out_lens) {
    if constexpr (STRIPED)
        r.init(in, in_size_bytes, c, bit_off[c], lds, threadIdx.x);
    else
        r.init(in, in_size_bytes, bit_off[c], lds, threadIdx.x);
    n = r.get(lds, P.size_bits);
    x = r.get(lds, P.nsb);
    out_lens[c] = n;
    st = 0;
    if (n > out_cap) {
        st |= SCL_ST_CAPACITY;
        n = 0;
    }
}

// (the step comes by value: by reference every decoder of scl_rans_fast.hip drifted further from its own loops)
template <class STEP, class DecIn>
__device__ __forceinline__ void ans_decode_rows(const STEP s, u32 &x, DecIn &r, char *lds, u32 n, u8 *out_sym, u64 c,
                                                u64 out_stride) {
    u8 *dst = out_sym + c * out_stride;
    // symbols come out last-first (rANS.py:291): the ragged head of the last 16-byte block ...
    u32 i = n;
    while (i & 15u) {
        dst[--i] = s.symbol(x, r, lds);
        if ((i & 3u) == 0) r.maybe_refill(lds);
    }
    // ... whole 16-byte blocks up to a line boundary ...
    while (i & 127u) {
        const uint4 v = s.template block16<true>(x, r, lds);
        i -= 16;
        *reinterpret_cast<uint4 *>(dst + i) = v;
    }
    // ... then one full 128-byte line per iteration, eight registers: stored cooperatively by the wave when every
    // lane is here with the same position (CoopLineStore, scl_ans_fast_io.h), else as a burst of eight 16-byte stores
    CoopLineStore cs;
    cs.init(out_sym, c, out_stride, i);
#pragma nounroll
    while (i) {
        uint4 a[8];
#pragma unroll
        for (int b = 7; b >= 0; --b)
            a[b] = ((b & 1) && STEP::SPARSE_REFILL) ? s.template block16<false>(x, r, lds)
                                                    : s.template block16<true>(x, r, lds);
        i -= 128;
        if (cs.on) {
            cs.store(a, i);
        } else {
            uint4 *p = reinterpret_cast<uint4 *>(dst + i);
#pragma unroll
            for (int b = 0; b < 8; ++b) p[b] = a[b];
        }
    }
}

// st_header: the status as the header left it (nothing between the header and here changes it).  A stream that ran out is
// truncated and says nothing about its state; a chunk whose header was refused decoded nothing, so its state is not judged.
// x: the final state as the stream carries it (the caller shifts a top-aligned one back).
__device__ __forceinline__ void ans_decode_close(u32 used_bits, u32 avail, u32 st_header, u32 x, u32 L, u64 c,
                                                 u32 *consumed, u32 *status) {
    u32 st = st_header;
    if (used_bits > avail) st |= SCL_ST_TRUNCATED;
    else if (st_header == 0 && x != L) st |= SCL_ST_STATE;  // assert state == INITIAL_STATE (rANS.py:295, tANS.py:277)
    consumed[c] = used_bits;
    if (status) status[c] = st;
}

// The stores behind a back writer's finish(): the stream ends at the end of slot c and is `total` bits long.
__device__ __forceinline__ void ans_encode_results(u64 total, u32 st, u64 c, u64 out_stride, u64 *out_bit_off,
                                                   u32 *out_nbits, u32 *status) {
    out_bit_off[c] = (c + 1) * out_stride * 8 - total;
    out_nbits[c] = (u32)total;
    if (status) status[c] = st;
}

#endif  // __HIPCC__

// ---- host side ------------------------------------------------------------------------------------------------------
// Workgroup size of the kernels that come in two: 1024 lanes (one workgroup per CU, tables staged once) for batches that
// fill the chip that way; up to 2 x 256 small workgroups are resident at once on 256 CUs, so batches of up to 131 072
// chunks take 256-lane workgroups and spread over all CUs instead.
#define ANS_THREADS_WIDE 1024
#define ANS_THREADS_SMALL 256
static inline bool ans_wide_workgroups(u64 n_chunks) { return n_chunks > 2ull * 256 * ANS_THREADS_SMALL; }
static inline SclGrid ans_grid(u64 n_chunks, u32 threads) { return {(u32)((n_chunks + threads - 1) / threads), threads}; }

// rANS decode slot table: slot -> {f | sym << 24, slot - cum}
static inline void ans_fill_dec_slots(uint2 *dec, const u32 *h_freq, const u32 *h_cum, u32 K) {
    for (u32 s = 0; s < K; ++s)
        for (u32 j = 0; j < h_freq[s]; ++j) dec[h_cum[s] + j] = make_uint2(h_freq[s] | (s << 24), j);
}

// NUM_BITS_OUT = b > 1: shrink_state (rANS.py:149-161) releases k_lo groups of b bits at x = L and at most one more at
// x = H, given a1 = max_shrunk_state + 1 (rANS.py:112).  False: more than one (cannot happen: H < L 2^b) or more than
// max_bits bits in all.
static inline bool ans_release_groups(u64 L, u64 H, u64 a1, u32 b, u32 max_bits, u32 *k_lo_out) {
    u32 k_lo = 0, k_hi = 0;
    while ((L >> (k_lo * b)) >= a1) ++k_lo;
    while ((H >> (k_hi * b)) >= a1) ++k_hi;
    *k_lo_out = k_lo;
    return k_hi <= k_lo + 1 && (k_lo + 1) * b <= max_bits;
}
