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
// ---- issue priority of the waves of a SIMD (profiles/wave_progress_timing.txt) -------------------------
// The headline batch puts four waves with the same work on every SIMD.  VALU issue between them goes by priority, then by
// age: at equal priority the oldest wave wins every contested slot, runs ahead and leaves; the SIMD then ends the kernel
// with three, two and one wave, which cannot cover the state chain's latency (measured: the oldest wave of a SIMD lived 0.59
// of the SIMD's span in the striped encoder, 0.69 in the 1024-lane decoder).  The line loops of those two kernels therefore
// set the priority anew for every 128-symbol line:
//   priority = (slot + lines still to go) & 3,  slot = HW_ID.wave_id, the wave's place on its SIMD -- not threadIdx: a
//   workgroup's waves start at a varying SIMD, and the striped encoder's four waves of a SIMD belong to four workgroups.
// Every wave is the winner a quarter of the time, and the count FALLS with progress: a wave that gets a line ahead of the
// others drops a step (three times out of four) and is caught up with.  Counting upwards measured 1.2 % slower in the
// encoder: there a wave that is ahead rises, ties with its neighbour and wins the tie by age.
//   SCL_WAVE_PRIO_ENC / _DEC = 1 that rotation (the default), 0 nothing (device code as before the rotation existed: the
//   "before" build of tools/wave_lifetimes.py), 2 priority 3 - slot set once (the other candidate of the timing note: it
//   hands the oldest wave what it takes anyway and changes nothing).
// Priority only steers the scheduler: behind the table-staging barrier neither kernel has a cross-wave dependency.
#ifndef SCL_WAVE_PRIO_ENC
#define SCL_WAVE_PRIO_ENC 1
#endif
#ifndef SCL_WAVE_PRIO_DEC
#define SCL_WAVE_PRIO_DEC 1
#endif
__device__ __forceinline__ u32 scl_wave_slot() { return __builtin_amdgcn_s_getreg(4 | (0 << 6) | (3 << 11)) & 3u; }  // HW_ID[3:0]
// p: the same in every active lane.  s_setprio takes an immediate and ignores EXEC, so the branches must be scalar ones.
__device__ __forceinline__ void scl_wave_prio(u32 p) {
    const u32 u = (u32)__builtin_amdgcn_readfirstlane((int)p) & 3u;
    if (u == 0) __builtin_amdgcn_s_setprio(0);
    else if (u == 1) __builtin_amdgcn_s_setprio(1);
    else if (u == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}
template <int MODE>
__device__ __forceinline__ u32 scl_wave_prio_enter() {  // once, behind the table staging; returns the rank for the line loop
    if constexpr (MODE == 0) return 0u;
    const u32 r = scl_wave_slot();
    if constexpr (MODE == 2) scl_wave_prio(3u - r);
    return r;
}
template <int MODE>
__device__ __forceinline__ void scl_wave_prio_line(u32 rank, u32 lines_left) {  // at the top of every line
    if constexpr (MODE == 1) scl_wave_prio(rank + lines_left);
}

#ifdef SCL_WAVE_TRACE
// tools/wave_lifetimes.py only: lane 0 of every wave records where it ran and when its main work began and ended.  The tool
// sets the two symbols (scl_wave_trace_set, scl_rans_fast.hip); without the macro nothing of this exists.
static __device__ unsigned long long *scl_wave_trace_buf;
static __device__ unsigned scl_wave_trace_cap;  // waves the buffer has room for
__device__ __forceinline__ u64 scl_wave_trace_now() { return __builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ void scl_wave_trace_put(u64 t0) {
    const u64 t1 = __builtin_amdgcn_s_memtime();
    const u32 hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));   // HW_ID
    const u32 xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));  // XCC_ID[3:0]
    const u32 w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0 && scl_wave_trace_buf && w < scl_wave_trace_cap) {
        unsigned long long *p = scl_wave_trace_buf + 4ull * w;
        p[0] = hw | ((u64)xcc << 32);
        p[1] = t0;
        p[2] = t1;
        p[3] = 1ull + w;
    }
}
#endif

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
// PRIO: the wave-priority mode of the line loop (scl_wave_prio_*, above); 0 for every decoder but the 1024-lane rANS / tANS one.
template <int PRIO = 0, class STEP, class DecIn>
__device__ __forceinline__ void ans_decode_rows(const STEP s, u32 &x, DecIn &r, char *lds, u32 n, u8 *out_sym, u64 c,
                                                u64 out_stride) {
    [[maybe_unused]] const u32 rank = scl_wave_prio_enter<PRIO>();
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
        scl_wave_prio_line<PRIO>(rank, i >> 7);  // (the first active lane's count)
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
