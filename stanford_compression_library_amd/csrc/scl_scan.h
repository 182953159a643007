// scl_scan.h -- the exclusive scans of csrc/: across a wavefront, across a workgroup, and one workgroup over an array.
// Every kernel that needs a prefix sum or a running maximum calls these (compaction in scl_core.hip, the prefix-block
// kernels, the LZ77 index, wide and entropy kernels); there is no other scan code.  Internal to csrc/.
#pragma once

#include "scl_common.h"

#ifdef __HIPCC__
// An operator is a type with an identity and an associative combine; T is u32 or u64.  exclusive(): a lane's exclusive
// value from its inclusive one across the wavefront.
struct SclScanSum {
    template <typename T>
    static __device__ __forceinline__ T identity() {
        return T(0);
    }
    template <typename T>
    static __device__ __forceinline__ T combine(T a, T b) {
        return a + b;
    }
    template <typename T>
    static __device__ __forceinline__ T exclusive(T incl, T v) {
        return incl - v;
    }
};

struct SclScanMax {
    template <typename T>
    static __device__ __forceinline__ T identity() {
        return T(0);  // unsigned values
    }
    template <typename T>
    static __device__ __forceinline__ T combine(T a, T b) {
        return a > b ? a : b;
    }
    template <typename T>
    static __device__ __forceinline__ T exclusive(T incl, T) {  // max has no inverse: the inclusive value of the lane before
        const T before = __shfl_up(incl, 1);
        return (threadIdx.x & (SCL_WAVE - 1)) ? before : identity<T>();
    }
};

// inclusive scan across the 64 lanes of the wavefront: log2(64) shuffles
template <typename T, typename Op>
__device__ __forceinline__ T scl_wave_scan_incl(T v) {
    const u32 lane = threadIdx.x & (SCL_WAVE - 1);
    T incl = v;
#pragma unroll
    for (u32 d = 1; d < SCL_WAVE; d <<= 1) {
        const T up = __shfl_up(incl, d);
        if (lane >= d) incl = Op::combine(up, incl);
    }
    return incl;
}

// Exclusive scan across the wavefront; *total = the combination of all 64 values, in every lane.
template <typename T, typename Op>
__device__ __forceinline__ T scl_wave_scan_excl(T v, T *total) {
    const T incl = scl_wave_scan_incl<T, Op>(v);
    *total = __shfl(incl, SCL_WAVE - 1);
    return Op::exclusive(incl, v);
}

// Exclusive scan across a workgroup of NT threads (one-dimensional; EVERY thread calls); *total = the combination of all NT
// values, in every thread.  One LDS word per wave and two barriers: behind the second one s_wave may be written again,
// so calls can follow each other at once.
template <typename T, int NT, typename Op>
__device__ __forceinline__ T scl_block_scan_excl(T v, T *s_wave /* [NT / 64] */, T *total) {
    static_assert(NT > 0 && NT % SCL_WAVE == 0, "whole wavefronts");
    const u32 lane = threadIdx.x & (SCL_WAVE - 1), wave = threadIdx.x / SCL_WAVE;
    const T incl = scl_wave_scan_incl<T, Op>(v);
    if (lane == SCL_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    T base = Op::template identity<T>(), all = Op::template identity<T>();
#pragma unroll
    for (u32 i = 0; i < NT / SCL_WAVE; ++i) {
        const T x = s_wave[i];
        if (i < wave) base = Op::combine(base, x);
        all = Op::combine(all, x);
    }
    __syncthreads();
    *total = all;
    return Op::combine(base, Op::exclusive(incl, v));
}

// ONE workgroup of NT threads: v[0..n) becomes its exclusive scan, in trips of NT values with a carried prefix; returns
// the combination of all n values to every thread.
template <typename T, int NT, typename Op>
__device__ __forceinline__ T scl_block_scan_array(T *v, u64 n, T *s_wave /* [NT / 64] */) {
    T carry = Op::template identity<T>();
    for (u64 at = 0; at < n; at += NT) {
        const u64 i = at + threadIdx.x;
        const T x = i < n ? v[i] : Op::template identity<T>();
        T total;
        const T ex = scl_block_scan_excl<T, NT, Op>(x, s_wave, &total);
        if (i < n) v[i] = Op::combine(carry, ex);
        carry = Op::combine(carry, total);
    }
    return carry;
}
#endif  // __HIPCC__
