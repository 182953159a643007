// scl_lz77_entropy_internal.h -- what the two entropy stages of LZ77 share: the field alphabets, the log-scale binning, the
// Elias-delta codeword of a count, the tree storage, the one-lane bit readers, the encoders' step from histograms to code
// tables (lze_build_codes) and the decoders' counts parser (lze_parse_counts).  scl_lz77_entropy.hip gives a stream one
// wavefront, scl_lz77_entropy_wide.hip gives ONE stream the whole GPU; both code the same bits.
// Internal to csrc/.
#pragma once

#include "scl_lz77_huffman.h"
#include "scl_lz77_internal.h"

#define LZE_FIELD_K 64u     // room for a sequence field's alphabet: 32 bins + binned_offset <= 32
#define LZE_LIT_BASE (3 * LZE_FIELD_K)
#define LZE_SYMS (LZE_LIT_BASE + 256u)

#ifdef __HIPCC__
// log-scale binning (lz77.py:237-264): v < o is its own bin, else bin o + floor(log2(v - o + 1)) and `log` residual bits.
// A bin past the alphabet (o = 0 and v = 2^32 - 1: the reference's "too large") comes back as it is: the caller refuses it.
__device__ __forceinline__ u32 lze_bin(u32 v, u32 o, u32 *log, u32 *residual) {
    if (v < o) {
        *log = 0;
        *residual = 0;
        return v;
    }
    const u64 x = (u64)v - o + 1;
    const u32 l = 63u - (u32)__builtin_clzll(x);
    *log = l;
    *residual = (u32)(x - (1ull << l));
    return o + l;
}

// Elias-delta codeword of c (elias_delta_uint_coder.py): y = c + 1, n = bit length of y - 1, l = bit length of (n + 1) - 1:
// l zeros, n + 1 in l + 1 bits, the n low bits of y.  At most 43 bits for c < 2^32.
__device__ __forceinline__ u32 lze_elias_delta(u32 c, u64 *val) {
    const u64 y = (u64)c + 1;
    const u32 n = 63u - (u32)__builtin_clzll(y);
    const u32 l = 31u - (u32)__builtin_clz(n + 1);
    *val = ((u64)(n + 1) << n) | (y - (1ull << n));
    return 2 * l + 1 + n;
}

struct LzeSmallTree {
    double prob[2 * LZE_FIELD_K];
    u16 heap[LZE_FIELD_K], parent[2 * LZE_FIELD_K], leaf_sym[LZE_FIELD_K];
};
struct LzeBigTree {
    double prob[2 * LZ_HUFF_MAX_K];
    u16 heap[LZ_HUFF_MAX_K], parent[2 * LZ_HUFF_MAX_K], kids[2 * LZ_HUFF_MAX_K], leaf_sym[LZ_HUFF_MAX_K];
};

// bits [p, p + w) of the input, w <= 32; reads only the bytes that hold them
__device__ __forceinline__ u32 lze_read_bits(const u8 *in, u64 p, u32 w) {
    if (w == 0) return 0;
    const u64 first = p >> 3, last = (p + w - 1) >> 3;
    u64 acc = 0;
    for (u64 i = first; i <= last; ++i) acc = (acc << 8) | in[i];
    const u32 have = (u32)(last - first + 1) * 8;
    return (u32)((acc >> (have - (u32)(p & 7) - w)) & (w == 32 ? 0xFFFFFFFFull : (1ull << w) - 1));
}

// one lane's forward cursor over a section of `left` bits: never loads a byte that holds no bit of the section, and the
// caller never takes more than `left`
struct LzeCursor {
    const u8 *in;
    u64 next_byte, last_byte, buf, left;
    u32 nbuf;

    __device__ __forceinline__ void init(const u8 *in_, u64 p, u64 nbits) {
        in = in_;
        left = nbits;
        buf = 0;
        nbuf = 0;
        next_byte = 1;
        last_byte = 0;
        if (nbits == 0) return;
        next_byte = p >> 3;
        last_byte = (p + nbits - 1) >> 3;
        const u32 skip = (u32)(p & 7);
        buf = (u64)in[next_byte++] << (56 + skip);
        nbuf = 8 - skip;
    }
    __device__ __forceinline__ void refill() {
        while (nbuf <= 56 && next_byte <= last_byte) {
            buf |= (u64)in[next_byte++] << (56 - nbuf);
            nbuf += 8;
        }
    }
    __device__ __forceinline__ u32 get(u32 w) {  // w <= 32, w <= left
        if (w == 0) return 0;
        if (nbuf < w) refill();
        const u32 v = (u32)(buf >> (64 - w));
        buf <<= w;
        nbuf -= w;
        left -= w;
        return v;
    }
};

// ---- the encoders: histograms -> trees -> code tables ----------------------------------------------------------------------
// EVERY one of the workgroup's THREADS threads calls, `tid` its index, with hist[LZE_SYMS] complete behind a barrier.  Four
// threads build the four trees (A = a sequence field's alphabet), then all fill code[] / clen[] of the symbols with a count
// and raise SCL_ST_SIZE in *flags for a codeword above 32 bits.  Ends behind a barrier: the tables and *flags are readable.
template <u32 THREADS>
__device__ __forceinline__ void lze_build_codes(const u32 *hist, u32 A, u32 tid, LzeSmallTree *small /* [3] */, LzeBigTree &big,
                                                u32 *n_leaves /* [4] */, u32 *code, u8 *clen, u32 *flags) {
    if (tid < 4) {
        LzHuffTree t;
        if (tid < 3) {
            t = {small[tid].prob, small[tid].heap, small[tid].parent, nullptr, small[tid].leaf_sym};
        } else {
            t = {big.prob, big.heap, big.parent, nullptr, big.leaf_sym};
        }
        n_leaves[tid] = lz_huffman_build(hist + tid * LZE_FIELD_K, tid < 3 ? A : 256u, t);
    }
    __syncthreads();
    for (u32 f = 0; f < 4; ++f) {
        const u16 *parent = f < 3 ? small[f].parent : big.parent;
        const u16 *leaf_sym = f < 3 ? small[f].leaf_sym : big.leaf_sym;
        for (u32 i = tid; i < n_leaves[f]; i += THREADS) {
            u32 c;
            const u32 len = lz_huffman_leaf_code(parent, i, &c);
            if (len > LZ_HUFF_MAX_CODE_BITS) atomicOr(flags, (u32)SCL_ST_SIZE);
            code[f * LZE_FIELD_K + leaf_sym[i]] = c;
            clen[f * LZE_FIELD_K + leaf_sym[i]] = (u8)(len > 255 ? 255 : len);
        }
    }
    __syncthreads();
}

// ---- the decoders: the counts of a field -----------------------------------------------------------------------------------
// ONE lane: the `counts_size` bits from bit `p` of `in` are Elias-delta codewords until the section is used up, exactly;
// the first K of them go to hist[] (zeroed by the caller; counts past the alphabet are ignored, as the reference does).
// Returns 0 or SCL_ST_STATE.
__device__ __forceinline__ u32 lze_parse_counts(const u8 *in, u64 p, u32 counts_size, u32 K, u32 *hist) {
    LzeCursor cur;
    cur.init(in, p, counts_size);
    u32 j = 0, st = 0;
    u64 total = 0;
    while (cur.left) {
        u32 l = 0;
        bool one = false;
        while (cur.left && l <= 5) {
            if (cur.get(1)) {
                one = true;
                break;
            }
            ++l;
        }
        // no 1 before the end, or n + 1 >= 64: a count of 2^32 or more, or a cut codeword
        if (!one || cur.left < l) {
            st = SCL_ST_STATE;
            break;
        }
        const u32 n = ((1u << l) | cur.get(l)) - 1;
        if (n > 32 || cur.left < n) {
            st = SCL_ST_STATE;
            break;
        }
        const u64 c = ((1ull << n) | cur.get(n)) - 1;
        if (c >> 32) {
            st = SCL_ST_STATE;
            break;
        }
        if (j < K) {
            hist[j] = (u32)c;
            total += c;
        }
        ++j;
    }
    if (st == 0 && (j < K || total == 0)) st = SCL_ST_STATE;
    return st;
}

#endif  // __HIPCC__
