// scl_uint_code.h -- the three prefix codes over unbounded non-negative integers (Golomb, universal, Elias-delta) as ONE
// rule for host and device: the codeword of a value, and one codeword read from 32 left-aligned bits.  The alphabet has no
// end, so there is no (code, len) table: the codeword is computed from the value and a decode step is one count of leading
// bits and a shift.  Codewords (reference golomb_coder.py, universal_uint_coder.py, elias_delta_uint_coder.py):
//   Golomb(M)    q = x / M ones, a zero, then r = x % M in b bits if M is a power of two or r < cutoff, else r + cutoff in
//                b + 1 bits (b = floor(log2 M), cutoff = 2^(b+1) - M)
//   universal    L - 1 ones, a zero, then x in L bits, L = max(1, bit length of x)
//   Elias-delta  y = x + 1, n = bit length of y minus one, l = bit length of (n + 1) minus one: l zeros, n + 1 in l + 1 bits,
//                the n bits of y below its leading one
// A codeword travels in one 32-bit word (PFB_MAX_LEN): universal x < 2^16, Elias-delta x <= 2^24 - 2, Golomb
// x / M + 1 + b (+ 1) <= 32; longer ones are refused (length 0 / PFB_END_STATE), never split.  Used by scl_uint_block.hip;
// DESIGN.md 3.5.2.  The lane-per-stream kernels of scl_uint.hip carry every 32-bit value: their form of the rule (the
// codeword in pieces, one codeword read sequentially) is at the end of this header; DESIGN.md 3.5.3.
#pragma once

#include "scl_bit_block.h"

// the rule as the kernels take it: b, cutoff and recip are derived from M by scl_uint_rule_make, in integer arithmetic
struct SclUintRule {
    u32 kind;    // SCL_UINT_*
    u32 M;       // Golomb's parameter, 1 <= M < 2^31 (1 for the other kinds)
    u32 b;       // floor(log2 M)
    u32 cutoff;  // 2^(b+1) - M; == M: M is a power of two (a Rice code)
    u64 recip;   // ceil(2^64 / M) for an M that is no power of two: x / M = (x * recip) >> 64 for every 32-bit x
};

struct SclUintWord {
    u32 bits;  // right-aligned, nothing above them
    u32 len;   // 0: the codeword is longer than 32 bits
};

static inline SclUintRule scl_uint_rule_make(u32 kind, u32 M) {
    SclUintRule c = {kind, kind == SCL_UINT_GOLOMB ? M : 1u, 0u, 0u, 0ull};
    while ((2u << c.b) <= c.M) ++c.b;  // M < 2^31: 2 << b stays below 2^32
    c.cutoff = (2u << c.b) - c.M;
    if (c.cutoff != c.M) c.recip = ~0ull / c.M + 1;  // M >= 3 divides no power of two: floor((2^64 - 1) / M) + 1 = ceil
    return c;
}

// the public {kind, M} checked and turned into the kernels' rule; `what` names the entry point in the error text
static inline int scl_uint_rule_checked(const char *what, const scl_uint_code *code, SclUintRule *rule) {
    SCL_REQUIRE(code, "%s: null pointer argument", what);
    SCL_REQUIRE(code->kind <= SCL_UINT_ELIAS_DELTA, "%s: unknown code kind %u", what, code->kind);
    SCL_REQUIRE(code->kind != SCL_UINT_GOLOMB || (code->M >= 1 && code->M < (1u << 31)),
                "%s: Golomb parameter M = %u: 1 <= M < 2^31", what, code->M);
    *rule = scl_uint_rule_make(code->kind, code->M);
    return SCL_OK;
}

__host__ __device__ __forceinline__ u32 scl_uint_clz(u32 v) { return v ? (u32)__builtin_clz(v) : 32u; }

// x / M: a shift for a power of two, else the high 64 bits of x * recip (x < 2^32, so two 64-bit products hold them).
// Exact: recip = 2^64 / M + e with 0 < e < 1, so x * recip / 2^64 = x / M + x * e / 2^64, and x * e / 2^64 < 2^-32 < 1 / M
// is too little to reach the next integer from a multiple of 1 / M.
__host__ __device__ __forceinline__ u32 scl_uint_div(const SclUintRule &c, u32 x) {
    if (c.cutoff == c.M) return x >> c.b;
    const u64 hi = (u64)x * (c.recip >> 32), lo = (u64)x * (c.recip & 0xFFFFFFFFull);
    return (u32)((hi + (lo >> 32)) >> 32);
}

__host__ __device__ __forceinline__ SclUintWord scl_uint_codeword(const SclUintRule &c, u32 x) {
    SclUintWord w = {0u, 0u};
    if (c.kind == SCL_UINT_GOLOMB) {
        const u32 q = scl_uint_div(c, x), r = x - q * c.M;
        const bool longer = c.cutoff != c.M && r >= c.cutoff;
        const u32 rb = c.b + (longer ? 1u : 0u);
        if (q > 31u || q + 1u + rb > PFB_MAX_LEN) return w;
        const u64 unary = ((1ull << q) - 1ull) << 1;  // q ones and the zero
        w.bits = (u32)((unary << rb) | (longer ? r + c.cutoff : r));
        w.len = q + 1u + rb;
    } else if (c.kind == SCL_UINT_UNIVERSAL) {
        const u32 L = x ? 32u - scl_uint_clz(x) : 1u;
        if (2u * L > PFB_MAX_LEN) return w;
        w.bits = ((((1u << (L - 1u)) - 1u) << 1) << L) | x;
        w.len = 2u * L;
    } else {
        if (x > (1u << 24) - 2u) return w;
        const u32 y = x + 1u, n = 31u - scl_uint_clz(y), l = 31u - scl_uint_clz(n + 1u);
        w.bits = ((n + 1u) << n) | (y - (1u << n));  // the l zeros in front are the word's own high bits
        w.len = 2u * l + 1u + n;
    }
    return w;
}

// One codeword from the left-aligned `bits`, of which `rem` >= 1 belong to the stream (what lies behind them is not looked
// at).  In the order a sequential reader meets them: the unary part (or Elias-delta's zeros) runs to the end of the stream
// -> PFB_END_TRUNC; what has been read announces more than 32 bits -> PFB_END_STATE; it announces more than `rem` ->
// PFB_END_TRUNC (the cut lies in the length field, the remainder or Golomb's extra bit); else PFB_END_EXIT, `x` in `len` bits.
__host__ __device__ __forceinline__ u32 scl_uint_decode(const SclUintRule &c, u32 bits, u32 rem, u32 &len, u32 &x) {
    if (c.kind == SCL_UINT_ELIAS_DELTA) {
        const u32 l = scl_uint_clz(bits);
        if (l >= rem) return PFB_END_TRUNC;
        if (2u * l + 1u > PFB_MAX_LEN) return PFB_END_STATE;
        if (2u * l + 1u > rem) return PFB_END_TRUNC;
        const u32 n = ((bits << l) >> (31u - l)) - 1u;  // l + 1 bits from the first one on: n + 1 >= 2^l
        const u32 total = 2u * l + 1u + n;
        if (total > PFB_MAX_LEN) return PFB_END_STATE;
        if (total > rem) return PFB_END_TRUNC;
        const u32 low = n ? (bits << (2u * l + 1u)) >> (32u - n) : 0u;
        x = ((1u << n) | low) - 1u;
        len = total;
        return PFB_END_EXIT;
    }
    const u32 q = scl_uint_clz(~bits);  // leading ones
    if (q >= rem) return PFB_END_TRUNC;
    if (c.kind == SCL_UINT_UNIVERSAL) {
        const u32 L = q + 1u;
        if (2u * L > PFB_MAX_LEN) return PFB_END_STATE;
        if (2u * L > rem) return PFB_END_TRUNC;
        x = (bits << L) >> (32u - L);
        len = 2u * L;
        return PFB_END_EXIT;
    }
    u32 need = q + 1u + c.b;
    if (need > PFB_MAX_LEN) return PFB_END_STATE;
    if (need > rem) return PFB_END_TRUNC;
    u32 r = c.b ? (bits << (q + 1u)) >> (32u - c.b) : 0u;  // b > 0: q + 1 <= 31
    if (c.cutoff != c.M && r >= c.cutoff) {
        if (++need > PFB_MAX_LEN) return PFB_END_STATE;
        if (need > rem) return PFB_END_TRUNC;
        r = 2u * r + ((bits >> (32u - need)) & 1u) - c.cutoff;
    }
    x = c.M * q + r;  // below 2^32: q <= 31 - b and M < 2^(b+1)
    len = need;
    return PFB_END_EXIT;
}

// ---- the rule without the 32-bit limit (scl_uint.hip: one lane per stream) ------------------------------
// The codeword of ANY 32-bit x in pieces a sequential writer can put: `run` ones, then two fields of at most 32 bits each
// (a field of 0 bits is empty).
//   Golomb       run = q, f0 = the zero and the remainder: 1 + b (+ 1) <= 32 bits (b <= 30); no second field
//   universal    no run; f0 = L - 1 ones and the zero, L <= 32 bits; f1 = x in L bits
//   Elias-delta  no run; f0 = n + 1 in 2l + 1 <= 11 bits (the l zeros are its high bits); f1 = the low n <= 32 bits of
//                y = x + 1 (y = 2^32 for x = 2^32 - 1: n = 32, f1 = 0, 43 bits in all)
// Golomb's run is as long as x / M; the other two codes stop at 64 bits.
struct SclUintFields {
    u32 run;
    u32 f0, n0;
    u32 f1, n1;
};

__host__ __device__ __forceinline__ u64 scl_uint_fields_len(const SclUintFields &f) { return (u64)f.run + f.n0 + f.n1; }

__host__ __device__ __forceinline__ SclUintFields scl_uint_fields(const SclUintRule &c, u32 x) {
    SclUintFields f = {0u, 0u, 0u, 0u, 0u};
    if (c.kind == SCL_UINT_GOLOMB) {
        const u32 q = scl_uint_div(c, x), r = x - q * c.M;
        const bool longer = c.cutoff != c.M && r >= c.cutoff;
        f.run = q;
        f.f0 = longer ? r + c.cutoff : r;  // below 2^(b+1): the zero in front of it is the field's own top bit
        f.n0 = 1u + c.b + (longer ? 1u : 0u);
    } else if (c.kind == SCL_UINT_UNIVERSAL) {
        const u32 L = x ? 32u - scl_uint_clz(x) : 1u;
        f.f0 = ((1u << (L - 1u)) - 1u) << 1;
        f.n0 = L;
        f.f1 = x;
        f.n1 = L;
    } else {
        const u64 y = (u64)x + 1u;
        const u32 n = (y >> 32) ? 32u : 31u - scl_uint_clz((u32)y), l = 31u - scl_uint_clz(n + 1u);
        f.f0 = n + 1u;
        f.n0 = 2u * l + 1u;
        f.f1 = (u32)(y - (1ull << n));
        f.n1 = n;
    }
    return f;
}

// One codeword read sequentially from a bit source of which `rem` >= 1 bits belong to the stream.  SRC supplies
//   u32 look()      the next 32 bits, left-aligned (what lies behind the stream is not looked at)
//   void skip(n)    consume n <= 32 bits
//   void relief()   every codeword passes one, and at most two words are consumed between two (a ring reader refills there)
// Returns 0 with `x` in `len` bits, or the verdict in the order a sequential reader meets it:
//   Golomb       the ones read inside the stream reach a quotient q with M * q >= 2^32 -> SCL_ST_SIZE (this, not the stream,
//                bounds the loop); the stream ends before the zero -> SCL_ST_TRUNCATED; the b remainder bits or the extra bit
//                of a long remainder are missing -> SCL_ST_TRUNCATED; M * q + r >= 2^32 -> SCL_ST_SIZE
//   universal    the 32nd one inside the stream -> SCL_ST_SIZE; the run reaches the end -> SCL_ST_TRUNCATED; 2L > rem ->
//                SCL_ST_TRUNCATED
//   Elias-delta  the 6th zero inside the stream -> SCL_ST_SIZE; the zeros reach the end, or 2l + 1 > rem -> SCL_ST_TRUNCATED;
//                n > 32 -> SCL_ST_SIZE; 2l + 1 + n > rem -> SCL_ST_TRUNCATED; n = 32 with a low field != 0 -> SCL_ST_SIZE
// After a verdict the source stands somewhere inside the codeword: the caller reads no further.
template <class SRC>
__host__ __device__ __forceinline__ u32 scl_uint_decode_wide(const SclUintRule &c, SRC &src, u32 rem, u32 &len, u32 &x) {
    if (c.kind == SCL_UINT_GOLOMB) {
        const u64 qlim = ((1ull << 32) + c.M - 1u) / c.M;  // the first quotient whose M * q leaves 32 bits
        u64 q = 0;
        u32 left = rem, k;
        for (;;) {  // the ones, up to a word at a time
            const u32 avail = left < 32u ? left : 32u;
            k = scl_uint_clz(~src.look());
            k = k < avail ? k : avail;
            if (q + k >= qlim) return SCL_ST_SIZE;
            q += k;
            left -= k;
            if (k < avail) break;  // the zero is in sight: k < 32 ones and the zero are still in front of the source
            if (left == 0) return SCL_ST_TRUNCATED;
            src.skip(32u);  // k == avail == 32
            src.relief();
        }
        src.skip(k + 1u);
        left -= 1u;
        src.relief();
        if (c.b > left) return SCL_ST_TRUNCATED;
        u32 r = c.b ? src.look() >> (32u - c.b) : 0u;
        src.skip(c.b);
        left -= c.b;
        if (c.cutoff != c.M && r >= c.cutoff) {
            if (left == 0) return SCL_ST_TRUNCATED;
            r = 2u * r + (src.look() >> 31) - c.cutoff;
            src.skip(1u);
            left -= 1u;
        }
        const u64 v = (u64)c.M * q + r;  // q < qlim: M * q is below 2^32, the remainder may carry it over
        if (v >> 32) return SCL_ST_SIZE;
        x = (u32)v;
        len = rem - left;
        return 0u;
    }
    if (c.kind == SCL_UINT_UNIVERSAL) {
        const u32 avail = rem < 32u ? rem : 32u;
        u32 k = scl_uint_clz(~src.look());
        k = k < avail ? k : avail;
        if (k >= 32u) return SCL_ST_SIZE;
        if (k == rem) return SCL_ST_TRUNCATED;
        const u32 L = k + 1u;
        if (2u * L > rem) return SCL_ST_TRUNCATED;
        src.skip(L);
        src.relief();
        x = src.look() >> (32u - L);
        src.skip(L);
        len = 2u * L;
        return 0u;
    }
    const u32 avail = rem < 32u ? rem : 32u;
    const u32 bits = src.look();
    u32 l = scl_uint_clz(bits);
    l = l < avail ? l : avail;
    if (l >= 6u) return SCL_ST_SIZE;
    if (l == rem || 2u * l + 1u > rem) return SCL_ST_TRUNCATED;
    const u32 n = ((bits << l) >> (31u - l)) - 1u;  // l + 1 bits from the first one on: n + 1 >= 2^l
    if (n > 32u) return SCL_ST_SIZE;
    if (2u * l + 1u + n > rem) return SCL_ST_TRUNCATED;
    src.skip(2u * l + 1u);
    src.relief();
    const u32 low = n ? src.look() >> (32u - n) : 0u;
    if (n == 32u && low != 0u) return SCL_ST_SIZE;
    src.skip(n);
    x = n == 32u ? 0xFFFFFFFFu : ((1u << n) | low) - 1u;
    len = 2u * l + 1u + n;
    return 0u;
}
