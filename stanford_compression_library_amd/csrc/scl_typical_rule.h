// scl_typical_rule.h -- which tuples of X^n are typical: the rule of the reference's is_typical (typical_set_coder.py:29-42),
// ONCE, for the host (scl_typical_table_host) and the device (the table kernels of scl_typical.hip).
//
// The reference adds neg_log_probability(x_i) in sequence order in float64, divides by n, subtracts the entropy and compares
// the absolute value with eps.  Membership depends on the ORDER of the symbols, not only on their counts, and on every
// rounding on the way: so the same operations, in the same order, and nothing else -- additions, one
// division, one subtraction, one comparison; no multiplication, hence nothing to contract, and the pragma says so anyway.
// Built with the Makefile's flags as they are (no fast-math).  Internal to csrc/.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SCL_TS_HD __host__ __device__
#else
#define SCL_TS_HD
#endif

// K^(n-1): the weight of position 0 of a tuple (the caller has checked K^n <= 2^24)
SCL_TS_HD static inline uint32_t scl_typical_top(uint32_t K, uint32_t n) {
    uint32_t p = 1;
    if (K > 1)
        for (uint32_t i = 1; i < n; ++i) p *= K;
    return p;
}

// Tuple t in itertools.product order has digits x_i = (t / K^(n-1-i)) mod K, position 0 varying slowest; top = K^(n-1).
SCL_TS_HD static inline bool scl_typical_rule(const double *nlp, uint32_t K, uint32_t n, uint32_t top, double entropy, double eps,
                                              uint32_t t) {
#pragma clang fp contract(off)
    uint32_t p = top;
    uint32_t x = t / p;
    t -= x * p;
    double s = nlp[x];
    for (uint32_t i = 1; i < n; ++i) {
        p = K > 1 ? p / K : 1u;
        x = t / p;
        t -= x * p;
        s += nlp[x];
    }
    return fabs(s / (double)n - entropy) <= eps;
}

// ceil(log2 x) in integers for x >= 1 (the reference: int(np.ceil(np.log2(x)))); 0xFFFFFFFF for x = 0: no such width
SCL_TS_HD static inline uint32_t scl_typical_index_bits(uint64_t x) {
    if (x == 0) return 0xFFFFFFFFu;
    uint32_t w = 0;
    for (uint64_t v = x - 1; v; v >>= 1) ++w;
    return w;
}
