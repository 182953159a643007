"""Yardstick of the arithmetic coder's rare renormalisation paths (tests/test_aec_rare_reference.py on the CPU,
tests/test_gpu_aec_rare_paths.py on the GPU): a literal restatement of the reference's encoder loops for PRECISION = 32
(scl/compressors/arithmetic_coding.py:80-161) with the three model kinds, in plain Python integers, and the inputs that
drive the tuned kernels (csrc/scl_aec_{static,fast,split,iid,sparse,wide}.hip) into the branches few symbols take:

  * `k + pending > 32`: the closed-form field of a symbol (b0, `pending` copies of its inverse, k - 1 more bits) no
    longer fits one put, the kernels fall back to the literal loops.  A run of E3 steps needs a symbol whose interval is
    symmetric about 1/2 (rounding drift ends the run at about 30 pending); a rare symbol placed at the peak then takes
    k = 4..6 E1/E2 steps.
  * the strict-comparison corners (quirk Q1) with low != 0 and high != 2^32: `high < HALF`, `low > HALF`,
    `low > QTR and high < 3 QTR` differ from the closed form (k = clz(low ^ (high - 1)), m = leading (1,0) bit pairs
    below) when low or high sits on a power-of-two boundary inside the shifted-out prefix.

Never the code under test: test_aec_rare_reference.py pins `encode` to the CPU oracle (scl_oracle.aec_encode, itself
pinned to the reference's goldens) bit for bit.
"""
from collections import namedtuple

import numpy as np

FIXED, IID, ORDERK = 0, 1, 2  # scl_oracle.MODEL_* / the C ABI's SCL_MODEL_*
FULL, HALF, QTR = 1 << 32, 1 << 31, 1 << 30
MAX_TOTAL = 1 << 30  # the models' rescale threshold: never reached by the short chunks coded here

# bits: the stream (header included) as a uint8 array of 0/1
# max_k_pending: the largest (E1/E2 steps of a symbol) + (pending count that symbol met), over symbols with >= 1 such step
# long_fields: symbols with k + pending > 32 on which the closed form agrees with the loops (the fallback alone sends them
#              through the literal loops)
# corners: symbols on which the closed form disagrees with the loops while low != 0 and high != 2^32
Coded = namedtuple("Coded", "bits max_k_pending long_fields corners")


class _Model:
    """FixedFreqModel / AdaptiveIIDFreqModel / AdaptiveOrderKFreqModel (probability_models.py:57-160) without the
    rescale rule: (c, c + f, T) of a symbol, then update_model"""

    def __init__(self, kind, K, k=0, f_init=None):
        self.kind, self.K, self.k = kind, K, k
        self.ctx = 0
        if kind == ORDERK:
            self.rows = {}  # context index -> counts (all ones until touched)
        else:
            self.counts = [int(f) for f in (f_init if f_init is not None else [1] * K)]
            assert len(self.counts) == K and min(self.counts) >= 1

    def _row(self):
        if self.kind != ORDERK:
            return self.counts
        return self.rows.setdefault(self.ctx, [1] * self.K)

    def lookup_and_update(self, s):
        row = self._row()
        c, f, T = sum(row[:s]), row[s], sum(row)
        assert T < MAX_TOTAL
        if self.kind != FIXED:
            row[s] += 1
        if self.kind == ORDERK and self.k:
            self.ctx = (self.ctx * self.K + s) % (self.K ** self.k)  # past_k[1:] + [s]
        return c, c + f, T


def _closed_form(low, high):
    """(k, m, low', high') of the kernels' closed form (csrc/scl_aec_math.h) on u32 low and hm = high - 1"""
    hm = high - 1
    k = 32 - (low ^ hm).bit_length()
    z = (((low & ~hm) << k) << 1) & 0xFFFFFFFF
    m = 32 - ((~z) & 0xFFFFFFFF).bit_length()
    kt = k + m
    nlow = (low << kt) & 0x7FFFFFFF
    nhm = ((hm << kt) | ((1 << kt) - 1) | HALF) & 0xFFFFFFFF
    return k, m, nlow, nhm + 1


def encode(symbols, kind, K, k=0, f_init=None, size_bits=32):
    model = _Model(kind, K, k, f_init)
    n = len(symbols)
    bits = [(n >> (size_bits - 1 - i)) & 1 for i in range(size_bits)]
    low, high, pending = 0, FULL, 0
    max_kp = long_fields = corners = 0
    for s in symbols:
        c, d, T = model.lookup_and_update(int(s))
        rng = high - low
        low, high = low + (rng * c) // T, low + (rng * d) // T
        low0, high0, pending0 = low, high, pending
        ksteps = msteps = 0
        while high < HALF or low > HALF:  # strict comparisons (quirk Q1)
            if high < HALF:
                bits.append(0)
                bits.extend([1] * pending)
                low, high = low << 1, high << 1
            else:
                bits.append(1)
                bits.extend([0] * pending)
                low, high = (low - HALF) << 1, (high - HALF) << 1
            pending = 0
            ksteps += 1
        while low > QTR and high < 3 * QTR:
            pending += 1
            msteps += 1
            low, high = (low - QTR) << 1, (high - QTR) << 1
        if ksteps:
            max_kp = max(max_kp, ksteps + pending0)
        agrees = _closed_form(low0, high0) == (ksteps, msteps, low, high)
        if agrees and ksteps + pending0 > 32:
            long_fields += 1
        if not agrees and low0 != 0 and high0 != FULL:
            corners += 1
    pending += 1
    bits.append(0 if low <= QTR else 1)
    bits.extend([1 if low <= QTR else 0] * pending)
    return Coded(np.array(bits, dtype=np.uint8), max_kp, long_fields, corners)


# ---- the inputs ----------------------------------------------------------------------------------------------------
# name -> model (the arguments of `encode` and of scl_oracle.aec_encode), the chunk's first symbols, and the largest
# k + pending they reach (found on the CPU with `encode`; test_aec_rare_reference.py asserts it).  The first symbols are a
# run of the alphabet's middle symbol -- its interval is symmetric about 1/2, every step of the run is an E3 step -- and
# then a rare symbol at the peak of the pending count.
F7 = (1, 1, 30, 1, 30, 1, 1)
RareCase = namedtuple("RareCase", "kind K k f_init prefix max_k_pending")
CASES = {
    "static": RareCase(FIXED, 7, 0, F7, (3,) * 5 + (0,), 35),
    "fast_iid": RareCase(IID, 7, 0, F7, (3,) * 7 + (0,), 36),
    "fast_order1": RareCase(ORDERK, 15, 1, None, (7,) * 16 + (0,), 34),
    "iid": RareCase(IID, 255, 0, None, (127,) * 4 + (0,), 34),
    "sparse": RareCase(ORDERK, 255, 1, None, (127,) * 4 + (126,), 35),
    # order-1 on 39 symbols: scl_aec_sparse.hip as shipped, scl_aec_wide.hip under SCL_AEC_WIDE=dense
    "order1_k39": RareCase(ORDERK, 39, 1, None, (19,) * 8 + (0,), 35),
}
N_CHUNKS, CHUNK_LEN = 130, 64  # two full waves and a partial one
# Random symbols do not reach a strict-comparison corner once low is nonzero (it takes low or high on a power-of-two
# boundary: about one symbol in 2^23).  A run of symbol 0 does: c = 0 leaves low where it is, every renormalisation
# shifts it further left, and when its last set bit arrives at the top (low == HALF, high above it) the strict `low > HALF`
# stops where the closed form sees one more common leading bit -- on that symbol and on every 0 after it.  One chunk of
# each wave carries such a run behind its prefix.
CORNER_CHUNKS, CORNER_RUN = (3, 70, 128), 16


def oracle_args(case):
    kw = dict(model_kind=case.kind, K=case.K, k=case.k)
    if case.f_init is not None:
        kw["f_init"] = np.array(case.f_init)
    return kw


def batch(name):
    """(symbols uint8 [N_CHUNKS, CHUNK_LEN], lens int32 [N_CHUNKS]) of one case: every chunk starts with the case's
    prefix, uniformly random symbols of the alphabet follow.  Lengths: the prefix alone (its rare symbol is the chunk's
    last: the decoder leaves before the renormalisation), prefix + 1 (the decoder renormalises it too), CHUNK_LEN, and
    random ones in between; the last chunk -- in the partial wave -- is again the prefix alone.  The CORNER_CHUNKS are
    full length with CORNER_RUN times symbol 0 behind the prefix."""
    case = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    sym = rng.integers(0, case.K, (N_CHUNKS, CHUNK_LEN)).astype(np.uint8)
    p = len(case.prefix)
    sym[:, :p] = case.prefix
    lens = rng.integers(p, CHUNK_LEN + 1, N_CHUNKS).astype(np.int32)
    lens[:3] = [p, p + 1, CHUNK_LEN]
    lens[-1] = p
    for c in CORNER_CHUNKS:
        sym[c, p:p + CORNER_RUN] = 0
        lens[c] = CHUNK_LEN
    return sym, lens
