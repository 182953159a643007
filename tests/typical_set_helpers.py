"""The typical-set coder restated in numpy, for tests/test_typical_set_host.py and tests/test_gpu_typical_set.py: the rule
(which tuples are typical), four named misreadings of it, the code (chunks -> bits, bits -> chunks with the sequential
decoder's verdicts) and the builders of the inputs the GPU tests use.

A tuple t of K^n in itertools.product order has digits x_i = (t // K^(n-1-i)) % K.  It is typical iff
``abs(s / n - entropy) <= eps`` with ``s = nlp[x_0]``, then ``s += nlp[x_i]`` for i = 1..n-1, in float64: numpy's elementwise
float64 addition, division and subtraction are the IEEE operations of the C rule, so the arrays below are bit-exact."""
import numpy as np

from conftest import load_golden

NONE = 0xFFFFFFFF
ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED, ST_STATE = 0x1, 0x2, 0x4, 0x8
TILE, PER_THREAD, SUB, GROUP = 4096, 16, 128, 32768  # PFB_TILE, PFB_PER_THREAD, PFB_SUB, PFB_GROUP of scl_bit_block.h
TABLE_TILE = 4096                                      # TS_TILE of scl_typical.hip

GOLDENS = load_golden("typical_set")
MISREADINGS = ("counts", "scaled", "reversed", "strict")


def digits(K, n, t=None):
    """[n] arrays of the digits of the tuples ``t`` (default: all K^n), position 0 first"""
    t = np.arange(K ** n, dtype=np.int64) if t is None else np.asarray(t, np.int64)
    return [(t // K ** (n - 1 - i)) % K for i in range(n)]


def typical_flags(nlp, n, entropy, eps, reading="rule"):
    """bool [K^n]: the rule, or one of MISREADINGS:
    counts   -- sum_k count_k * nlp_k in place of the sum in sequence order
    scaled   -- abs(s - n * entropy) <= n * eps in place of the division
    reversed -- the sum taken from the last symbol
    strict   -- < in place of <="""
    nlp = np.asarray(nlp, np.float64)
    K = nlp.size
    x = digits(K, n)
    if reading == "counts":
        s = np.zeros(K ** n, np.float64)
        for k in range(K):
            s = s + sum((xi == k).astype(np.int64) for xi in x) * nlp[k]
    else:
        order = x[::-1] if reading == "reversed" else x
        s = nlp[order[0]].copy()
        for xi in order[1:]:
            s = s + nlp[xi]
    if reading == "scaled":
        return np.abs(s - n * np.float64(entropy)) <= n * np.float64(eps)
    d = np.abs(s / n - np.float64(entropy))
    return d < eps if reading == "strict" else d <= eps


def tables_of(flags):
    """-> (rank[N] uint32 with NONE, inv[count] uint32, count)"""
    flags = np.asarray(flags, bool)
    rank = np.where(flags, np.cumsum(flags) - 1, NONE).astype(np.uint32)
    return rank, np.flatnonzero(flags).astype(np.uint32), int(flags.sum())


def ceil_log2(x):
    """the reference's expression"""
    return int(np.ceil(np.log2(x)))


def widths(count, N):
    """-> (bt or None, bo)"""
    return (None if count == 0 else ceil_log2(count)), ceil_log2(N)


def tuples_of(idx, K, n):
    idx = np.asarray(idx, np.int64).reshape(-1, n)
    t = np.zeros(idx.shape[0], np.int64)
    for i in range(n):
        t = t * K + idx[:, i]
    return t


def symbols_of(t, K, n):
    return np.stack(digits(K, n, t), axis=1).reshape(-1) if len(t) else np.zeros(0, np.int64)


def code_of_tuples(t, rank, bt, bo):
    """-> (values, lengths) of the codewords of the tuples ``t``"""
    r = rank[t].astype(np.int64)
    typical = r != NONE
    return (np.where(typical, r, (1 << bo) | t), np.where(typical, 1 + (bt or 0), 1 + bo))


def encode_bits(idx, K, n, rank, bt, bo):
    """the stream of a block of symbol indices -> (bits uint8 0/1, the bit behind every chunk)"""
    val, ln = code_of_tuples(tuples_of(idx, K, n), rank, bt, bo)
    shifts = ln[:, None] - 1 - np.arange(1 + bo)[None, :]
    bits = ((val[:, None] >> np.maximum(shifts, 0)) & 1).astype(np.uint8)
    return bits[shifts >= 0], np.cumsum(ln)


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8))


def decode_stream(bits, nbits, K, n, inv, bt, bo, cap_symbols):
    """the sequential decoder -> (symbol indices, consumed, status): the capacity is looked at before every codeword; flag 0:
    no typical set STATE, a cut codeword TRUNCATED, an index >= count STATE; flag 1: TRUNCATED, an index >= K^n STATE"""
    N, count = K ** n, len(inv)
    out, pos, cap = [], 0, cap_symbols // n
    status = 0
    while pos < nbits:
        if len(out) == cap:
            status = ST_CAPACITY
            break
        other = int(bits[pos])
        w = bo if other else bt
        if w is None:
            status = ST_STATE
            break
        if pos + 1 + w > nbits:
            status = ST_TRUNCATED
            break
        index = int("0" + "".join(map(str, np.asarray(bits[pos + 1:pos + 1 + w]).tolist())), 2)
        if index >= (N if other else count):
            status = ST_STATE
            break
        out.append(index if other else int(inv[index]))
        pos += 1 + w
    return symbols_of(np.array(out, np.int64), K, n), pos, status


# ---- the goldens -----------------------------------------------------------------------------------------------------------
def golden_flags(case):
    return np.unpackbits(case.arr("bitmap"))[: case.K ** case.n].astype(bool)


def golden_model(case):
    """-> (nlp, n, entropy, eps) as the C ABI takes them"""
    return case.arr("nlp"), case.n, float(case.arr("entropy")[0]), float(case.eps)


def golden_dist(case):
    """the golden's distribution as the dict a ProbabilityDist takes"""
    names = [chr(ord("A") + i) for i in range(case.K)] if case.symbols == "str" else list(range(case.K))
    # the reference's {"A": 1} holds the int 1
    probs = [1 if case.group == "a1" else float(p) for p in case.arr("probs")]
    return dict(zip(names, probs))


# ---- the models of the GPU tests: (nlp, n, entropy, eps), handed to the C ABI as they are -----------------------------------
# nlp = [0, 1]: s counts the ones of a binary chunk, so a window on s / n picks whole weight classes
ONE_BIT = ([0.0], 1, 0.0, 0.0)          # {A: 1}, n = 1: one typical tuple, bt = bo = 0, a chunk is the bit 0
ALL_ATYPICAL = ([0.0], 1, 0.0, -1.0)    # the same with an empty typical set: a chunk is the bit 1
EQUAL_LENGTHS = ([0.0, 1.0], 4, 0.5, 0.25)       # weight 1..3 of 4: 14 of 16 typical, lengths 5 and 5
SHARED_GCD = ([0.0, 1.0], 7, 1.0 / 7, 0.01)      # weight 1 of 7: 7 of 128 typical, lengths 4 and 8
COPRIME = ([0.0, 1.0], 6, 1.0 / 6, 0.01)         # weight 1 of 6: 6 of 64 typical, lengths 4 and 7
NOT_POWER_OF_TWO = ([0.0, 1.0, 2.0], 3, 1.0, 0.1)  # K = 3, n = 3: N = 27 of 32 five-bit indices; s = 3: 7 typical of 8


def host_tables(model):
    """the restated rule's tables of one of the models above -> (K, n, rank, inv, bt, bo)"""
    nlp, n, entropy, eps = model
    rank, inv, count = tables_of(typical_flags(nlp, n, entropy, eps))
    bt, bo = widths(count, len(nlp) ** n)
    return len(nlp), n, rank, inv, bt, bo


def mixed_block(model, n_chunks, seed=0):
    """symbol indices of ``n_chunks`` chunks, about half of them typical (where the set has members), in random order"""
    K, n, rank, inv, _, _ = host_tables(model)
    rng = np.random.default_rng(seed + n_chunks)
    t = rng.integers(0, K ** n, n_chunks)
    if len(inv) and len(inv) < K ** n:
        others = np.flatnonzero(rank == NONE)
        pick = rng.random(n_chunks) < 0.5
        t = np.where(pick, rng.choice(inv.astype(np.int64), n_chunks), rng.choice(others, n_chunks))
    return symbols_of(t, K, n)
