"""The three integer codes (Golomb, universal, Elias-delta) restated in plain Python, and the fixtures of their tests.

``codeword`` is the rule on unbounded Python integers; ``decode_stream`` is the sequential decoder with the device's limits:
it reports ``(values, consumed, status)`` for any stream, damaged ones included, as the block kernels must.  In the order a
reader meets them: the unary part (Elias-delta: the zeros) runs to the end of the stream -> ST_TRUNCATED; what has been read
announces a codeword above 32 bits -> ST_SIZE; it announces more bits than are left -> ST_TRUNCATED.
"""
import numpy as np

from conftest import load_golden

ST_CAPACITY, ST_TRUNCATED, ST_SIZE = 0x1, 0x4, 0x20
KIND_ID = {"golomb": 0, "universal": 1, "elias_delta": 2}
GOLOMB_MS = (1, 2, 3, 4, 10, 64, 1000)
CODES = [("golomb", M) for M in GOLOMB_MS] + [("universal", None), ("elias_delta", None)]
CODE_IDS = [f"{k}{M or ''}" for k, M in CODES]
MAX_LEN = 32


def golomb_params(M):
    b = M.bit_length() - 1
    return b, (2 << b) - M


def codeword(kind, M, x):
    """-> (bits as an integer, length) of the codeword of x >= 0, of any length"""
    if kind == "golomb":
        b, cutoff = golomb_params(M)
        q, r = divmod(x, M)
        head = ((1 << q) - 1) << 1
        if cutoff == M or r < cutoff:
            return (head << b) | r, q + 1 + b
        return (head << (b + 1)) | (r + cutoff), q + 2 + b
    if kind == "universal":
        L = max(1, x.bit_length())
        return ((((1 << (L - 1)) - 1) << 1) << L) | x, 2 * L
    y = x + 1
    n = y.bit_length() - 1
    l = (n + 1).bit_length() - 1
    return ((n + 1) << n) | (y - (1 << n)), 2 * l + 1 + n


def codeword_length(kind, M, x):
    """the length of the codeword of x alone (a Golomb codeword of a large x is mostly ones: no need to write them)"""
    if kind == "golomb":
        b, cutoff = golomb_params(M)
        q, r = divmod(x, M)
        return q + 1 + b + (cutoff != M and r >= cutoff)
    return codeword(kind, M, x)[1]


def encode_bits(kind, M, values):
    """-> (bits as a uint8 0/1 array, ends: the bit behind every codeword)"""
    text, ends = [], []
    total = 0
    for x in values:
        v, n = codeword(kind, M, int(x))
        text.append(format(v, f"0{n}b"))
        total += n
        ends.append(total)
    return np.frombuffer("".join(text).encode(), np.uint8) - ord("0"), np.array(ends, np.int64)


def decode_one(kind, M, text, pos, total):
    """one codeword from bit ``pos`` of the 0/1 string ``text``, of which ``total`` bits are the stream
    -> (0, length, value) or (ST_TRUNCATED / ST_SIZE, 0, 0)"""
    rem = total - pos
    w = text[pos: pos + min(rem, MAX_LEN)]
    lead = "0" if kind == "elias_delta" else "1"
    run = len(w) - len(w.lstrip(lead))
    if run == len(w):  # nothing but the run in sight
        return (ST_TRUNCATED if rem <= MAX_LEN else ST_SIZE), 0, 0

    def check(need):
        return ST_SIZE if need > MAX_LEN else ST_TRUNCATED if need > rem else 0

    if kind == "elias_delta":
        st = check(2 * run + 1)
        if st:
            return st, 0, 0
        n = int(w[run: 2 * run + 1], 2) - 1
        st = check(2 * run + 1 + n)
        if st:
            return st, 0, 0
        low = w[2 * run + 1: 2 * run + 1 + n]
        return 0, 2 * run + 1 + n, (1 << n) + (int(low, 2) if low else 0) - 1
    if kind == "universal":
        L = run + 1
        st = check(2 * L)
        if st:
            return st, 0, 0
        return 0, 2 * L, int(w[L: 2 * L], 2)
    b, cutoff = golomb_params(M)
    need = run + 1 + b
    st = check(need)
    if st:
        return st, 0, 0
    r = int(w[run + 1: need], 2) if b else 0
    if cutoff != M and r >= cutoff:
        need += 1
        st = check(need)
        if st:
            return st, 0, 0
        r = 2 * r + int(w[need - 1]) - cutoff
    return 0, need, M * run + r


def decode_stream(kind, M, bits, nbits=None, cap=None):
    """the sequential decode of the first ``nbits`` of the 0/1 array ``bits`` into at most ``cap`` values
    -> (values, consumed, status): the whole codewords in front of the fault, the bits they take, what ended the stream"""
    text = (np.asarray(bits, np.uint8) + ord("0")).astype(np.uint8).tobytes().decode()
    total = len(text) if nbits is None else int(nbits)
    out, pos, status = [], 0, 0
    while pos < total:
        if cap is not None and len(out) == cap:
            status = ST_CAPACITY
            break
        status, n, x = decode_one(kind, M, text, pos, total)
        if status:
            break
        out.append(x)
        pos += n
    return np.array(out, np.uint32), pos, status


def length_boundaries(kind, M):
    """every value whose codeword is the shortest or the longest of its length (Golomb: of its quotient's short and long
    remainders), up to 32 bits, each with its two neighbours (that stay below 2^32)"""
    if kind == "universal":
        core = {v for L in range(1, 17) for v in ((1 << (L - 1)) if L > 1 else 0, (1 << L) - 1)}
    elif kind == "elias_delta":
        core = {v for n in range(24) for v in ((1 << n) - 1, (1 << (n + 1)) - 2)}
    else:
        b, cutoff = golomb_params(M)
        core = {q * M + r for q in range(33 - b) for r in (0, cutoff - 1, cutoff, M - 1) if 0 <= r < M}
    return sorted({v + d for v in core for d in (-1, 0, 1) if 0 <= v + d < (1 << 32)})


def pack(bits):
    """0/1 array -> packed bytes, MSB first"""
    return np.packbits(np.asarray(bits, np.uint8))


def geometric(n, mean=8.0, seed=5):
    """n values from a geometric source on 0, 1, 2, ... with the given mean"""
    return (np.random.default_rng(seed).geometric(1.0 / (mean + 1.0), n) - 1).astype(np.uint32)


GOLDENS = load_golden("uint_codes")
DEVICE_GOLDENS = [c for c in GOLDENS if c.device]


def golden_code(case):
    return case.kind, (case.M if case.kind == "golomb" else None)
