"""The batched integer coders (csrc/scl_uint.hip) restated in plain Python, and the fixtures of their tests.

``uint_code_helpers.codeword`` already works on unbounded integers; what is restated here is the sequential DECODE rule of
the lane-per-stream kernels, which carry every uint32 value: ``decode_one_wide`` reads one codeword from a 0/1 string bit by
bit and gives the verdicts in the order a sequential reader meets them, ``decode_stream_wide`` reports
``(values, consumed, status)`` for any stream, damaged ones included.
"""
import numpy as np

from conftest import load_golden
from uint_code_helpers import (CODES, GOLDENS, ST_CAPACITY, ST_SIZE, ST_TRUNCATED, codeword, codeword_length,  # noqa: F401
                               encode_bits, golden_code, golomb_params)

TOP = (1 << 32) - 1
WIDE_GOLDENS = load_golden("uint_wide")
# every golden whose values the batch kernels carry: the old ones below 2^32 (past_limit included) and all new ones
BATCH_GOLDENS = [c for c in GOLDENS if c.n == 0 or int(c.arr("values").max()) <= TOP] + WIDE_GOLDENS
# Golomb parameters at the edges of what the entry points take (no golden: the reference's float logarithm, and its speed)
EDGE_MS = (1, 2, 3, 1 << 30, (1 << 30) + 1, (1 << 31) - 1)


def decode_one_wide(kind, M, text, pos, total):
    """one codeword from bit ``pos`` of the 0/1 string ``text``, of which ``total`` bits are the stream
    -> (0, length, value) or (ST_TRUNCATED / ST_SIZE, 0, 0)"""
    at = pos
    if kind == "golomb":
        b, cutoff = golomb_params(M)
        q = 0
        while True:  # the ones, one at a time
            if at == total:
                return ST_TRUNCATED, 0, 0
            if text[at] == "0":
                break
            q += 1
            at += 1
            if M * q >= 1 << 32:
                return ST_SIZE, 0, 0
        at += 1
        if at + b > total:
            return ST_TRUNCATED, 0, 0
        r = int(text[at: at + b], 2) if b else 0
        at += b
        if cutoff != M and r >= cutoff:
            if at == total:
                return ST_TRUNCATED, 0, 0
            r = 2 * r + int(text[at]) - cutoff
            at += 1
        x = M * q + r
        return (ST_SIZE, 0, 0) if x > TOP else (0, at - pos, x)
    rem = total - pos
    if kind == "universal":
        ones = 0
        while True:
            if at == total:
                return ST_TRUNCATED, 0, 0
            if text[at] == "0":
                break
            ones += 1
            at += 1
            if ones == 32:
                return ST_SIZE, 0, 0
        L = ones + 1
        if 2 * L > rem:
            return ST_TRUNCATED, 0, 0
        return 0, 2 * L, int(text[pos + L: pos + 2 * L], 2)
    zeros = 0
    while True:
        if at == total:
            return ST_TRUNCATED, 0, 0
        if text[at] == "1":
            break
        zeros += 1
        at += 1
        if zeros == 6:
            return ST_SIZE, 0, 0
    if 2 * zeros + 1 > rem:
        return ST_TRUNCATED, 0, 0
    n = int(text[at: at + zeros + 1], 2) - 1
    if n > 32:
        return ST_SIZE, 0, 0
    if 2 * zeros + 1 + n > rem:
        return ST_TRUNCATED, 0, 0
    low = text[pos + 2 * zeros + 1: pos + 2 * zeros + 1 + n]
    y = (1 << n) + (int(low, 2) if low else 0)
    return (ST_SIZE, 0, 0) if y - 1 > TOP else (0, 2 * zeros + 1 + n, y - 1)


def as_text(bits):
    return (np.asarray(bits, np.uint8) + ord("0")).astype(np.uint8).tobytes().decode()


def decode_stream_wide(kind, M, bits, nbits=None, cap=None):
    """the sequential decode of the first ``nbits`` of the 0/1 array ``bits`` into at most ``cap`` values
    -> (values, consumed, status): the whole codewords in front of the fault, the bits they take, what ended the stream"""
    text = as_text(bits)
    total = len(text) if nbits is None else int(nbits)
    out, pos, status = [], 0, 0
    while pos < total:
        if cap is not None and len(out) == cap:
            status = ST_CAPACITY
            break
        status, n, x = decode_one_wide(kind, M, text, pos, total)
        if status:
            break
        out.append(x)
        pos += n
    return np.array(out, np.uint32), pos, status


def stream_bits(kind, M, values):
    """the 0/1 array of the values' codewords back to back (a long Golomb run is written as a run, not through an integer)"""
    parts = []
    for x in values:
        x = int(x)
        if kind == "golomb":
            q = x // M
            v, n = codeword(kind, M, x - q * M)  # the codeword of the remainder alone: quotient 0
            parts += [np.ones(q, np.uint8), np.frombuffer(format(v, f"0{n}b").encode(), np.uint8) - ord("0")]
        else:
            v, n = codeword(kind, M, x)
            parts.append(np.frombuffer(format(v, f"0{n}b").encode(), np.uint8) - ord("0"))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def golden_bits(case):
    """the reference's bits of a golden case as a 0/1 array"""
    return np.unpackbits(case.arr("out"))[: case.nbits]
