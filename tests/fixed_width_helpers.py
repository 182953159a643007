"""The fixed-width stream restated in numpy, for tests/test_fixed_shannon_host.py and tests/test_gpu_fixed_width.py: index i
of a stream of width w is the w stream bits [i * w, (i + 1) * w), most significant first; stream bit b is bit 7 - b % 8 of byte
b / 8 (``numpy.packbits``); the unused bits of the last byte are 0."""
import numpy as np


def pack_bits(idx, width):
    """indices -> the stream as a uint8 0/1 array of ``len(idx) * width`` bits"""
    idx = np.asarray(idx, np.uint64)
    shifts = np.arange(width - 1, -1, -1, dtype=np.uint64)
    return ((idx[:, None] >> shifts) & np.uint64(1)).astype(np.uint8).reshape(-1)


def pack(idx, width):
    """indices -> (packed stream bytes, nbits)"""
    bits = pack_bits(idx, width)
    return np.packbits(bits), int(bits.size)


def unpack(packed, bit_offset, n, width):
    """``n`` indices from bit ``bit_offset`` of the packed bytes"""
    bits = np.unpackbits(np.asarray(packed, np.uint8))[bit_offset: bit_offset + n * width]
    assert bits.size == n * width
    weights = np.uint64(1) << np.arange(width - 1, -1, -1, dtype=np.uint64)
    return (bits.reshape(n, width).astype(np.uint64) * weights).sum(axis=1).astype(np.uint64)


def embed(stream_bits, bit_offset, total_bytes, rng):
    """random bytes with ``stream_bits`` (0/1 array) laid over them from bit ``bit_offset``"""
    bits = np.unpackbits(rng.integers(0, 256, total_bytes, dtype=np.uint8))
    bits[bit_offset: bit_offset + stream_bits.size] = stream_bits
    return np.packbits(bits)


def golden_symbols(case, name="data"):
    """a golden's block or alphabet as the Python symbols the reference coded"""
    values = case.arr(name).tolist()
    return [chr(v) for v in values] if case.symbols == "str" else values
