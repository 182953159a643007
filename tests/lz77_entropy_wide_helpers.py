"""Shared by the tests of LZ77's wide entropy stage (csrc/scl_lz77_entropy_wide.hip): one stream through encode_wide /
decode_wide between guard bands, the same stream through the one-wave batch calls (the yardstick), the synthetic streams of
the tile and workgroup edges, the damaged inputs, and the hand-made literal field whose decoder never falls into step.

Host code only up to the functions that take ``torch``; tests/test_lz77_entropy_wide_host.py checks the fixtures."""
import numpy as np

from lz77_entropy_helpers import FILL, FILL32, U32_MAX, edge_values, guarded, guards_intact, header_positions

TILE = 4096            # values per encoder tile and per residual tile
GROUP_BITS = 256 * 128  # bits per decoder workgroup


# ---- streams ---------------------------------------------------------------------------------------------------------------
def edge_stream(n_seq, n_lit, offset, seed, lit_hi=128):
    """values from edge_values (every bin, values below and at the offset); the top value 2^32 - 1 has no bin under offset 0"""
    rng = np.random.default_rng(seed)
    pool = edge_values(U32_MAX - 1 if offset == 0 else U32_MAX)
    return rng.choice(pool, size=(n_seq, 3)).astype(np.int64), rng.integers(0, lit_hi, n_lit).astype(np.uint8)


N_SEQ_EDGES = (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
N_LIT_EDGES = (0, 1, TILE - 1, TILE, TILE + 1, 40000)


def grid_cases():
    """[(name, stream, offset)]: the n_seq x n_lit x offset grid thinned to a diagonal walk (every n_seq, every n_lit and
    every offset occurs, each n_seq with two n_lit), then the special fields"""
    out = []
    for i, n_seq in enumerate(N_SEQ_EDGES):
        for d in (0, 3):
            n_lit = N_LIT_EDGES[(i + d) % len(N_LIT_EDGES)]
            offset = (0, 16, 32)[(i + d // 3) % 3]
            out.append((f"seq{n_seq}-lit{n_lit}-o{offset}", edge_stream(n_seq, n_lit, offset, 100 + len(out)), offset))
    rng = np.random.default_rng(7)
    # one distinct value per field and one distinct literal: the one-symbol code "0", sections of a few bits that share
    # their output words with the headers around them
    out.append(("one-symbol-2", (np.tile(np.array([[3, 5, 9]], np.int64), (2, 1)), np.full(1, 7, np.uint8)), 16))
    out.append(("one-symbol-4097", (np.tile(np.array([[3, 16, 16 + (1 << 20)]], np.int64), (TILE + 1, 1)),
                                    np.full(TILE + 1, 200, np.uint8)), 16))
    # every value below the offset: all residual widths 0
    out.append(("widths-0", (rng.integers(0, 16, (TILE + 1, 3)).astype(np.int64), rng.integers(0, 256, 300).astype(np.uint8)), 16))
    # every value at least offset + 2^31 - 1: all residual widths 31
    wide = 16 + (1 << 31) - 1 + rng.integers(0, U32_MAX - (16 + (1 << 31) - 1) + 1, (TILE + 1, 3))
    out.append(("widths-31", (wide.astype(np.int64), rng.integers(0, 256, 10).astype(np.uint8)), 16))
    # literals at about 7 bits: inside one decoder workgroup, just over one, nine
    for n_lit in (4000, 5000, 40000):
        out.append((f"lit{n_lit}", edge_stream(70, n_lit, 16, 300 + n_lit), 16))
    return out


# ---- the code that never falls into step -------------------------------------------------------------------------------------
NEVER_SYMBOLS, NEVER_COUNTS, NEVER_PAIRS = (10, 77, 130, 255), (3, 2, 1, 1), 50000


def never_counts():
    counts = np.zeros(256, np.uint64)
    counts[list(NEVER_SYMBOLS)] = NEVER_COUNTS
    return counts


def elias_delta_bits(c):
    """the Elias-delta codeword of the count c as the reference writes it"""
    y = int(c) + 1
    n = y.bit_length() - 1
    l = (n + 1).bit_length() - 1
    text = "0" * l + format(n + 1, f"0{l + 1}b") + (format(y - (1 << n), f"0{n}b") if n else "")
    return [int(ch) for ch in text]


def never_in_step_stream(codes, lengths, pairs=NEVER_PAIRS):
    """A block built by hand: three empty sequence fields, then a literal field whose counts are ``never_counts()`` and whose
    values are the 1-bit codeword followed by the codeword "11", ``pairs`` times -- "011011011...".  A decoder that starts at
    a bit = 2 mod 3 reads "101" for ever and never meets a true codeword boundary, so a decoder workgroup whose first bit is
    one needs the exit of the workgroup on its left.  (codes, lengths): ``huffman_from_counts(never_counts())``.
    -> (0/1 bit array, the literals it decodes to)"""
    word = {format(int(codes[s]), f"0{int(lengths[s])}b"): s for s in NEVER_SYMBOLS}
    one, two = word["0"], word["11"]
    counts_bits = [b for c in never_counts().tolist() for b in elias_delta_bits(c)]
    head = lambda v: [(v >> (31 - i)) & 1 for i in range(32)]  # noqa: E731
    bits = [0] * 96 + head(len(counts_bits)) + counts_bits + head(3 * pairs) + [0, 1, 1] * pairs
    return np.array(bits, np.uint8), np.tile(np.array([one, two], np.uint8), pairs)


# ---- damaged inputs ----------------------------------------------------------------------------------------------------------
def damaged_inputs(stream, bits, offset=16, flips=48, seed=12):
    """-> [(name, 0/1 bit array, bits fed)]: truncations at every header and inside every section, every size header replaced
    by 0, 1, 2^32 - 1 and its value -+ 1, single-bit flips spread over counts, codewords and residuals"""
    heads = header_positions(stream, bits, offset)
    assert len(heads) == 8
    out = []
    cuts = {0, 1, 31, len(bits) - 1}
    for a, b in zip(heads, heads[1:] + [len(bits)]):
        cuts |= {a, a + 31, a + 32, a + 33, (a + 32 + b) // 2, b - 1}
    for cut in sorted(c for c in cuts if 0 <= c < len(bits)):
        out.append((f"cut{cut}", bits, cut))
    for at in heads:
        true = int("".join(map(str, bits[at:at + 32].tolist())), 2)
        for v in (0, 1, U32_MAX, true - 1, true + 1):
            d = bits.copy()
            d[at:at + 32] = [(v >> (31 - i)) & 1 for i in range(32)]
            out.append((f"head{at}={v}", d, len(d)))
    rng = np.random.default_rng(seed)
    spots = [int(rng.integers(a + 32, b)) for a, b in zip(heads, heads[1:] + [len(bits)]) for _ in range(flips // 8)]
    for at in spots:
        d = bits.copy()
        d[at] ^= 1
        out.append((f"flip{at}", d, len(d)))
    return out


# ---- one stream through the device calls, between guard bands ------------------------------------------------------------------
def encode_wide_guarded(torch, dev, dev_lz77, parsed, offset, cap, **kw):
    """encode_wide into ``cap`` bytes between guard bands -> (status, nbits, the cap bytes as a numpy array); asserts the bands
    and everything behind the stream's last 32-bit word untouched (a faulted stream: every byte)"""
    whole, bits = guarded(torch, dev, cap)
    out = dev_lz77.EncodedBatch(bits, torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                torch.zeros(1, dtype=torch.int32, device=dev), cap)
    enc = dev_lz77.encode_wide(parsed, offset, out=out, **kw)
    torch.cuda.synchronize()
    assert guards_intact(whole)
    status, nbits, slot = int(enc.status.item()), int(enc.nbits64.item()), bits.cpu().numpy()
    assert int(enc.nbits.item()) & 0xFFFFFFFF == nbits & 0xFFFFFFFF and int(enc.bit_offset.item()) == 0
    used = 0 if status else min((nbits + 31) // 32 * 4, cap)
    assert (slot[used:] == FILL).all()
    return status, nbits, slot


def encode_batch_ref(torch, dev, dev_lz77, parsed, offset, stride):
    """the one-wave kernel on the same one-stream batch -> (status, nbits, the slot's bytes)"""
    enc = dev_lz77.encode_batch(parsed, offset, out_stride=stride)
    torch.cuda.synchronize()
    return int(enc.status.item()), int(enc.nbits.item()) & 0xFFFFFFFF, enc.bits.cpu().numpy()[:stride]


class Decoded:
    def __init__(self, status, n_seq, n_lit, consumed, seqs, lits, sync_passes=None):
        self.status, self.n_seq, self.n_lit, self.consumed = status, n_seq, n_lit, consumed
        self.seqs, self.lits, self.sync_passes = seqs, lits, sync_passes

    def scalars(self):
        return self.status, self.n_seq, self.n_lit, self.consumed

    def same_values(self, other):
        return self.seqs.tolist() == other.seqs.tolist() and self.lits.tolist() == other.lits.tolist()


def _rows_between_guards(torch, dev, dev_lz77, seq_cap, lit_cap, batch):
    wholes, rows = zip(*(guarded(torch, dev, seq_cap * 4) for _ in range(3)))
    lit_whole, lit = guarded(torch, dev, max(lit_cap, 1))
    words = lambda: torch.zeros(1, dtype=torch.int32, device=dev) if batch else None  # noqa: E731
    out = dev_lz77.DecodedBatch(*(r.view(torch.int32).view(1, seq_cap) for r in rows), lit, words(), words(), words(),
                                torch.zeros(1, dtype=torch.int64, device=dev), seq_cap, words())
    return wholes + (lit_whole,), rows, lit, out


def _collect(torch, wholes, rows, lit, res, seq_cap, lit_cap, wide):
    torch.cuda.synchronize()
    assert all(guards_intact(w) for w in wholes)
    status = int(res.status.item())
    n_seq, n_lit = int(res.n_seq.item()) & 0xFFFFFFFF, int(res.n_lit.item()) & 0xFFFFFFFF
    consumed = int(res.consumed.item()) & (0xFFFFFFFFFFFFFFFF if wide else 0xFFFFFFFF)
    assert n_seq <= seq_cap and n_lit <= lit_cap
    got_rows = [r.cpu().numpy().view(np.uint32) for r in rows]
    got_lit = lit.cpu().numpy()
    if status == 0:  # a clean stream leaves the rest of its rows and of the literal range alone
        assert all((r[n_seq:] == FILL32).all() for r in got_rows) and (got_lit[n_lit:] == FILL).all()
    seqs = np.stack([r[:n_seq] for r in got_rows], axis=1).astype(np.int64)
    return Decoded(status, n_seq, n_lit, consumed, seqs, got_lit[:n_lit].copy(),
                   int(res.sync_passes.item()) if wide else None)


def decode_wide_guarded(torch, dev, dev_lz77, d_bits, bit_offset, nbits, seq_cap, lit_cap, offset=16, **kw):
    """decode_wide of the nbits bits at bit_offset of the device buffer d_bits into rows and literals between guard bands"""
    wholes, rows, lit, out = _rows_between_guards(torch, dev, dev_lz77, seq_cap, lit_cap, batch=False)
    res = dev_lz77.decode_wide(d_bits, int(bit_offset), int(nbits), seq_cap, lit_cap, offset, out=out, **kw)
    return _collect(torch, wholes, rows, lit, res, seq_cap, lit_cap, wide=True)


def decode_batch_ref(torch, dev, dev_lz77, d_bits, bit_offset, nbits, seq_cap, lit_cap, offset=16):
    """the one-wave kernel on the same input, as a batch of one"""
    wholes, rows, lit, out = _rows_between_guards(torch, dev, dev_lz77, seq_cap, lit_cap, batch=True)
    t = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)  # noqa: E731
    as_i32 = lambda v: int(np.array([v], np.uint32).view(np.int32)[0])  # noqa: E731
    res = dev_lz77.decode_batch(d_bits, t(int(bit_offset), torch.int64), t(as_i32(nbits), torch.int32), seq_cap,
                                torch.zeros(1, dtype=torch.int64, device=dev), t(as_i32(lit_cap), torch.int32), offset, out=out)
    return _collect(torch, wholes, rows, lit, res, seq_cap, lit_cap, wide=False)


def bits_on_device(torch, dev, codes, lead_bits=(0, 3, 61), garbage=(61, 0, 3), seed=9):
    """0/1 arrays packed into ONE device buffer, stream s behind lead_bits[s % 3] random bits from a byte boundary on and
    followed by garbage[s % 3] random bits that count as its input -> (device uint8 tensor, bit offsets, bits fed)"""
    rng = np.random.default_rng(seed)
    parts, offs, fed, at = [], [], [], 0
    for s, code in enumerate(codes):
        lead = rng.integers(0, 2, lead_bits[s % len(lead_bits)]).astype(np.uint8)
        tail = rng.integers(0, 2, garbage[s % len(garbage)]).astype(np.uint8)
        pad = np.zeros((-(len(lead) + len(code) + len(tail))) % 32, np.uint8)  # the next stream starts on a word
        parts += [lead, np.asarray(code, np.uint8), tail, pad]
        offs.append(at + len(lead))
        fed.append(len(code) + len(tail))
        at += len(lead) + len(code) + len(tail) + len(pad)
    return torch.from_numpy(np.packbits(np.concatenate(parts))).to(dev), offs, fed
