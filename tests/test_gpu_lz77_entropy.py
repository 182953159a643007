"""LZ77's entropy stage on the GPU (csrc/scl_lz77_entropy.hip): encode_batch / decode_batch against the reference's goldens
and against the host classes, bit for bit; slots, rows and literal ranges between guard bands; the 32-bit code-length limit;
damaged input; and parse -> encode -> compact -> decode -> replay end to end.

Shapes are the smallest at which the kernels take another path: counts around the 64 values of one wave step, fields that
are empty, have one symbol or hit every bin, 1 / 3 / 4 / 5 / 257 streams, and the two Fibonacci fields around the limit."""
import numpy as np
import pytest

from lz77_entropy_helpers import (FILL, FILL32, GUARD, U32_MAX, guarded, guards_intact, header_positions, host_decode, host_encode,
                                  pack_bit_streams, synthetic_streams, upload_streams)
from lz77_helpers import golden_blocks, goldens, markov1_stream, pack_windows, use_host_prefix_coder
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from stanford_compression_library_amd.backend import models as dev_models
from stanford_compression_library_amd.compressors.lz77 import LZ77Encoder
from stanford_compression_library_amd.core.data_block import DataBlock

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED, ST_STATE, ST_SIZE = 0x1, 0x2, 0x4, 0x8, 0x20


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def expected():
    """host_encode of every synthetic stream, per offset, computed once"""
    mp = pytest.MonkeyPatch()
    use_host_prefix_coder(mp)
    try:
        out = {o: (streams, [host_encode(s, o) for s in streams])
               for o, streams in ((0, synthetic_streams(top=U32_MAX - 1)), (16, synthetic_streams()), (32, synthetic_streams()))}
    finally:
        mp.undo()
    return out


def encode_guarded(parsed, dev, offset, out_stride):
    """encode_batch into slots between guard bands -> (EncodedBatch, the slots as a numpy array [n, out_stride]); asserts
    the bands and, per slot, everything behind the stream's last 32-bit word untouched (a failed stream: the whole slot)"""
    n = int(parsed.n_seq.numel())
    whole, bits = guarded(torch, dev, n * out_stride)
    out = dev_lz77.EncodedBatch(bits, torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                                torch.zeros(n, dtype=torch.int32, device=dev), out_stride)
    enc = dev_lz77.encode_batch(parsed, offset, out=out)
    torch.cuda.synchronize()
    assert guards_intact(whole)
    slots = bits.cpu().numpy().reshape(n, out_stride)
    nbits, status = enc.nbits.cpu().numpy().view(np.uint32), enc.status.cpu().numpy()
    assert enc.bit_offset.cpu().numpy().tolist() == [8 * s * out_stride for s in range(n)]
    for s in range(n):
        used = 0 if status[s] else (int(nbits[s]) + 31) // 32 * 4
        assert (slots[s, used:] == FILL).all(), s
    return enc, slots


def decode_guarded(dev, bits, bit_offset, nbits, seq_cap, lit_caps, offset):
    """decode_batch into rows and literal ranges between guard bands (3 FILL bytes between the ranges)
    -> (status, consumed, [(sequences [k, 3], literals)] per stream); asserts that nothing outside what was decoded changed"""
    n = len(nbits)
    lit_caps = np.asarray(lit_caps, np.int64)
    lit_off = 1 + np.concatenate([[0], np.cumsum(lit_caps + 3)])[:-1].astype(np.int64)
    wholes, rows = zip(*(guarded(torch, dev, n * seq_cap * 4) for _ in range(3)))
    lit_whole, lit = guarded(torch, dev, int((lit_caps + 3).sum()) + 2)
    words = lambda: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = dev_lz77.DecodedBatch(*(r.view(torch.int32).view(n, seq_cap) for r in rows), lit, words(), words(), words(),
                                t(lit_off), seq_cap, words())
    res = dev_lz77.decode_batch(t(bits), t(bit_offset), t(nbits), seq_cap, t(lit_off), t(lit_caps.astype(np.uint32).view(np.int32)),
                                offset, out=out)
    torch.cuda.synchronize()
    assert all(guards_intact(w) for w in wholes) and guards_intact(lit_whole)
    got_rows = [r.cpu().numpy().view(np.uint32).reshape(n, seq_cap) for r in rows]
    got_lit = lit.cpu().numpy()
    n_seq, n_lit = res.n_seq.cpu().numpy().view(np.uint32), res.n_lit.cpu().numpy().view(np.uint32)
    status = res.status.cpu().numpy()
    streams, keep = [], np.ones(got_lit.size, bool)
    for s in range(n):
        assert n_seq[s] <= seq_cap and n_lit[s] <= lit_caps[s], s
        if status[s] == 0:  # a clean stream leaves the rest of its rows alone (a faulted one may have decoded a longer field)
            assert all((r[s, n_seq[s]:] == FILL32).all() for r in got_rows), s
        streams.append((np.stack([r[s, : n_seq[s]] for r in got_rows], axis=1).astype(np.int64),
                        got_lit[lit_off[s]: lit_off[s] + n_lit[s]].copy()))
        keep[lit_off[s]: lit_off[s] + lit_caps[s]] = False
    assert (got_lit[keep] == FILL).all()  # the bytes between the literal ranges
    return status, res.consumed.cpu().numpy().view(np.uint32), streams


def same_streams(got, want):
    return all(g[0].tolist() == w[0].tolist() and g[1].tolist() == np.asarray(w[1]).tolist() for g, w in zip(got, want))


# ---- 1. the goldens --------------------------------------------------------------------------------------------------------
def test_goldens_as_one_ragged_batch(dev):
    blocks = [blk for case in goldens()["lz77"] for blk in golden_blocks(case)]
    assert len(goldens()["lz77"]) == 31 and len(blocks) == 34
    streams = [(seq, lit) for _, _, seq, lit, _, _, _ in blocks]
    parsed = upload_streams(torch, dev, streams)
    stride = dev_lz77.entropy_slot_bytes(max(len(s) for s, _ in streams), max(len(l) for _, l in streams))
    enc, slots = encode_guarded(parsed, dev, 16, stride)
    assert not enc.status.any().item()
    nbits = enc.nbits.cpu().numpy()
    empties = 0
    for s, (_, _, seq, lit, out, want_nbits, consumed) in enumerate(blocks):
        assert nbits[s] == want_nbits, s
        assert np.array_equal(slots[s, : (want_nbits + 7) // 8], out[: (want_nbits + 7) // 8]), s
        assert len(set(consumed)) == 1 and consumed[0] == want_nbits
        if len(seq) == 0 and len(lit) == 0:
            empties += 1
            assert want_nbits == 128 and not slots[s, :16].any()
    assert empties >= 1
    # decode the golden bits with 0, 3 and 61 bits of garbage behind them, at varied alignments
    codes = [np.unpackbits(out)[:nb] for _, _, _, _, out, nb, _ in blocks]
    packed, bit_offset, in_nbits = pack_bit_streams(codes)
    assert len(set((bit_offset % 8).tolist())) >= 4 and (bit_offset % 2).any() and set((in_nbits - [len(c) for c in codes]).tolist()) == {0, 3, 61}
    status, used, got = decode_guarded(dev, packed, bit_offset, in_nbits, parsed.seq_cap, [len(l) for _, l in streams], 16)
    assert not status.any() and used.tolist() == [nb for *_, nb, _ in blocks]
    assert same_streams(got, streams)


# ---- 2. a synthetic ragged batch against the host classes ---------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 16, 32])
def test_synthetic_batch_equals_the_host_classes(dev, expected, offset):
    streams, want = expected[offset]
    stride = dev_lz77.entropy_slot_bytes(4097, 5000, offset)
    for n in (1, 3, 4, 5, 257):
        parsed = upload_streams(torch, dev, streams[:n])
        enc, slots = encode_guarded(parsed, dev, offset, stride)
        assert not enc.status.any().item(), n
        nbits = enc.nbits.cpu().numpy()
        for s in range(n):
            assert nbits[s] == len(want[s]), (n, s)
            assert np.array_equal(slots[s, : (len(want[s]) + 7) // 8], np.packbits(want[s])), (n, s)
        # the encoder's own slots, decoded
        status, used, got = decode_guarded(dev, slots.reshape(-1), enc.bit_offset.cpu().numpy(), nbits, parsed.seq_cap,
                                           [len(l) for _, l in streams[:n]], offset)
        assert not status.any() and used.tolist() == nbits.tolist(), n
        assert same_streams(got, streams[:n]), n


def test_the_value_without_a_bin_is_refused_as_the_reference_refuses_it(dev):
    """binned_offset 0 and the value 2^32 - 1: v - o + 1 = 2^32 has log 32, and the alphabet ends at bin 31.  The reference
    raises "too large" (tests/test_lz77_entropy_host.py); the kernel reports SCL_ST_SYMBOL and stores nothing.  Under any other
    offset the value is coded (the synthetic streams hold it)."""
    streams = [(np.array([[1, 2, 3]], np.int64), np.zeros(2, np.uint8)),
               (np.array([[1, 2, 3], [4, U32_MAX, 5]], np.int64), np.zeros(2, np.uint8)),
               (np.array([[U32_MAX - 1, 2, 3]], np.int64), np.zeros(0, np.uint8))]
    enc, _ = encode_guarded(upload_streams(torch, dev, streams), dev, 0, 256)
    assert enc.status.cpu().tolist() == [0, ST_SYMBOL, 0] and enc.nbits.cpu().tolist()[1] == 0


# ---- 3. capacity and ownership -------------------------------------------------------------------------------------------------
def test_short_slots_and_short_rows(dev, expected):
    streams, want = expected[16]
    streams, want = streams[1:60], want[1:60]
    parsed = upload_streams(torch, dev, streams)
    stride = 128
    fits = np.array([(len(w) + 7) // 8 <= stride for w in want])
    assert fits.any() and (~fits).any()
    enc, slots = encode_guarded(parsed, dev, 16, stride)
    assert enc.status.cpu().numpy().tolist() == [0 if f else ST_CAPACITY for f in fits]
    assert enc.nbits.cpu().numpy().tolist() == [len(w) for w in want]  # what a large-enough run reports
    for s in np.flatnonzero(fits):
        assert np.array_equal(slots[s, : (len(want[s]) + 7) // 8], np.packbits(want[s])), s
    # decode: one entry short in the rows, then one byte short in a literal range
    pick = [s for s in range(len(streams)) if len(streams[s][0]) and len(streams[s][1])][:12]
    codes = [want[s] for s in pick]
    packed, bit_offset, in_nbits = pack_bit_streams(codes, garbage=(0,))
    seq_cap = max(len(streams[s][0]) for s in pick)
    status, _, _ = decode_guarded(dev, packed, bit_offset, in_nbits, seq_cap - 1, [len(streams[s][1]) for s in pick], 16)
    assert status.tolist() == [ST_CAPACITY if len(streams[s][0]) == seq_cap else 0 for s in pick] and status.any()
    short = [len(streams[s][1]) - (i % 2) for i, s in enumerate(pick)]
    status, _, got = decode_guarded(dev, packed, bit_offset, in_nbits, seq_cap, short, 16)
    assert status.tolist() == [ST_CAPACITY if i % 2 else 0 for i in range(len(pick))]
    assert same_streams(got[::2], [streams[s] for s in pick[::2]])


# ---- 4. the code-length limit ----------------------------------------------------------------------------------------------------
def test_fibonacci_counts_at_the_32_bit_limit(dev):
    fib = [1, 1]
    while len(fib) < 34:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(4)
    for K, fits in ((33, True), (34, False)):
        counts = np.array(fib[:K], np.int64)
        lit = torch.from_numpy(rng.permutation(np.repeat(np.arange(K, dtype=np.uint8), counts))).to(dev)
        n = int(counts.sum())
        assert n == (9227464, 14930351)[K - 33]
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        parsed = dev_lz77.ParsedBatch(zero.view(1, 1), zero.view(1, 1).clone(), zero.view(1, 1).clone(), lit, zero.clone(),
                                      torch.tensor([n], dtype=torch.int32, device=dev), zero.clone(),
                                      torch.zeros(1, dtype=torch.int64, device=dev), 1)
        enc = dev_lz77.encode_batch(parsed, out_stride=dev_lz77.entropy_slot_bytes(0, n))
        torch.cuda.synchronize()
        if not fits:
            assert enc.status.cpu().tolist() == [ST_SIZE] and enc.nbits.cpu().tolist() == [0]
            assert not enc.bits.any().item()  # nothing is emitted for it
            continue
        _, length = dev_lz77.huffman_from_counts(np.bincount(np.arange(K), weights=counts, minlength=256).astype(np.uint64))
        assert length.max() == 32
        full = np.zeros(256, np.int64)
        full[:K] = counts
        y = full + 1
        nlen = np.array([int(v).bit_length() - 1 for v in y])
        elias = sum(2 * (int(v + 1).bit_length() - 1) + 1 + int(v) for v in nlen)
        want = 3 * 32 + 32 + elias + 32 + int((full * length.astype(np.int64)).sum())
        assert enc.status.cpu().tolist() == [0] and enc.nbits.cpu().tolist() == [want]
        dec = dev_lz77.decode_batch(enc.bits, enc.bit_offset, enc.nbits, 1, parsed.lit_off,
                                    torch.tensor([n], dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        assert dec.status.cpu().tolist() == [0] and dec.n_lit.cpu().tolist() == [n] and dec.n_seq.cpu().tolist() == [0]
        assert dec.consumed.cpu().tolist() == [want] and torch.equal(dec.literals[:n], lit)


# ---- 5. damaged input -----------------------------------------------------------------------------------------------------------
def test_damaged_streams_raise_a_status_or_decode_to_what_the_classes_decode(dev, expected):
    """Truncated inputs, every size header replaced by 0, 1, 2^32 - 1 and its value -+ 1, and 200 single-bit flips, all in ONE
    call between guard bands.  Every stream either raises a status or is a block the host classes decode to the very same
    sequences, literals and bit count (so it re-encodes to a block that decodes to it again)."""
    streams, want = expected[16]
    base = [s for s in range(5, 60) if len(streams[s][0]) and len(streams[s][1]) and len(want[s]) < 6000][:3]
    assert len(base) == 3
    rng = np.random.default_rng(12)
    damaged, nbits_fed, origin, cuts = [], [], [], []
    for s in base:
        bits = want[s]
        heads = header_positions(streams[s], bits)
        assert len(heads) == 8
        for cut in (0, 1, 31, 32, 33, len(bits) // 2, len(bits) - 1):
            cuts.append(len(damaged))
            damaged.append(bits)
            nbits_fed.append(cut)
            origin.append(s)
        for at in heads:
            true = int("".join(map(str, bits[at:at + 32].tolist())), 2)
            for v in (0, 1, U32_MAX, true - 1, true + 1):
                d = bits.copy()
                d[at:at + 32] = [(v >> (31 - i)) & 1 for i in range(32)]
                damaged.append(d)
                nbits_fed.append(len(d))
                origin.append(s)
    for _ in range(200):
        s = base[int(rng.integers(0, 3))]
        d = want[s].copy()
        d[int(rng.integers(0, len(d)))] ^= 1
        damaged.append(d)
        nbits_fed.append(len(d))
        origin.append(s)
    packed, bit_offset, _ = pack_bit_streams(damaged, garbage=(0,))
    in_nbits = np.array(nbits_fed, np.uint32).view(np.int32)
    seq_cap = max(len(streams[s][0]) for s in base) + 2
    lit_caps = [len(streams[s][1]) + 2 for s in origin]
    status, used, got = decode_guarded(dev, packed, bit_offset, in_nbits, seq_cap, lit_caps, 16)  # it returns: nothing hangs
    assert (status[cuts] != 0).all()  # every section is needed whole
    clean = np.flatnonzero(status == 0)
    assert 0 < len(clean) < len(damaged)
    mp = pytest.MonkeyPatch()
    use_host_prefix_coder(mp)
    try:
        for i in clean.tolist():
            seq, lit = got[i]
            try:
                (host_seq, host_lit), host_used = host_decode(damaged[i][: nbits_fed[i]])
            except AssertionError as e:  # the one limit the classes have and the kernels have not: a count so large
                assert "too small" in str(e), i  # that another symbol's probability falls below 1e-6 (prob_dist.py)
            else:
                assert host_used == used[i] and host_seq.tolist() == seq.tolist() and host_lit.tolist() == lit.tolist(), i
            again = host_encode((seq, lit))
            (seq2, lit2), _ = host_decode(again)
            assert seq2.tolist() == seq.tolist() and lit2.tolist() == lit.tolist(), i
    finally:
        mp.undo()


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_compress_compact_decompress(dev):
    rng = np.random.default_rng(6)
    source = markov1_stream(300 * 2200, seed=6)
    windows, at = [], 0
    for s in range(300):
        n = int(rng.integers(1800, 2200))
        windows.append(source[at: at + n])
        at += n
    windows += [np.zeros(0, np.uint8), np.array([7], np.uint8), np.zeros(0, np.uint8), np.array([200], np.uint8)]
    batch = pack_windows(windows, [0] * len(windows))
    win, win_off, start = (torch.from_numpy(batch[k]).to(dev) for k in ("buf", "win_off", "start"))
    enc, parsed = dev_lz77.compress_batch(win, win_off, start, 6, 64)
    assert not (enc.status | parsed.status).any().item()
    dense, offsets = dev_models.compact(enc)
    offsets_h, nbits_h = offsets.cpu().numpy(), enc.nbits.cpu().numpy()
    assert (np.diff(offsets_h) == (nbits_h + 7) // 8).all()
    assert nbits_h[300] == 128 and nbits_h[302] == 128  # the empty streams
    # back from the dense buffer: fresh slots that hold nothing yet
    slots = torch.full_like(win, FILL)
    have = torch.zeros_like(start)
    out_len, status, used = dev_lz77.decompress_batch(dense, offsets[:-1] * 8, enc.nbits, slots, win_off, have, parsed.seq_cap)
    torch.cuda.synchronize()
    assert not status.any().item() and torch.equal(used, enc.nbits)
    assert out_len.cpu().numpy().tolist() == [len(w) for w in windows] and torch.equal(slots, win)
    # the class path's bits, for a sample
    dense_h = dense.cpu().numpy()
    for s in (0, 137, 299, 300, 301):
        bits = LZ77Encoder().encode_block(DataBlock(windows[s].tolist()))
        assert len(bits) == nbits_h[s] and np.array_equal(dense_h[offsets_h[s]: offsets_h[s + 1]], bits.packed()), s
