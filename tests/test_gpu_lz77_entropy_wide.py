"""LZ77's entropy stage for ONE stream on the whole GPU (csrc/scl_lz77_entropy_wide.hip): encode_wide / decode_wide against
what the suite already trusts -- the reference's goldens, and encode_batch / decode_batch on a batch of the one stream -- bit
for bit, with every output between guard bands.

Shapes are the smallest at which the kernels take another path: counts around the 4096 values of a tile, literal fields
inside one decoder workgroup (32768 bits), just over one and over nine, fields that are empty or have one symbol, residual
widths all 0 and all 31, section bases at every alignment, capacities exact, one byte short and not a multiple of 4."""
import numpy as np
import pytest

from lz77_entropy_helpers import U32_MAX, header_positions, upload_streams
from lz77_entropy_wide_helpers import (GROUP_BITS, bits_on_device, damaged_inputs, decode_batch_ref, decode_wide_guarded,
                                       edge_stream, encode_batch_ref, encode_wide_guarded, grid_cases, never_counts,
                                       never_in_step_stream)
from lz77_helpers import golden_blocks, goldens, markov1_stream
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from stanford_compression_library_amd.backend import models as dev_models

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED, ST_STATE, ST_SIZE = 0x1, 0x2, 0x4, 0x8, 0x20


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def one(dev, stream):
    return upload_streams(torch, dev, [stream])


def unpack(slot, nbits):
    return np.unpackbits(slot[: (nbits + 7) // 8])[:nbits]


# ---- 1. the goldens --------------------------------------------------------------------------------------------------------
def test_goldens(dev):
    blocks = [blk for case in goldens()["lz77"] for blk in golden_blocks(case)]
    assert len(blocks) == 34
    codes = []
    for s, (_, _, seq, lit, out, want_nbits, _) in enumerate(blocks):
        cap = dev_lz77.entropy_slot_bytes(len(seq), len(lit))
        status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, one(dev, (seq, lit)), 16, cap)
        assert status == 0 and nbits == want_nbits, s
        assert np.array_equal(slot[: (nbits + 7) // 8], out[: (nbits + 7) // 8]), s
        codes.append(np.unpackbits(out)[:want_nbits])
    # every block at bit offsets 0, 3 and 61, with garbage bits behind it
    for shift in range(3):
        lead = ((0, 3, 61), (3, 61, 0), (61, 0, 3))[shift]
        d_bits, offs, fed = bits_on_device(torch, dev, codes, lead_bits=lead, seed=9 + shift)
        for s, (_, _, seq, lit, _, want_nbits, _) in enumerate(blocks):
            assert offs[s] % 32 == lead[s % 3] % 32
            got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, offs[s], fed[s], max(len(seq), 1), len(lit))
            assert got.scalars() == (0, len(seq), len(lit), want_nbits), (shift, s)
            assert got.seqs.tolist() == seq.tolist() and got.lits.tolist() == lit.tolist(), (shift, s)


# ---- 2. tile and workgroup edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", grid_cases(), ids=lambda c: c[0])
def test_edges_equal_the_one_wave_kernels(dev, case):
    _, (seq, lit), offset = case
    parsed = one(dev, (seq, lit))
    stride = dev_lz77.entropy_slot_bytes(len(seq), len(lit), offset)
    want_status, want_nbits, want = encode_batch_ref(torch, dev, dev_lz77, parsed, offset, stride)
    status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, parsed, offset, stride)
    assert (status, nbits) == (want_status, want_nbits) and status == 0
    n_bytes = (nbits + 31) // 32 * 4  # every bit up to the next word boundary is defined
    assert np.array_equal(slot[:n_bytes], want[:n_bytes])
    d_bits = torch.from_numpy(slot.copy()).to(dev)
    got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, 0, nbits, max(len(seq), 1), len(lit), offset)
    assert got.scalars() == (0, len(seq), len(lit), nbits)
    assert got.seqs.tolist() == seq.tolist() and got.lits.tolist() == lit.tolist()
    if len(lit) == 40000:
        assert 8 * GROUP_BITS < 40000 * 7 <= 9 * GROUP_BITS


# ---- 3. section bases at every alignment, capacities ---------------------------------------------------------------------------
def test_section_bases_at_every_alignment_and_the_capacity_edges(dev):
    """Streams whose counts move the four fields over the bit positions: the one-wave kernel codes a batch of candidates, and
    the ones picked start a field at 0, 1 and 31 mod 32 (and the codeword and residual sections wherever that leaves them)."""
    rng = np.random.default_rng(31)
    candidates = [edge_stream(int(rng.integers(1, 40)), int(rng.integers(1, 60)), 16, 500 + i, lit_hi=int(rng.integers(2, 257)))
                  for i in range(96)]
    stride = dev_lz77.entropy_slot_bytes(40, 60)
    enc = dev_lz77.encode_batch(upload_streams(torch, dev, candidates), 16, out_stride=stride)
    torch.cuda.synchronize()
    assert not enc.status.any().item()
    slots, nbits_all = enc.bits.cpu().numpy()[: 96 * stride].reshape(96, stride), enc.nbits.cpu().numpy()
    picked, covered = [], set()
    for s, stream in enumerate(candidates):
        bits = unpack(slots[s], int(nbits_all[s]))
        starts = {p % 32 for p in header_positions(stream, bits)[::2][1:]}  # the fields behind the first
        if (starts & {0, 1, 31}) - covered:
            covered |= starts & {0, 1, 31}
            picked.append((stream, bits))
    assert covered == {0, 1, 31} and len(picked) <= 3
    for stream, bits in picked:
        parsed = one(dev, stream)
        exact = (len(bits) + 7) // 8
        for cap in (exact, exact + 1, exact + 2, exact + 3, exact + 5):  # exact, and every remainder mod 4
            status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, parsed, 16, cap)
            assert (status, nbits) == (0, len(bits)), cap
            assert np.array_equal(slot[:exact], np.packbits(bits)), cap  # (the guard bands: nothing at or past the cap)
        status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, parsed, 16, exact - 1)
        assert (status, nbits) == (ST_CAPACITY, len(bits))  # nothing stored: encode_wide_guarded saw every byte untouched


# ---- 4. faults on encode -----------------------------------------------------------------------------------------------------
def test_the_value_without_a_bin(dev):
    seq = np.array([[1, 2, 3], [4, U32_MAX, 5]], np.int64)
    parsed = one(dev, (seq, np.zeros(2, np.uint8)))
    assert encode_batch_ref(torch, dev, dev_lz77, parsed, 0, 256)[:2] == (ST_SYMBOL, 0)
    assert encode_wide_guarded(torch, dev, dev_lz77, parsed, 0, 256)[:2] == (ST_SYMBOL, 0)
    assert encode_wide_guarded(torch, dev, dev_lz77, parsed, 16, 256)[0] == 0  # under any other offset it is coded


def test_fibonacci_counts_at_the_32_bit_limit(dev):
    fib = [1, 1]
    while len(fib) < 34:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(4)
    for K, fits in ((33, True), (34, False)):
        counts = np.array(fib[:K], np.int64)
        lit = torch.from_numpy(rng.permutation(np.repeat(np.arange(K, dtype=np.uint8), counts))).to(dev)
        n = int(counts.sum())
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        parsed = dev_lz77.ParsedBatch(zero.view(1, 1), zero.view(1, 1).clone(), zero.view(1, 1).clone(), lit, zero.clone(),
                                      torch.tensor([n], dtype=torch.int32, device=dev), zero.clone(),
                                      torch.zeros(1, dtype=torch.int64, device=dev), 1)
        stride = dev_lz77.entropy_slot_bytes(0, n)
        want_status, want_nbits, want = encode_batch_ref(torch, dev, dev_lz77, parsed, 16, stride)
        assert want_status == (0 if fits else ST_SIZE)
        status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, parsed, 16, stride)  # (a fault: no byte stored)
        assert (status, nbits) == (want_status, want_nbits)
        if fits:
            n_bytes = (nbits + 31) // 32 * 4
            assert nbits > 0 and np.array_equal(slot[:n_bytes], want[:n_bytes])


# ---- 5. faults on decode -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_groups(dev):
    """a stream whose literal field takes three decoder workgroups and whose sequence fields take one each, coded by the
    one-wave kernel"""
    stream = edge_stream(3000, 12000, 16, 77, lit_hi=256)
    parsed = one(dev, stream)
    status, nbits, slot = encode_batch_ref(torch, dev, dev_lz77, parsed, 16, dev_lz77.entropy_slot_bytes(3000, 12000))
    assert status == 0 and 12000 * 7 > 2 * GROUP_BITS
    return stream, unpack(slot, nbits)


def test_damaged_streams_get_the_one_wave_decoders_verdict(dev, three_groups):
    stream, bits = three_groups
    cases = damaged_inputs(stream, bits)
    d_bits, offs, _ = bits_on_device(torch, dev, [d for _, d, _ in cases], garbage=(0,))
    seq_cap, lit_cap = len(stream[0]) + 2, len(stream[1]) + 2
    faults = clean = 0
    seen = set()
    for (name, _, fed), at in zip(cases, offs):
        want = decode_batch_ref(torch, dev, dev_lz77, d_bits, at, fed, seq_cap, lit_cap)
        got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, at, fed, seq_cap, lit_cap)
        assert got.scalars() == want.scalars(), (name, got.scalars(), want.scalars())
        seen.add(want.status)
        if want.status == 0:
            clean += 1
            assert got.same_values(want), name
        else:
            faults += 1
    assert faults > 40 and clean > 0
    assert {ST_TRUNCATED, ST_STATE} <= seen


def test_rows_and_literals_one_too_small(dev, three_groups):
    stream, bits = three_groups
    d_bits, offs, fed = bits_on_device(torch, dev, [bits], lead_bits=(3,), garbage=(0,))
    n_seq, n_lit = len(stream[0]), len(stream[1])
    for seq_cap, lit_cap in ((n_seq - 1, n_lit), (n_seq, n_lit - 1)):
        want = decode_batch_ref(torch, dev, dev_lz77, d_bits, offs[0], fed[0], seq_cap, lit_cap)
        got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, offs[0], fed[0], seq_cap, lit_cap)  # (guards: nothing past them)
        assert want.status == ST_CAPACITY and got.scalars() == want.scalars()
    got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, offs[0], fed[0], n_seq, n_lit)
    assert got.scalars() == (0, n_seq, n_lit, len(bits)) and got.seqs.tolist() == stream[0].tolist()


# ---- 6. the code that never falls into step ------------------------------------------------------------------------------------
def test_the_carry_between_decoder_workgroups(dev):
    codes, lengths = dev_lz77.huffman_from_counts(never_counts())
    bits, literals = never_in_step_stream(codes, lengths)
    d_bits, offs, fed = bits_on_device(torch, dev, [bits], lead_bits=(0,), garbage=(0,))
    n_groups = -(-(3 * len(literals) // 2) // GROUP_BITS)
    assert n_groups == 5
    want = decode_batch_ref(torch, dev, dev_lz77, d_bits, offs[0], fed[0], 1, len(literals))
    got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, offs[0], fed[0], 1, len(literals))
    assert want.scalars() == (0, 0, len(literals), len(bits)) and want.lits.tolist() == literals.tolist()
    assert got.scalars() == want.scalars() and got.same_values(want)
    assert 1 <= got.sync_passes <= n_groups


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------
def test_compress_wide_compact_decompress_wide(dev):
    history, block = 100 << 10, 1 << 20
    window = torch.from_numpy(markov1_stream(history + block, seed=21)).to(dev)
    win_off = torch.tensor([0, window.numel()], dtype=torch.int64, device=dev)
    start = torch.tensor([history], dtype=torch.int32, device=dev)
    want, _ = dev_lz77.compress_batch(window, win_off, start, 6, 64)
    # scratch from a larger call, reused; then the same buffers written again (out=)
    big = torch.empty(2 * max(dev_lz77.wide_scratch_bytes(window.numel()),
                              dev_lz77.entropy_wide_scratch_bytes(block // 6, block, 16 * block)), dtype=torch.uint8, device=dev)
    big.fill_(0xA5)
    enc, parsed = dev_lz77.compress_wide(window, history, 6, 64, out_stride=want.out_stride, scratch=big)
    torch.cuda.synchronize()
    assert int(want.status.item()) == 0 and int(enc.status.item()) == 0 and int(parsed.status.item()) == 0
    nbits = int(want.nbits.item())
    assert int(enc.nbits64.item()) == nbits and torch.equal(enc.bits[: (nbits + 7) // 8], want.bits[: (nbits + 7) // 8])
    enc.bits.fill_(0x5A)
    again, _ = dev_lz77.compress_wide(window, history, 6, 64, scratch=big, out=enc)
    assert again is enc and torch.equal(enc.bits[: (nbits + 7) // 8], want.bits[: (nbits + 7) // 8])
    dense, offsets = dev_models.compact(enc)
    assert offsets.cpu().tolist() == [0, (nbits + 7) // 8]
    slot = torch.zeros_like(window)
    slot[:history] = window[:history]
    out_len, status, used = dev_lz77.decompress_wide(dense, 0, nbits, slot, history, parsed.seq_cap, scratch=big)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(used.item()) == nbits and int(out_len.item()) == block
    assert torch.equal(slot, window)


# ---- 8. the threshold ------------------------------------------------------------------------------------------------------
def test_the_same_bits_on_both_sides_of_the_threshold(dev):
    """the threshold counts coded values, 3 n_seq + n_lit: a stream of exactly that many and one of one fewer"""
    t = dev_lz77.entropy_wide_threshold()
    n_seq = min(t // 6, 5000)
    assert t >= 1 and 3 * n_seq <= t - 1
    for values in (t, t - 1):
        seq, lit = edge_stream(n_seq, values - 3 * n_seq, 16, 600 + values % 2, lit_hi=200)
        assert 3 * len(seq) + len(lit) == values
        parsed = one(dev, (seq, lit))
        stride = dev_lz77.entropy_slot_bytes(len(seq), len(lit))
        want_status, want_nbits, want = encode_batch_ref(torch, dev, dev_lz77, parsed, 16, stride)
        status, nbits, slot = encode_wide_guarded(torch, dev, dev_lz77, parsed, 16, stride)
        assert (status, nbits) == (want_status, want_nbits) == (0, nbits)
        n_bytes = (nbits + 31) // 32 * 4
        assert np.array_equal(slot[:n_bytes], want[:n_bytes])
        d_bits = torch.from_numpy(slot.copy()).to(dev)
        got = decode_wide_guarded(torch, dev, dev_lz77, d_bits, 0, nbits, max(len(seq), 1), len(lit))
        ref = decode_batch_ref(torch, dev, dev_lz77, d_bits, 0, nbits, max(len(seq), 1), len(lit))
        assert got.scalars() == ref.scalars() == (0, len(seq), len(lit), nbits) and got.same_values(ref)
