"""GPU: the prefix-code kernels (csrc/scl_prefix.hip, csrc/scl_prefix_block.hip) at the limits their headers document:
codes of 28..32 bits with the top bit set, the tuned decoder's table geometry (T = max_len = 11, one level of deep nodes,
512 and 513 deep nodes), scans of more than 1024 entries, and the exact number of correction passes.

Every expectation comes from prefix_helpers (encode_vectorised, decode_reference, the table builders), which
tests/test_prefix_reference.py pins on the reference's goldens, or from a derivation written next to the assertion."""
import functools

import numpy as np
import pytest

from prefix_helpers import (ST_CAPACITY, ST_STATE, ST_TRUNCATED, comb, count_deep_nodes, decode_reference, deep_chains,
                            encode_vectorised, stream_bits, table_case)
from test_gpu_prefix import Arena as RowArena
from test_gpu_prefix import arena_decoded, arena_encoded, check_decoded, check_encoded, decode_damaged, forms, to_rows
from test_gpu_prefix_block import Arena, block_decode, device, sym_tensor
from test_gpu_prefix_block import table as block_table

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5
BUILDERS = {"comb11": lambda: comb(11), "comb12": lambda: comb(12), "comb32": lambda: comb(32),
            "deep512": lambda: deep_chains(512), "deep513": lambda: deep_chains(513)}
LIMIT_TABLES = list(BUILDERS)
WITH_32 = ["comb32", "deep512", "deep513"]


class Table:
    def __init__(self, name):
        from stanford_compression_library_amd.backend.models import PrefixModel

        self.name = name
        self.code, self.len = BUILDERS[name]()
        self.K, self.max_len, self.min_len = len(self.code), int(self.len.max()), int(self.len.min())
        self.longest = np.nonzero(self.len == self.max_len)[0]  # comb: the two codes of L bits; deep_chains: 24 of 32 bits
        self.model = PrefixModel(self.code, self.len)
        info = self.model.block_info()
        self.S, self.tile, self.W = int(info.sub_bits), int(info.tile_symbols), 256 * int(info.sub_bits)

    def encode(self, sym):
        return encode_vectorised(self.code, self.len, sym)

    def decode(self, data, bit_offset, nbits, cap):
        sym, consumed, status = decode_reference(self.code, self.len, data, bit_offset, nbits, cap)
        return sym, len(sym), consumed, status

    def back_to_back(self, n):
        """the longest codewords alone, in turn: comb(32) alternates 0xFFFFFFFE and 0xFFFFFFFF"""
        return self.longest[np.arange(n) % len(self.longest)]

    def mix(self, rng, n):
        """a longest codeword with probability 0.8, any symbol otherwise"""
        sym = rng.integers(0, self.K, int(n))
        long = rng.random(int(n)) < 0.8
        sym[long] = rng.choice(self.longest, int(long.sum()))
        return sym

    def mix_bits(self, rng, target):
        """a mix whose stream is the first to reach `target` bits"""
        sym = self.mix(rng, target // self.min_len + 1)
        return sym[:int(np.searchsorted(np.cumsum(self.len[sym]), target)) + 1]


@functools.lru_cache(maxsize=None)
def table(name):
    device()
    return Table(name)


def place(packed, nbits, bit_offset, behind, dev):
    """a device buffer (a multiple of 16 bytes) with the stream at `bit_offset`: ones in front of it, and `behind` (0, 1, or
    an rng for random bits) in every bit after it"""
    total = ((bit_offset + nbits + 7) // 8 + 64 + 15) // 16 * 16
    bits = np.ones(8 * total, np.uint8)
    tail = 8 * total - bit_offset - nbits
    bits[bit_offset:bit_offset + nbits] = np.unpackbits(np.asarray(packed, np.uint8))[:nbits]
    bits[bit_offset + nbits:] = behind if isinstance(behind, int) else behind.integers(0, 2, tail)
    return torch.from_numpy(np.packbits(bits)).to(dev)


def same_as_reference(t, data, bit_offset, nbits, cap, what):
    """the block decoder, between guard bands, against decode_reference"""
    got = block_decode(t, data, bit_offset, nbits, cap, what)
    want = t.decode(data.cpu().numpy(), bit_offset, nbits, cap)
    assert got[1:4] == want[1:4], f"{what}: (n_out, consumed, status) {got[1:4]}, the reference {want[1:4]}"
    assert np.array_equal(got[0], want[0]), f"{what}: symbols differ"
    return got


def batch_same_as_reference(t, streams, cap, what):
    """[(data bytes, nbits)] as one chunk each, at bit 3 of slots of one stride, through both one-lane forms (which must
    agree: decode_damaged) against decode_reference -> [(symbols, n_out, consumed, status)] of the reference"""
    dev = device()
    stride = (max(len(d) for d, _ in streams) + 1 + 15) // 16 * 16
    host = np.full(len(streams) * stride, 0xFF, np.uint8)
    for c, (d, nb) in enumerate(streams):
        bits = np.unpackbits(host[c * stride:(c + 1) * stride])
        bits[3:3 + 8 * len(d)] = np.unpackbits(np.asarray(d, np.uint8))
        host[c * stride:(c + 1) * stride] = np.packbits(bits)
    offsets = 8 * stride * np.arange(len(streams), dtype=np.int64) + 3
    nbits = np.array([nb for _, nb in streams], np.int64).astype(np.uint32).view(np.int32)
    sym, lens, used, status = decode_damaged(t.model, torch.from_numpy(host).to(dev), torch.from_numpy(offsets).to(dev),
                                             torch.from_numpy(nbits).to(dev), cap, what)
    wants = []
    for c, (d, nb) in enumerate(streams):
        want = t.decode(host, int(offsets[c]), nb, cap)
        got = (int(lens[c]), int(used[c]) & 0xFFFFFFFF, int(status[c]))
        assert got == want[1:], f"{what}: chunk {c}: (n_out, consumed, status) {got}, the reference {want[1:]}"
        assert np.array_equal(sym[c, :lens[c]].astype(np.int64), want[0]), f"{what}: chunk {c}: symbols differ"
        wants.append(want)
    return wants


# ---- the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIMIT_TABLES)
def test_table_geometry(name):
    t = table(name)
    info = t.model.info()
    assert (info.K, info.min_len, info.max_len) == (t.K, t.min_len, t.max_len) and t.K <= 256
    assert info.lut_bits == min(t.max_len, 11)
    n_deep = count_deep_nodes(t.code, t.len)
    assert n_deep == {"comb11": 0, "comb12": 1, "comb32": 21, "deep512": 512, "deep513": 513}[name]
    assert t.model.fast_path() == (n_deep <= 512) == (name != "deep513")
    # a byte alphabet that falls off the tuned path runs the any-parameter byte kernels with the default setting
    assert forms(t.model)[0] == (False, "default" if name == "deep513" else "tuned")
    if name in WITH_32:
        assert t.max_len == 32 and (t.code[t.longest] >= 1 << 31).all()
    if name == "comb32":
        assert sorted(t.code[t.longest].tolist()) == [0xFFFFFFFE, 0xFFFFFFFF]


# ---- ragged batches through both one-lane forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIMIT_TABLES)
def test_ragged_batch_in_slots_of_exactly_slot_bytes(name):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(t.K)
    n_chunks, longest = 270, 320  # a full workgroup of lanes and a partial one
    lens = rng.integers(0, longest + 1, n_chunks)
    lens[:4] = [0, 1, longest, longest - 1]
    chunks = [t.mix(rng, n) for n in lens]
    chunks[2] = t.back_to_back(longest)  # with 32-bit codes the tuned reader consumes four whole words between refills
    assert len(chunks[2]) >= 300 and (t.len[chunks[2]] == t.max_len).all() and len(set(chunks[2][:2])) == 2
    if name.startswith("deep"):  # every long symbol: every deep node, index 511 and the leaf of symbol 255 among them
        every_long = np.nonzero(t.len > 11)[0]
        chunks[5] = rng.permutation(np.concatenate([every_long, every_long, t.mix(rng, 40)]))
        assert set(every_long) <= set(chunks[5]) and 255 in every_long and len(every_long) >= 25
    expected = [t.encode(c) for c in chunks]
    for chunk, (packed, nb) in zip(chunks, expected):
        back = t.decode(packed, 0, nb, len(chunk))
        assert back[1:] == (len(chunk), nb, 0) and np.array_equal(back[0], chunk)
    sym, d_lens, _ = to_rows(t.model, chunks, dev)
    stride = t.model.slot_bytes(longest)
    assert stride % 128 == 0 and stride >= (longest * t.max_len + 7) // 8
    buffers = []
    for any_par, enc_name in forms(t.model):
        arena = RowArena(n_chunks * (stride + 400) + 80 * GUARD, dev)
        enc = arena_encoded(arena, n_chunks, stride)
        enc.data.zero_()
        t.model.encode_batch(sym[:, :longest], d_lens, out=enc, any_parameter_kernels=any_par)
        torch.cuda.synchronize()
        arena.check(f"{name}/{enc_name} encode")
        check_encoded(enc, expected, f"{name}/{enc_name}")
        buffers.append(enc.data.cpu().numpy())
        for dec_any, dec_name in forms(t.model):
            rows, out = arena_decoded(arena, n_chunks, 320, longest)
            dec = t.model.decode_batch(enc.data, enc.bit_offset, enc.nbits, longest, out=out, any_parameter_kernels=dec_any)
            torch.cuda.synchronize()
            arena.check(f"{name}/{enc_name}->{dec_name} decode")
            check_decoded(dec, chunks, expected, f"{name}/{enc_name}->{dec_name}")
            host = rows.cpu().numpy().reshape(n_chunks, 320)
            for c, chunk in enumerate(chunks):
                assert (host[c, len(chunk):] == FILL).all(), f"{name}/{dec_name}: row {c} written behind its symbols"
    assert np.array_equal(buffers[0], buffers[1]), f"{name}: the two forms' slots differ"


@pytest.mark.parametrize("name", WITH_32)
def test_slot_filled_to_its_last_byte_and_one_symbol_more(name):
    """32-bit codewords alone: `stride / 4` of them fill a slot to the last byte and fit; one more does not"""
    dev = device()
    t = table(name)
    stride = 1296  # a multiple of 16, not of 128: 324 words
    fits, over = t.back_to_back(stride // 4), t.back_to_back(stride // 4 + 1)
    chunks = [fits, over, fits[:100], over, fits]
    expected = [t.encode(c) for c in chunks]
    assert expected[0][1] == 8 * stride and expected[1][1] == 8 * stride + 32
    sym, d_lens, _ = to_rows(t.model, chunks, dev)
    for any_par, form in forms(t.model):
        arena = RowArena(5 * stride + 80 * GUARD, dev)
        enc = arena_encoded(arena, 5, stride)
        t.model.encode_batch(sym, d_lens, out=enc, any_parameter_kernels=any_par)
        torch.cuda.synchronize()
        arena.check(f"{name}/{form} encode")
        data, status, nbits = enc.data.cpu().numpy(), enc.status.cpu().numpy(), enc.nbits.cpu().numpy()
        assert status.tolist() == [0, ST_CAPACITY, 0, ST_CAPACITY, 0], form
        assert nbits.tolist() == [nb for _, nb in expected], form  # what the stream needs, whole, also when it did not fit
        for c in (0, 2, 4):
            assert np.array_equal(stream_bits(data, 8 * c * stride, expected[c][1]), expected[c][0]), (form, c)
        # the full slots decode to exactly out_cap symbols with no bit left: status 0, not CAPACITY
        rows, out = arena_decoded(arena, 5, 336, stride // 4)
        t.model.decode_batch(enc.data, enc.bit_offset, enc.nbits, stride // 4, out=out, any_parameter_kernels=any_par)
        torch.cuda.synchronize()
        arena.check(f"{name}/{form} decode")
        dsym, dlens, used, dstatus = (x.cpu().numpy() for x in out)
        for c in (0, 2, 4):
            want = t.decode(data, 8 * c * stride, expected[c][1], stride // 4)
            assert (int(dlens[c]), int(used[c]), int(dstatus[c])) == want[1:] == (len(chunks[c]), expected[c][1], 0)
            assert np.array_equal(dsym[c, :dlens[c]], chunks[c]), (form, c)


# ---- one block through the grid-wide kernels ----------------------------------------------------------------------------------
def check_block_encode(t, sym, what):
    dev = device()
    want, want_bits = t.encode(sym)
    nbytes = (want_bits + 7) // 8
    for cap in sorted({nbytes, (nbytes + 3) // 4 * 4 + 8}):  # exactly the stream's bytes, and room to spare
        arena = Arena(cap + 4 * GUARD, dev)
        out = arena.take(max(cap, 1), align=4)
        out.fill_(0x3C)  # the call zeroes what it ORs into
        meta = t.model.encode_block_into(sym_tensor(t, sym, dev), out, out_cap_bytes=cap)
        torch.cuda.synchronize()
        arena.check(f"{what}/cap{cap}")
        nbits, status = (int(v) for v in meta.cpu())
        assert (nbits, status & 0xFFFFFFFF) == (want_bits, 0), what
        assert np.array_equal(out.cpu().numpy()[:nbytes], want), f"{what}/cap{cap}: stream differs from the restatement"


@pytest.mark.parametrize("name", LIMIT_TABLES)
def test_block_encode_equals_the_restatement(name):
    t = table(name)
    rng = np.random.default_rng(t.K + 1)
    for n in (t.tile - 1, t.tile + 1, 3 * t.tile + 17):
        sym = t.mix(rng, n)
        if n > t.tile and name in WITH_32:
            # a 32-bit codeword behind 31 pending bits: the thread's 64-bit accumulator holds 63
            starts = np.cumsum(t.len[sym]) - t.len[sym]
            assert ((starts % 32 == 31) & (t.len[sym] == 32)).any()
        check_block_encode(t, sym, f"{name}/{n}")
    sym = t.back_to_back(t.tile + 1)
    assert (t.len[sym] == t.max_len).all()
    check_block_encode(t, sym, f"{name}/back to back")


@pytest.mark.parametrize("bit_offset", [0, 5, 107])
@pytest.mark.parametrize("name", LIMIT_TABLES)
def test_block_decode_equals_the_reference(name, bit_offset):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(2000 + bit_offset)
    streams = [t.mix_bits(rng, target) for target in (t.W - 1, t.W + 1, 3 * t.W + 77)]
    streams.append(t.back_to_back(t.tile + 1))  # with 32-bit codes exactly 4 W + 32 bits: every boundary is a true one
    for sym in streams:
        packed, nbits = t.encode(sym)
        data = place(packed, nbits, bit_offset, rng, dev)
        got = same_as_reference(t, data, bit_offset, nbits, len(sym), f"{name}/{nbits}@{bit_offset}")
        assert got[1:4] == (len(sym), nbits, 0) and np.array_equal(got[0], sym)


# ---- a stream cut inside its last codeword, at and around the width of the lookup table ------------------------------------------
def cut_cases(t):
    """[(symbol, bits of its codeword that remain)]: a 32-bit and a 12-bit last codeword where the table has one"""
    cases = []
    if t.max_len == 32:
        cases += [(int(t.longest[-1]), left) for left in (1, 10, 11, 12, 31)]
    if (t.len == 12).any():
        cases += [(int(np.nonzero(t.len == 12)[0][0]), left) for left in (1, 10, 11)]
    return cases


@pytest.mark.parametrize("name", ["comb12", "comb32", "deep512", "deep513"])
def test_cut_codeword_in_the_one_lane_decoders(name):
    """whatever lies behind the stream chose the table entry: the bits behind the cut are the codeword's own, zeros, ones"""
    t = table(name)
    rng = np.random.default_rng(12)
    head = t.mix(rng, 40)
    streams, derived = [], []
    for last, left in cut_cases(t):
        sym = np.concatenate([head, [last]])
        packed, nbits = t.encode(sym)
        start = nbits - int(t.len[last])
        bits = np.unpackbits(packed)[:nbits]
        for behind in (None, 0, 1):
            b = np.concatenate([bits, np.ones(64, np.uint8)])
            if behind is not None:
                b[start + left:] = behind
            streams.append((np.packbits(b), start + left))
            derived.append((40, start, ST_TRUNCATED))
    assert len(streams) >= 9
    wants = batch_same_as_reference(t, streams, 48, f"{name}/cut")
    for want, d in zip(wants, derived):
        assert want[1:] == d and np.array_equal(want[0], head)


@pytest.mark.parametrize("name", ["comb12", "comb32", "deep512", "deep513"])
def test_cut_codeword_in_the_block_decoder(name):
    """the cut codeword lies across a subsequence boundary, and across a workgroup boundary"""
    dev = device()
    t = table(name)
    rng = np.random.default_rng(13)
    shortest = int(np.argmin(t.len))
    for boundary in (5 * t.S, t.W):
        head = t.mix_bits(rng, boundary - 64)
        head = head[:-1]  # ends below boundary - 64; the shortest code (1 or 2 bits) fills up to 6 or 5 bits before it
        pad = (boundary - 5 - int(t.len[head].sum())) // t.min_len
        head = np.concatenate([head, np.full(pad, shortest)])
        for last, left in cut_cases(t):
            sym = np.concatenate([head, [last]])
            packed, nbits = t.encode(sym)
            start = nbits - int(t.len[last])
            assert start < boundary < nbits and boundary - start in (5, 6)
            for bit_offset in (0, 5):
                for behind in (0, 1):
                    data = place(packed, start + left, bit_offset, behind, dev)
                    got = same_as_reference(t, data, bit_offset, start + left, len(sym),
                                            f"{name}/cut {left} of {t.len[last]} at {boundary}@{bit_offset}/{behind}")
                    assert got[1:4] == (len(head), start, ST_TRUNCATED) and np.array_equal(got[0], head)


# ---- damage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["comb32", "deep512"])
def test_damaged_streams_equal_the_reference(name):
    """64 single-bit flips and 8 buffers of random bytes: every form gives what decode_reference gives, the block decoder too"""
    dev = device()
    t = table(name)
    rng = np.random.default_rng(32)
    sym = t.mix_bits(rng, 2 * t.W + 50)
    packed, nbits = t.encode(sym)
    assert nbits > 2 * t.W
    cap = nbits // t.min_len + 4
    streams = []
    for bit in rng.integers(0, nbits, 64):
        flipped = packed.copy()
        flipped[int(bit) >> 3] ^= 0x80 >> (int(bit) & 7)
        streams.append((flipped, nbits))
    streams += [(rng.integers(0, 256, packed.size, dtype=np.uint8), nbits) for _ in range(8)]
    wants = batch_same_as_reference(t, streams, cap, f"{name}/damage")
    statuses = {w[3] for w in wants}
    print(f"{name}: statuses met {sorted(statuses)}")
    assert statuses <= {0, ST_TRUNCATED, ST_STATE}
    if name == "deep512":
        assert ST_STATE in statuses  # the incomplete tree meets a missing child
    else:
        assert ST_STATE not in statuses  # a complete tree has none
    for i, ((d, nb), want) in enumerate(zip(streams, wants)):
        data = place(d, nb, 0, rng, dev)
        got = block_decode(t, data, 0, nb, cap, f"{name}/damage {i}")
        assert got[1:4] == want[1:], f"{name}/damage {i}: block decoder {got[1:4]}, the reference {want[1:]}"
        assert np.array_equal(got[0], want[0]), f"{name}/damage {i}: symbols differ"


# ---- scans of more than 1024 entries --------------------------------------------------------------------------------------------
class LargeBlock:
    """one block of the golden random17 table over more than 1024 encoder tiles and more than 1030 decoder workgroups"""

    def __init__(self):
        self.t = t = block_table("random17")
        mean = float((t.probs * t.len).sum())
        n = max(int(1032 * t.W / mean), 1025 * t.tile)
        self.sym = t.draw(np.random.default_rng(1024), n)
        self.packed, self.nbits = encode_vectorised(t.code, t.len, self.sym)
        self.ends = np.cumsum(t.len[self.sym])
        self.starts = self.ends - t.len[self.sym]
        self.n_tiles = -(-n // t.tile)
        self.n_groups = -(-self.nbits // t.W)
        assert self.n_tiles > 1024 and self.n_groups > 1030, (self.n_tiles, self.n_groups)
        assert self.nbits == int(self.ends[-1]) < 1 << 32
        dev = device()
        tail = np.random.default_rng(1).integers(0, 256, 16 + (-self.packed.size) % 16, dtype=np.uint8)
        self.data = torch.from_numpy(np.concatenate([self.packed, tail])).to(dev)
        self.d_sym = sym_tensor(t, self.sym, dev)

    def tail_reference(self, group, nbits, cap):
        """decode_reference from the first codeword that starts in workgroup `group`, plus what lies in front of it
        -> (n_out, consumed, status, j, symbols from j on)"""
        j = int(np.searchsorted(self.starts, group * self.t.W))
        first = int(self.starts[j])
        assert group * self.t.W <= first < group * self.t.W + self.t.max_len and cap >= j
        sym, consumed, status = decode_reference(self.t.code, self.t.len, self.packed, first, nbits - first, cap - j)
        return j + len(sym), first + consumed, status, j, sym


@functools.lru_cache(maxsize=None)
def large_block():
    return LargeBlock()


def test_large_block_encode_scans_more_than_1024_tiles():
    b = large_block()
    dev = device()
    nbytes = (b.nbits + 7) // 8
    odd = nbytes + 1 if (nbytes + 1) % 4 else nbytes + 2
    assert odd % 4 != 0 and b.n_tiles > 1024
    arena = Arena(2 * (nbytes + 8) + 8 * GUARD, dev)
    want = b.data[:nbytes]
    for cap in (nbytes, odd):
        out = arena.take(cap, align=4)
        out.fill_(0x3C)
        meta = b.t.model.encode_block_into(b.d_sym, out, out_cap_bytes=cap)
        torch.cuda.synchronize()
        nbits, status = (int(v) for v in meta.cpu())
        assert (nbits, status & 0xFFFFFFFF) == (b.nbits, 0), cap
        assert torch.equal(out[:nbytes], want), f"cap {cap}: stream differs from the restatement"
        assert (out[nbytes:] == 0).all()  # zeroed, nothing ORed in behind the stream
    arena.check("large encode")


def large_decode(b, nbits, cap, what):
    """-> (n_out, consumed, status) and the symbols on the device; the output lies between guard bands"""
    arena = Arena(max(cap, 1) + 4 * GUARD, b.data.device)
    out = arena.take(max(cap, 1))
    sym, n_out, consumed, status, _ = b.t.model.decode_block_device(b.data, nbits, 0, out_cap=cap, out=out)
    torch.cuda.synchronize()
    arena.check(what)
    assert n_out <= cap and (out[n_out:] == FILL).all(), f"{what}: symbols stored behind n_out"
    return (n_out, consumed, status), out[:n_out]


def test_large_block_decode_scans_more_than_1024_workgroups():
    b = large_block()
    assert b.n_groups > 1030
    got, sym = large_decode(b, b.nbits, len(b.sym), "large decode")
    assert got == (len(b.sym), b.nbits, 0)
    assert torch.equal(sym, b.d_sym)


def test_large_block_cut_in_workgroup_1029():
    """the stream ends inside a codeword that starts in workgroup 1029: thread 5 of the search for the first cut finds it
    in its second turn (5 + 1024), and every count in front of it comes through the carried scan"""
    b = large_block()
    t = b.t
    k = int(np.searchsorted(b.starts, 1029 * t.W + t.W // 2))
    k += int(np.argmax(t.len[b.sym[k:k + 1000]] >= 2))  # the next codeword that a cut can fall into
    cut = int(b.starts[k]) + 1
    assert t.len[b.sym[k]] >= 2 and cut // t.W == 1029 and -(-cut // t.W) == 1030
    n_out, consumed, status, j, tail = b.tail_reference(1029, cut, len(b.sym))
    assert (n_out, consumed, status) == (k, int(b.starts[k]), ST_TRUNCATED) and np.array_equal(tail, b.sym[j:k])
    got, sym = large_decode(b, cut, len(b.sym), "large cut")
    assert got == (k, int(b.starts[k]), ST_TRUNCATED)
    assert torch.equal(sym, b.d_sym[:k])


@pytest.mark.parametrize("group", [1025, 3])
def test_large_block_out_cap_ends_inside_a_workgroup(group):
    b = large_block()
    t = b.t
    cap = int(np.searchsorted(b.starts, group * t.W + t.W // 2))  # codeword `cap` starts in the middle of the workgroup
    assert int(b.ends[cap - 1]) // t.W == group and int(b.starts[cap]) // t.W == group
    n_out, consumed, status, j, tail = b.tail_reference(group, b.nbits, cap)
    assert (n_out, consumed, status) == (cap, int(b.ends[cap - 1]), ST_CAPACITY) and np.array_equal(tail, b.sym[j:cap])
    got, sym = large_decode(b, b.nbits, cap, f"large cap in {group}")
    assert got == (cap, int(b.ends[cap - 1]), ST_CAPACITY)
    assert torch.equal(sym, b.d_sym[:cap])


# ---- the number of correction passes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [4, 9])
def test_never_synchronising_code_takes_one_pass_per_workgroup(n_groups):
    """[0] + [1] * n with {0: "0", 1: "11", 2: "101", 3: "100"}: one 0 bit, then ones.  Every true boundary is odd.  W is
    even, so every guess of pass 0 is even, and a walk from an even bit reads "11" to the next even bit for ever: pass 0
    leaves workgroup 0 (whose first thread starts at bit 0, the truth) on odd starts and every other one on even starts
    that agree with each other.  Pass p reads the exits of pass p - 1.  Workgroup p finds its left neighbour's exit odd and
    moves; workgroup p + 1 reads the even exit its left neighbour still had in pass p - 1, which is its own start, and
    stands, as does every workgroup behind it.  So passes 1 .. n_groups - 1 each move exactly one workgroup:
    sync_passes == n_groups - 1."""
    dev = device()
    t = block_table("never")
    n = (n_groups * t.W - t.W // 2) // 2
    sym = np.concatenate([[0], np.ones(n, np.int64)])
    packed, nbits = encode_vectorised(t.code, t.len, sym)
    assert t.W % 2 == 0 and (n_groups - 1) * t.W < nbits <= n_groups * t.W and nbits == 2 * n + 1
    data = place(packed, nbits, 0, np.random.default_rng(5), dev)
    got = block_decode(t, data, 0, nbits, len(sym), f"never/{n_groups}")
    want = decode_reference(t.code, t.len, packed, 0, nbits, len(sym))
    assert got[1:4] == (len(want[0]), want[1], want[2]) == (len(sym), nbits, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], sym)
    assert got[4] == n_groups - 1


def test_fixed_length_code_takes_no_pass_at_9_workgroups():
    """all codes 3 bits: the guesses, rounded up to a multiple of 3, are the boundaries"""
    dev = device()
    t = block_table("fixed3")
    rng = np.random.default_rng(9)
    sym = t.draw(rng, 9 * t.W // 3)
    packed, nbits = encode_vectorised(t.code, t.len, sym)
    assert nbits == 9 * t.W
    data = place(packed, nbits, 0, rng, dev)
    got = block_decode(t, data, 0, nbits, len(sym), "fixed3/9")
    want = decode_reference(t.code, t.len, packed, 0, nbits, len(sym))
    assert got[1:4] == (len(want[0]), want[1], want[2]) == (len(sym), nbits, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], sym)
    assert got[4] == 0
