"""GPU: one large prefix-code block coded by the whole grid (csrc/scl_prefix_block.hip).

Yardsticks, never the code under test: the numpy restatement of the stream (prefix_helpers.encode_numpy) and the one-lane
kernels of csrc/scl_prefix.hip, which the reference's goldens pin (test_gpu_prefix.py) -- reached through
encode_batch / decode_batch with one chunk, or through the classes with BLOCK_PARALLEL_MIN raised on the instance.
Sizes are in units of the geometry the library reports: W = 256 * sub_bits bits per decoder workgroup, tile_symbols per
encoder tile."""
import numpy as np
import pytest

from prefix_helpers import code_bits, deep_chains, encode_numpy, goldens, make_dist, stream_bits, table_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5
ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED, ST_STATE = 0x1, 0x2, 0x4, 0x8
NEVER = 1 << 62  # a BLOCK_PARALLEL_MIN no block reaches: the one-lane path


def device():
    from stanford_compression_library_amd.backend import lib

    lib.require_device()
    return torch.device("cuda:0")


# ---- tables -----------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, name, code, length, probs):
        from stanford_compression_library_amd.backend.models import PrefixModel

        self.name, self.code, self.len = name, np.asarray(code, np.int64), np.asarray(length, np.int64)
        self.K, self.max_len, self.min_len = len(self.code), int(self.len.max()), int(self.len.min())
        self.probs = np.asarray(probs, np.float64) / np.sum(probs)
        self.bits_of = [np.array([(int(c) >> (int(n) - 1 - j)) & 1 for j in range(int(n))], np.uint8)
                        for c, n in zip(self.code, self.len)]
        self.model = PrefixModel(self.code, self.len)
        info = self.model.block_info()
        self.S, self.tile, self.gcd = int(info.sub_bits), int(info.tile_symbols), int(info.code_len_gcd)
        self.W = 256 * self.S
        assert self.S >= 32 and self.S % 32 == 0 and self.tile >= 256
        assert self.gcd == int(np.gcd.reduce(self.len))

    def draw(self, rng, n):
        return rng.choice(self.K, size=int(n), p=self.probs).astype(np.int64)

    def draw_bits(self, rng, target):
        """symbols from the table's distribution whose stream is as near to `target` bits as the table can come"""
        sym = self.draw(rng, target // self.min_len + 2)
        cum = np.cumsum(self.len[sym])
        n = int(np.argmin(np.abs(cum - target))) + 1
        assert abs(int(cum[n - 1]) - target) <= self.max_len
        return sym[:n]


_tables = {}


def table(name):
    device()
    if name not in _tables:
        if name in ("random17", "random256", "skewed28", "one_symbol", "random300"):
            case = table_case(name)
            _tables[name] = Table(name, case.arr("code"), case.arr("len"), case.arr("probs"))
            assert [b.tolist() for b in _tables[name].bits_of] == [b.tolist() for b in code_bits(case)]
        elif name == "incomplete":  # the golden random17 code without three of its symbols: walks can meet a missing child
            case = table_case("random17")
            keep = [s for s in range(case.K) if s not in (2, 9, 16)]
            _tables[name] = Table(name, case.arr("code")[keep], case.arr("len")[keep], case.arr("probs")[keep])
        elif name == "deep512":  # the incomplete 256-symbol table of test_gpu_prefix_limits.py, lengths 2 .. 32
            code, length = deep_chains(512)
            _tables[name] = Table(name, code, length, 2.0 ** -length.astype(np.float64))
        elif name == "fixed3":  # 8 symbols, all 3 bits: every guess is exact
            _tables[name] = Table(name, np.arange(8), np.full(8, 3), np.ones(8))
        elif name == "never":  # {0: "0", 1: "11", 2: "101", 3: "100"}
            _tables[name] = Table(name, [0b0, 0b11, 0b101, 0b100], [1, 2, 3, 3], [4, 2, 1, 1])
    return _tables[name]


TABLES = ["random17", "skewed28", "one_symbol", "incomplete"]


# ---- buffers between guard bands (the pattern of test_gpu_prefix.py) ------------------------------------------------------------
class Arena:
    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes + 16 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.pos = GUARD
        self.used = []

    def take(self, nbytes, dtype=torch.uint8, align=256):
        start = (self.pos + align - 1) // align * align
        self.used.append((start, start + nbytes))
        self.pos = start + nbytes + GUARD
        assert self.pos + GUARD <= self.buf.numel()
        return self.buf[start:start + nbytes].view(dtype)

    def check(self, what):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for a, b in self.used:
            mask[a:b] = False
        bad = ((self.buf != FILL) & mask).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} guard bytes overwritten, first at arena offset {int(bad[0])}"


def sym_tensor(t, sym, dev):
    host = np.ascontiguousarray(sym, dtype=t.model.sym_dtype)
    if t.model.wide:
        return torch.from_numpy(host.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(host).to(dev)


# ---- the yardstick: the one-lane kernels, one chunk -----------------------------------------------------------------------------
def one_lane_encode(t, sym, dev):
    """-> (packed bytes, nbits, status) of a batch of one chunk"""
    n = len(sym)
    row = np.zeros((1, max((n + 15) // 16 * 16, 16)), t.model.sym_dtype)
    row[0, :n] = sym
    d = torch.from_numpy(row.view(np.int16) if t.model.wide else row).to(dev)
    d = d.view(torch.uint16) if t.model.wide else d
    enc = t.model.encode_batch(d, torch.tensor([n], dtype=torch.int32, device=dev), out_stride=t.model.slot_bytes(n))
    nbits = int(enc.nbits[0]) & 0xFFFFFFFF
    return stream_bits(enc.data.cpu().numpy(), 0, nbits), nbits, int(enc.status[0])


def one_lane_decode(t, data, bit_offset, nbits, cap):
    """-> (symbols, n_out, consumed, status) of a batch of one chunk"""
    dev = data.device
    width = (cap + 15) // 16 * 16 + 16
    dtype = torch.uint16 if t.model.wide else torch.uint8
    out = (torch.zeros((1, width), dtype=torch.int16 if t.model.wide else torch.uint8, device=dev).view(dtype),
           torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
           torch.zeros(1, dtype=torch.int32, device=dev))
    sym, lens, used, status = t.model.decode_batch(data, torch.tensor([bit_offset], dtype=torch.int64, device=dev),
                                                   torch.tensor([nbits], dtype=torch.int32, device=dev), cap, out=out)
    n = int(lens[0])
    host = out[0].cpu().view(torch.int16 if t.model.wide else torch.uint8).numpy().view(t.model.sym_dtype)
    return host[0, :n].astype(np.int64), n, int(used[0]) & 0xFFFFFFFF, int(status[0])


def block_decode(t, data, bit_offset, nbits, cap, what):
    """the code under test, its output between guard bands -> (symbols, n_out, consumed, status, sync_passes)"""
    item = 2 if t.model.wide else 1
    arena = Arena(max(cap, 1) * item + 4 * GUARD, data.device)
    out = arena.take(max(cap, 1) * item, torch.uint16 if t.model.wide else torch.uint8)
    sym, n_out, consumed, status, passes = t.model.decode_block_device(data, nbits, bit_offset, out_cap=cap, out=out)
    torch.cuda.synchronize()
    arena.check(what)
    assert n_out <= cap, what
    raw = out.view(torch.uint8).cpu().numpy()
    assert (raw[n_out * item:] == FILL).all(), f"{what}: symbols stored behind n_out"
    host = raw[:n_out * item].view(t.model.sym_dtype).astype(np.int64)
    return host, n_out, consumed, status, passes


def same_as_one_lane(t, data, bit_offset, nbits, cap, what):
    got = block_decode(t, data, bit_offset, nbits, cap, what)
    want = one_lane_decode(t, data, bit_offset, nbits, cap)
    assert got[1:4] == want[1:4], f"{what}: (n_out, consumed, status) {got[1:4]}, the one-lane decoder {want[1:4]}"
    assert np.array_equal(got[0], want[0]), f"{what}: symbols differ"
    return got


def place(packed, nbits, bit_offset, rng, dev, tail=64):
    """a device buffer with the stream at `bit_offset`, random bits in front of it and behind it"""
    bits = np.unpackbits(np.asarray(packed, np.uint8))[:nbits]
    total = (bit_offset + nbits + 7) // 8 + tail
    total = (total + 15) // 16 * 16
    all_bits = rng.integers(0, 2, 8 * total).astype(np.uint8)
    all_bits[bit_offset:bit_offset + nbits] = bits
    return torch.from_numpy(np.packbits(all_bits)).to(dev)


# ---- 1. encode equals both yardsticks -----------------------------------------------------------------------------------------
def check_encode(t, sym, what):
    dev = device()
    want, want_bits = encode_numpy(t.bits_of, sym)
    lane, lane_bits, lane_status = one_lane_encode(t, sym, dev)
    assert lane_status == 0 and lane_bits == want_bits and np.array_equal(lane, want), f"{what}: the yardsticks disagree"
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
        got = out.cpu().numpy()
        assert np.array_equal(got[:nbytes], want), f"{what}/cap{cap}: stream differs from the restatement"
    data, nb = t.model.encode_block_device(sym_tensor(t, sym, dev))
    assert nb == want_bits and np.array_equal(data.cpu().numpy(), want), what


def block_sizes(t):
    return [0, 1, t.tile - 1, t.tile, t.tile + 1, 3 * t.tile + 17]


@pytest.mark.parametrize("name", TABLES)
def test_encode_equals_the_restatement_and_the_one_lane_kernel(name):
    t = table(name)
    rng = np.random.default_rng(t.K)
    for n in block_sizes(t):
        check_encode(t, t.draw(rng, n), f"{name}/{n}")


def test_encode_one_bit_codes_meet_in_one_word():
    """a block of the 1-bit code alone: 16 symbols a thread, 32 contributions to every word"""
    t = table("skewed28")
    shortest = int(np.argmin(t.len))
    assert t.len[shortest] == 1
    for n in (31, 2 * t.tile + 33):
        check_encode(t, np.full(n, shortest), f"one-bit/{n}")
    t = table("one_symbol")
    check_encode(t, np.zeros(t.tile + 5, np.int64), "one_symbol")


def test_encode_long_codes_straddle_the_tile_words():
    t = table("skewed28")
    assert t.max_len == 27
    rng = np.random.default_rng(27)
    rare = np.argsort(t.len)[::-1][:6]
    sym = rng.choice(rare, size=3 * t.tile + 17)
    mix = rng.random(sym.size) < 0.1
    sym[mix] = t.draw(rng, int(mix.sum()))
    check_encode(t, sym, "rare")
    check_encode(t, np.full(t.tile + 1, rare[0]), "rarest")


def test_encode_wide_alphabet():
    t = table("random300")
    assert t.model.wide
    rng = np.random.default_rng(300)
    for n in (1, t.tile + 1, 3 * t.tile + 17):
        check_encode(t, t.draw(rng, n), f"random300/{n}")


# ---- 2. encode statuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random17", "random300"])
def test_encode_symbol_outside_the_alphabet(name):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(2)
    sym = t.draw(rng, 2 * t.tile + 9)
    bad = sym.copy()
    where = [0, t.tile - 1, t.tile, 2 * t.tile + 8]
    bad[where] = [t.K, 255 if not t.model.wide else 65535, t.K + 1, t.K]
    sym[where] = 0  # what the stream codes there
    want, want_bits = encode_numpy(t.bits_of, sym)
    out = torch.empty(t.model.slot_bytes(len(sym)), dtype=torch.uint8, device=dev)
    nbits, status = (int(v) for v in t.model.encode_block_into(sym_tensor(t, bad, dev), out).cpu())
    assert (nbits, status & 0xFFFFFFFF) == (want_bits, ST_SYMBOL)
    assert np.array_equal(out.cpu().numpy()[:(want_bits + 7) // 8], want)


@pytest.mark.parametrize("name", ["random17", "skewed28"])
def test_encode_capacity_one_byte_short(name):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(3)
    sym = t.draw(rng, 2 * t.tile + 100)
    _, want_bits = encode_numpy(t.bits_of, sym)
    cap = (want_bits + 7) // 8 - 1
    arena = Arena(cap + 4 * GUARD, dev)
    out = arena.take(cap, align=4)
    meta = t.model.encode_block_into(sym_tensor(t, sym, dev), out)
    torch.cuda.synchronize()
    arena.check("capacity")
    nbits, status = (int(v) for v in meta.cpu())
    assert (nbits, status & 0xFFFFFFFF) == (want_bits, ST_CAPACITY)  # the length it needs is still reported


@pytest.mark.parametrize("name", ["random17", "random300"])
def test_encode_symbol_outside_the_alphabet_and_capacity_at_once(name):
    """both faults are reported, with the length needed, and no codeword is stored: the output holds the zeros the call lays
    down (as far as the longest stream of n symbols reaches, the cap at the most) and the filler behind them"""
    dev = device()
    t = table(name)
    rng = np.random.default_rng(12)
    sym = t.draw(rng, 2 * t.tile + 9)
    bad = sym.copy()
    bad[2 * t.tile + 5] = t.K
    sym[2 * t.tile + 5] = 0  # what the stream codes there
    _, want_bits = encode_numpy(t.bits_of, sym)
    cap = (want_bits + 7) // 8 - 1
    zeroed = min(((len(sym) * t.max_len + 7) // 8 + 3) // 4 * 4, cap)
    arena = Arena(cap + 8 + 4 * GUARD, dev)
    out = arena.take(cap + 8, align=4)
    meta = t.model.encode_block_into(sym_tensor(t, bad, dev), out, out_cap_bytes=cap)
    torch.cuda.synchronize()
    arena.check(f"{name}/symbol+capacity")
    nbits, status = (int(v) for v in meta.cpu())
    assert (nbits, status & 0xFFFFFFFF) == (want_bits, ST_SYMBOL | ST_CAPACITY)
    raw = out.cpu().numpy()
    assert not raw[:zeroed].any() and (raw[zeroed:] == FILL).all()


def trimmed_to_byte_residues(ends, least):
    """-> {r: n} for r = 1, 2, 3: the largest n > ``least`` whose first n codewords end in a stream of r mod 4 bytes"""
    nbytes = (np.asarray(ends, np.int64) + 7) // 8
    found = {}
    for r in (1, 2, 3):
        hits = np.nonzero(nbytes[least:] % 4 == r)[0]
        assert hits.size, f"no prefix of {r} mod 4 bytes"
        found[r] = least + int(hits[-1]) + 1
    return found


@pytest.mark.parametrize("name", ["random17", "random300"])
def test_exact_fit_through_the_tail_word(name):
    """out_cap_bytes = the stream's bytes, 1, 2 and 3 mod 4: the last word reaches the output through the tail kernel, byte
    by byte, and the byte behind the cap stays; the decoder then reads the same bytes with in_size_bytes cutting its last
    word (the byte-wise tail of its window)"""
    dev = device()
    t = table(name)
    rng = np.random.default_rng(13)
    sym = t.draw(rng, 2 * t.tile + 40)
    for r, n in trimmed_to_byte_residues(np.cumsum(t.len[sym]), 2 * t.tile).items():
        want, want_bits = encode_numpy(t.bits_of, sym[:n])
        cap = (want_bits + 7) // 8
        assert cap % 4 == r and want.size == cap
        arena = Arena(cap + 4 * GUARD, dev)
        out = arena.take(cap, align=4)  # the guard starts at the byte behind the cap
        out.fill_(0x3C)
        meta = t.model.encode_block_into(sym_tensor(t, sym[:n], dev), out, out_cap_bytes=cap)
        torch.cuda.synchronize()
        arena.check(f"{name}/fit{r}")
        nbits, status = (int(v) for v in meta.cpu())
        assert (nbits, status & 0xFFFFFFFF) == (want_bits, 0)
        assert np.array_equal(out.cpu().numpy(), want)
        assert out.numel() == cap
        got = block_decode(t, out, 0, want_bits, n, f"{name}/fit{r}/decode")
        assert got[1:4] == (n, want_bits, 0) and np.array_equal(got[0], sym[:n])


# ---- 3. decode equals the one-lane decoder --------------------------------------------------------------------------------------
def decode_targets(t):
    return [1, t.W - 1, t.W, t.W + 1, 3 * t.W + 77]


@pytest.mark.parametrize("bit_offset", [0, 5, 8 * 13 + 3])
@pytest.mark.parametrize("name", TABLES)
def test_decode_equals_the_one_lane_decoder(name, bit_offset):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(1000 + bit_offset)
    used = []
    for target in decode_targets(t):
        sym = t.draw_bits(rng, target)
        packed, nbits = encode_numpy(t.bits_of, sym)
        used.append(nbits)
        data = place(packed, nbits, bit_offset, rng, dev)
        got = same_as_one_lane(t, data, bit_offset, nbits, nbits // t.min_len, f"{name}/{target}@{bit_offset}")
        assert got[1:4] == (len(sym), nbits, 0) and np.array_equal(got[0], sym)
    print(f"{name}: stream lengths used {used} for targets {decode_targets(t)}")
    assert used[0] <= t.max_len and abs(used[2] - t.W) <= t.max_len and used[4] > 3 * t.W


def test_decode_empty_stream():
    dev = device()
    t = table("random17")
    data = torch.full((64,), 0xFF, dtype=torch.uint8, device=dev)
    got = block_decode(t, data, 7, 0, 0, "empty")
    assert got[1:] == (0, 0, 0, 0)
    got = block_decode(t, data, 7, 0, 10, "empty")
    assert got[1:] == (0, 0, 0, 0)


def test_decode_long_codes_across_subsequences_and_workgroups():
    """the 27-bit table, mostly its rarest symbols: nearly every subsequence boundary, and the workgroup boundaries,
    fall inside a codeword, and the decoder walks the tree below its lookup table"""
    dev = device()
    t = table("skewed28")
    rare = np.argsort(t.len)[::-1][:6]
    for seed in range(28, 60):  # the first seed whose stream has a codeword across each workgroup boundary
        rng = np.random.default_rng(seed)
        sym = rng.choice(rare, size=2 * t.W // 12)  # 85 % of them have 23 bits and more: well over 2 W bits
        mix = rng.random(sym.size) < 0.15
        sym[mix] = t.draw(rng, int(mix.sum()))
        ends = np.cumsum(t.len[sym])
        sym = sym[:int(np.searchsorted(ends, 2 * t.W + 50)) + 1]  # the first prefix of at least 2 W + 50 bits
        ends = set(ends[:sym.size].tolist())
        if t.W not in ends and 2 * t.W not in ends:
            break
    n = sym.size
    packed, nbits = encode_numpy(t.bits_of, sym)
    assert nbits >= 2 * t.W + 50 and t.W not in ends and 2 * t.W not in ends
    for bit_offset in (0, 5):
        data = place(packed, nbits, bit_offset, rng, dev)
        got = same_as_one_lane(t, data, bit_offset, nbits, n, f"rare@{bit_offset}")
        assert got[1:4] == (n, nbits, 0) and np.array_equal(got[0], sym)


def test_decode_wide_alphabet():
    dev = device()
    t = table("random300")
    rng = np.random.default_rng(301)
    for target in (1, t.W + 1, 3 * t.W + 77):
        sym = t.draw_bits(rng, target)
        packed, nbits = encode_numpy(t.bits_of, sym)
        data = place(packed, nbits, 5, rng, dev)
        got = same_as_one_lane(t, data, 5, nbits, len(sym) + 3, f"random300/{target}")
        assert got[1:4] == (len(sym), nbits, 0) and np.array_equal(got[0], sym)


# ---- 4. synchronisation ---------------------------------------------------------------------------------------------------------
def test_sync_fixed_length_code_needs_no_correction():
    dev = device()
    t = table("fixed3")
    assert t.gcd == 3
    rng = np.random.default_rng(4)
    sym = t.draw(rng, 3 * t.W // 3)
    packed, nbits = encode_numpy(t.bits_of, sym)
    assert nbits == 3 * t.W
    data = place(packed, nbits, 0, rng, dev)
    got = same_as_one_lane(t, data, 0, nbits, len(sym), "fixed3")
    assert got[1:] == (len(sym), nbits, 0, 0) and np.array_equal(got[0], sym)


def test_sync_code_that_never_falls_into_step():
    """[0] + [1] * n with {0: "0", 1: "11", ...}: every true boundary is odd, every guess even, and a walk from an even
    bit reads "11" for ever -- one correction pass per workgroup, and the loop ends"""
    dev = device()
    t = table("never")
    n = (4 * t.W - t.W // 2) // 2
    sym = np.concatenate([[0], np.ones(n, np.int64)])
    packed, nbits = encode_numpy(t.bits_of, sym)
    assert 3 * t.W < nbits <= 4 * t.W
    rng = np.random.default_rng(5)
    data = place(packed, nbits, 0, rng, dev)
    got = same_as_one_lane(t, data, 0, nbits, len(sym), "never")
    assert got[1:4] == (len(sym), nbits, 0) and np.array_equal(got[0], sym)
    print("never-synchronising stream over 4 workgroups: sync_passes =", got[4])
    assert got[4] >= 2


def test_sync_typical_huffman_table():
    dev = device()
    t = table("random256")
    rng = np.random.default_rng(6)
    sym = t.draw_bits(rng, 4 * t.W - 100)
    packed, nbits = encode_numpy(t.bits_of, sym)
    assert 3 * t.W < nbits <= 4 * t.W
    data = place(packed, nbits, 0, rng, dev)
    got = same_as_one_lane(t, data, 0, nbits, len(sym), "random256")
    assert got[1:4] == (len(sym), nbits, 0) and np.array_equal(got[0], sym)
    print("random256 over 4 workgroups: sync_passes =", got[4])


# ---- 5. damaged streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random17", "incomplete", "one_symbol"])
def test_damaged_streams_equal_the_one_lane_decoder(name):
    dev = device()
    t = table(name)
    rng = np.random.default_rng(50)
    sym = t.draw_bits(rng, 2 * t.W + 50)
    # a codeword lies across the first workgroup boundary where the code has one long enough
    ends = np.cumsum(t.len[sym])
    starts = ends - t.len[sym]
    if t.max_len > 1:
        k = int(np.searchsorted(ends, t.W))
        if not starts[k] < t.W < ends[k]:
            longest = int(np.argmax(t.len))
            sym[k] = longest
            ends = np.cumsum(t.len[sym])
            starts = ends - t.len[sym]
            k = int(np.searchsorted(ends, t.W))
        assert starts[k] < t.W < ends[k], "no codeword across the workgroup boundary"
    packed, nbits = encode_numpy(t.bits_of, sym)
    n = len(sym)
    assert nbits == int(ends[-1]) and 2 * t.W < nbits
    cap = nbits // t.min_len + 4
    data = place(packed, nbits, 0, rng, dev)
    host = data.cpu().numpy()
    statuses = set()

    def compare(d, nb, c, what):
        got = same_as_one_lane(t, d, 0, nb, c, f"{name}/{what}")
        statuses.add(got[3])
        return got

    got = compare(data, nbits, cap, "intact")
    assert got[1:4] == (n, nbits, 0)
    # cut inside the last codeword, and inside the codeword across the workgroup boundary
    if t.max_len > 1:
        last = int(np.nonzero(t.len[sym] >= 2)[0][-1])
        for j, label in ((last, "cut-last"), (k, "cut-boundary")):
            for cut_at in sorted({int(starts[j]) + 1, int(ends[j]) - 1} | ({t.W} if j == k else set())):
                got = compare(data, cut_at, cap, f"{label}@{cut_at}")
                if name != "incomplete":  # (an incomplete tree may meet a missing child before the cut)
                    assert got[1:4] == (j, int(starts[j]), ST_TRUNCATED), (label, cut_at, got[1:4])
    # 64 single-bit flips
    for bit in rng.integers(0, nbits, 64):
        flipped = host.copy()
        flipped[int(bit) >> 3] ^= 0x80 >> (int(bit) & 7)
        compare(torch.from_numpy(flipped).to(dev), nbits, cap, f"flip@{int(bit)}")
    # 8 buffers of random bytes
    for i in range(8):
        noise = torch.from_numpy(rng.integers(0, 256, host.size, dtype=np.uint8)).to(dev)
        compare(noise, nbits, cap, f"random{i}")
    # out_cap below the count
    for c in (n - 1, n // 2, 0):
        got = compare(data, nbits, c, f"cap{c}")
        assert got[1:4] == (c, int(ends[c - 1]) if c else 0, ST_CAPACITY) and np.array_equal(got[0], sym[:c])
    print(f"{name}: statuses met {sorted(statuses)}")
    assert ST_CAPACITY in statuses and 0 in statuses
    if name != "random17":
        assert ST_STATE in statuses  # a complete tree has no missing child
    if t.max_len > 1:
        assert ST_TRUNCATED in statuses


def test_host_decode_of_a_stream_that_ends_one_bit_into_a_word():
    """decode_block_host stages the stream in a padded device buffer; a stream of 1 mod 32 bits leaves three bytes between
    its end and the next word that the decoder's window loads.  Whatever they hold, the symbols, `consumed` and the error
    are those of the one-lane scl_prefix_decode_host -- as coded, and cut inside the last codeword.  An incomplete table:
    bits behind the stream could lead into a missing child."""
    import ctypes as C

    from stanford_compression_library_amd.backend import lib as _lib
    from stanford_compression_library_amd.backend.models import PrefixModel

    t = table("deep512")
    assert sum(2.0 ** -t.len.astype(np.float64)) < 1  # incomplete
    rng = np.random.default_rng(14)
    sym = t.draw(rng, 2 * PrefixModel.BLOCK_PARALLEL_MIN)
    ends = np.cumsum(t.len[sym])
    n = int(np.nonzero((ends % 32 == 1) & (t.len[sym] >= 2))[0][-1]) + 1  # the longest prefix of 1 mod 32 bits
    sym, ends = sym[:n], ends[:n]
    packed, nbits = encode_numpy(t.bits_of, sym)
    assert nbits % 32 == 1 and nbits - int(t.len[sym[-1]]) >= PrefixModel.BLOCK_PARALLEL_MIN * t.min_len

    def call(name, nb):
        out = np.zeros(nb // t.min_len, t.model.sym_dtype)
        n_out, used = C.c_uint64(0), C.c_uint64(0)
        rc = t.model._sym_fn(name)(t.model._h, _lib.u8_ptr(packed), nb, t.model._host_ptr(out), out.size, C.byref(n_out),
                                   C.byref(used))
        return rc, int(n_out.value), int(used.value), out[:n_out.value if rc == 0 else 0].astype(np.int64)

    for nb, want in ((nbits, (0, n, nbits)), (nbits - 1, (_lib.E_CHUNK, n - 1, int(ends[-2])))):
        block, lane = call("decode_block_host", nb), call("decode_host", nb)
        assert block[:3] == lane[:3] == want, (nb, block[:3], lane[:3], want)
        assert np.array_equal(block[3], lane[3]) and (block[0] or np.array_equal(block[3], sym))
        host, used = None, None
        try:
            host, used = t.model.decode_host(packed, nb)  # the path the classes take: the block call at this size
        except _lib.SclHipError as e:
            assert e.code == want[0] and "TRUNCATED" in str(e)
        if want[0] == 0:
            assert used == nbits and np.array_equal(host, sym)
        else:
            assert host is None


# ---- 6. 64-bit addressing ---------------------------------------------------------------------------------------------------------
def test_decode_at_a_bit_offset_above_2_to_32():
    """positions relative to the buffer are 64-bit: a stream at bit 2^32 + 5 of a 513 MiB buffer.  (Positions RELATIVE TO
    THE STREAM above 2^32 would need a stream of 512 MiB and more: 64-bit by construction, exercised by no test.)"""
    dev = device()
    t = table("random17")
    rng = np.random.default_rng(64)
    sym = t.draw(rng, 1000)
    packed, nbits = encode_numpy(t.bits_of, sym)
    small = place(packed, nbits, 5, np.random.default_rng(0), dev, tail=16)
    near = same_as_one_lane(t, small, 5, nbits, 1000, "offset 5")
    assert near[1:4] == (1000, nbits, 0) and np.array_equal(near[0], sym)
    try:
        big = torch.zeros(513 << 20, dtype=torch.uint8, device=dev)
    except RuntimeError as e:
        pytest.skip(f"no 513 MiB device allocation: {e}")
    bits = np.zeros(8 * ((nbits + 5 + 7) // 8), np.uint8)
    bits[5:5 + nbits] = np.unpackbits(packed)[:nbits]
    piece = np.packbits(bits)
    big[1 << 29:(1 << 29) + piece.size] = torch.from_numpy(piece).to(dev)
    far = block_decode(t, big, (1 << 32) + 5, nbits, 1000, "offset 2^32 + 5")
    assert far[1:4] == near[1:4] and np.array_equal(far[0], near[0])


# ---- 7. through the classes -----------------------------------------------------------------------------------------------------
def class_round_trip(dist, symbols):
    from stanford_compression_library_amd.backend.models import PrefixModel
    from stanford_compression_library_amd.compressors import HuffmanDecoder, HuffmanEncoder
    from stanford_compression_library_amd.core.data_block import DataBlock

    block = DataBlock(symbols)
    enc, dec, enc1, dec1 = HuffmanEncoder(dist), HuffmanDecoder(dist), HuffmanEncoder(dist), HuffmanDecoder(dist)
    assert "BLOCK_PARALLEL_MIN" not in vars(enc._device_model())  # the default threshold: the block path runs
    assert block.size >= PrefixModel.BLOCK_PARALLEL_MIN
    enc1._device_model().BLOCK_PARALLEL_MIN = NEVER
    dec1._device_model().BLOCK_PARALLEL_MIN = NEVER
    bits = enc.encode_block(block)
    assert bits == enc1.encode_block(block)
    assert len(bits) >= PrefixModel.BLOCK_PARALLEL_MIN * dec._device_model().min_len
    out, used = dec.decode_block(bits)
    out1, used1 = dec1.decode_block(bits)
    assert used == used1 == len(bits)
    assert out.data_list == out1.data_list == symbols


def test_huffman_classes_take_the_block_path():
    device()
    case = table_case("random256")
    rng = np.random.default_rng(7)
    symbols = rng.choice(case.K, size=300_000, p=case.arr("probs")).tolist()
    class_round_trip(make_dist(case), symbols)


def test_huffman_classes_wide_alphabet():
    from stanford_compression_library_amd.core.prob_dist import ProbabilityDist

    device()
    rng = np.random.default_rng(8)
    counts = rng.integers(50, 1050, 1000)
    probs = counts / counts.sum()
    dist = ProbabilityDist({i: float(p) for i, p in enumerate(probs)})
    symbols = rng.choice(1000, size=100_000, p=probs).tolist()
    class_round_trip(dist, symbols)


def test_huffman_files_with_large_blocks(tmp_path):
    from stanford_compression_library_amd.backend.models import PrefixModel
    from stanford_compression_library_amd.compressors import HuffmanDecoder, HuffmanEncoder
    from stanford_compression_library_amd.core.prob_dist import ProbabilityDist

    device()
    case = goldens()["file"][0]
    dist = ProbabilityDist({c: float(p) for c, p in zip(case.chars, case.arr("probs"))})
    rng = np.random.default_rng(9)
    text = "".join(rng.choice(list(case.chars), size=700_000, p=case.arr("probs")))
    assert len(text.encode("ascii")) == 700_000 and 250_000 >= PrefixModel.BLOCK_PARALLEL_MIN
    src, dst, dst1, back = (str(tmp_path / n) for n in ("in.txt", "out.bin", "out1.bin", "back.txt"))
    with open(src, "w", newline="") as f:
        f.write(text)
    HuffmanEncoder(dist).encode_file(src, dst, block_size=250_000)
    one_lane = HuffmanEncoder(dist)
    one_lane._device_model().BLOCK_PARALLEL_MIN = NEVER
    one_lane.encode_file(src, dst1, block_size=250_000)
    assert np.array_equal(np.fromfile(dst, np.uint8), np.fromfile(dst1, np.uint8))
    HuffmanDecoder(dist).decode_file(dst, back)
    assert open(back, newline="").read() == text
