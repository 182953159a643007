"""The wide LZ77 path on the GPU (csrc/scl_lz77_wide.hip): ONE stream parsed and replayed across the whole chip must store
what the one-wave batch kernels store for that stream, bit for bit, and both must equal the rule.

Every case of lz77_wide_helpers is a few tiles long and sits on an edge of the scheme: the cap of a scored extension (C), the
tile (T), the start of the block, the end of the window.  parse_wide is compared with lz77_helpers.parse_restated and with
parse_batch on the same stream (rows, n_seq, literals, n_lit, status), replay_wide with replay_restated and replay_batch
(bytes, out_len, status).  tests/test_lz77_wide_host.py checks on the host that every case has the edge it is named for."""
import numpy as np
import pytest

from lz77_helpers import ST_CAPACITY, markov1_long_stream, markov1_stream, replay_restated
from lz77_wide_helpers import _noise, all_cases, damage_cases, reference
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL, FILL = 0x5A5A5A5A, 0xC3
T, C = dev_lz77.wide_shape()
CASES = all_cases(T, C)
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def fresh_out(n, seq_cap, start, dev):
    """a one-stream ParsedBatch the caller owns: rows full of SENTINEL, literals full of FILL, the counts of -1"""
    rows = lambda: torch.full((1, seq_cap), SENTINEL, dtype=torch.int32, device=dev)  # noqa: E731
    words = lambda: torch.full((1,), -1, dtype=torch.int32, device=dev)  # noqa: E731
    return dev_lz77.ParsedBatch(rows(), rows(), rows(), torch.full((max(n, 1),), FILL, dtype=torch.uint8, device=dev), words(),
                                words(), words(), torch.full((1,), start, dtype=torch.int64, device=dev), int(seq_cap))


def unpack(res, start):
    """-> dict(rows [seq_cap, 3] as int64 of the uint32 values, n_seq, n_lit, status, literals = the whole buffer)"""
    torch.cuda.synchronize()
    rows = np.stack([t.cpu().numpy().view(np.uint32).astype(np.int64)[0]
                     for t in (res.literal_count, res.match_length, res.match_offset)], axis=1)
    n_seq, n_lit, status = (int(t.cpu().numpy().view(np.uint32)[0]) for t in (res.n_seq, res.n_lit, res.status))
    return dict(rows=rows, n_seq=n_seq, n_lit=n_lit, status=status, literals=res.literals.cpu().numpy(), start=start)


def parse_both(case, dev, seq_cap=None, scratch=None):
    """parse_wide and parse_batch of the case into buffers full of sentinels -> (wide, batch) as unpack() gives them"""
    w, start, L, M = case["window"], case["start"], case["L"], case["M"]
    n = len(w)
    cap = dev_lz77.default_seq_cap(n - start, L) if seq_cap is None else seq_cap
    win = torch.from_numpy(w).to(dev) if n else torch.zeros(0, dtype=torch.uint8, device=dev)
    wide = dev_lz77.parse_wide(win, start, L, M, scratch=scratch, out=fresh_out(n, cap, start, dev))
    win_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    start_t = torch.tensor([start], dtype=torch.int32, device=dev)
    batch = dev_lz77.parse_batch(win, win_off, start_t, L, M, cap, out=fresh_out(n, cap, start, dev))
    return unpack(wide, start), unpack(batch, start)


def assert_same_store(wide, batch, what):
    """everything the two calls own is equal, and neither stored anything else"""
    for key in ("n_seq", "n_lit", "status"):
        assert wide[key] == batch[key], f"{what}: {key} {wide[key]} != {batch[key]}"
    assert np.array_equal(wide["rows"], batch["rows"]), f"{what}: sequence rows (sentinels behind n_seq included)"
    assert np.array_equal(wide["literals"], batch["literals"]), f"{what}: literal bytes (fill outside [0, n_lit) included)"
    assert (wide["rows"][wide["n_seq"]:] == SENTINEL).all(), f"{what}: a row at or behind n_seq was stored"
    lit, a = wide["literals"], wide["start"]
    assert (lit[:a] == FILL).all() and (lit[a + wide["n_lit"]:] == FILL).all(), f"{what}: a literal outside [0, n_lit)"


def assert_is_the_rule(got, ref, what):
    seq, lit = ref
    assert got["status"] == 0 and got["n_seq"] == len(seq) and got["n_lit"] == len(lit), what
    assert got["rows"][: got["n_seq"]].tolist() == seq.tolist(), what
    assert got["literals"][got["start"]: got["start"] + got["n_lit"]].tolist() == lit.tolist(), what


def replay_both(history, seqs, literals, cap, dev):
    """replay_wide and replay_batch into slots of `cap` bytes inside a buffer full of FILL (16 guard bytes on either side)
    -> ((new bytes, out_len, status) of the wide call, of the batch call)"""
    hist, seqs = np.asarray(history, np.uint8), np.asarray(seqs, np.int64).reshape(-1, 3)
    have, n_seq, n_lit = len(hist), len(seqs), len(literals)
    rows = [torch.from_numpy(seqs[:, j].astype(np.uint32).view(np.int32).copy()).to(dev).reshape(1, -1) for j in range(3)]
    lit = torch.from_numpy(np.concatenate([np.asarray(literals, np.uint8), np.zeros(1, np.uint8)])).to(dev)
    out = []
    for wide in (True, False):
        buf = torch.full((cap + 32,), FILL, dtype=torch.uint8, device=dev)
        buf[16: 16 + have] = torch.from_numpy(hist).to(dev)
        slot = buf[16: 16 + cap]
        if wide:
            out_len, status = dev_lz77.replay_wide(slot, have, *rows, n_seq, lit, n_lit)
        else:
            win_off = torch.tensor([16, 16 + cap], dtype=torch.int64, device=dev)
            words = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)  # noqa: E731
            out_len, status = dev_lz77.replay_batch(buf, win_off, words(have), *rows, words(n_seq), lit,
                                                    torch.zeros(1, dtype=torch.int64, device=dev), words(n_lit))
        torch.cuda.synchronize()
        host, k = buf.cpu().numpy(), int(out_len[0])
        assert (host[:16] == FILL).all() and (host[16 + have + k:] == FILL).all(), "bytes outside [have, have + out_len)"
        assert host[16: 16 + have].tolist() == hist.tolist(), "the history was changed"
        out.append((host[16 + have: 16 + have + k], k, int(status[0])))
    return out


def assert_replay(history, seqs, literals, cap, dev, what):
    want, want_status = replay_restated(history, seqs, literals, cap)
    wide, batch = replay_both(history, seqs, literals, cap, dev)
    assert wide[2] == want_status == batch[2], f"{what}: status {wide[2]}, the rule {want_status}, one wave {batch[2]}"
    assert wide[1] == batch[1] == len(want), f"{what}: out_len {wide[1]}, one wave {batch[1]}, the rule {len(want)}"
    assert wide[0].tolist() == want.tolist() and batch[0].tolist() == want.tolist(), f"{what}: bytes"
    return want_status


# ---- every case: parse and replay ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_parse_and_replay_equal_the_rule_and_the_one_wave_kernels(case, dev):
    ref = reference(T, C)[case["name"]]
    wide, batch = parse_both(case, dev)
    assert_is_the_rule(wide, ref, case["name"])
    assert_same_store(wide, batch, case["name"])
    w, start = case["window"], case["start"]
    status = assert_replay(w[:start], ref[0], ref[1], len(w), dev, case["name"])
    assert status == 0


@pytest.mark.parametrize("name", ["markov-L6-M64", "markov-L1-M1", "rand4-L4-M64", "entry-is-long", "older" + str(C),
                                  "history-longer-than-block", "start" + str(T + 1)])
def test_one_sequence_too_few_is_capacity_as_on_one_wave(name, dev):
    case, (seq, lit) = BY_NAME[name], reference(T, C)[name]
    assert len(seq) >= 2
    wide, batch = parse_both(case, dev, seq_cap=len(seq) - 1)
    assert wide["status"] == ST_CAPACITY and wide["n_seq"] == len(seq) - 1
    assert wide["rows"][: wide["n_seq"]].tolist() == seq[:-1].tolist() and wide["n_lit"] == int(seq[:-1, 0].sum())
    assert_same_store(wide, batch, name)


def test_more_than_64_candidates_and_none_are_refused(dev):
    win = torch.zeros(4 * T, dtype=torch.uint8, device=dev)
    for M in (0, 65):
        with pytest.raises(backend_lib.SclHipError) as err:
            dev_lz77.parse_wide(win, 0, 6, M)
        assert err.value.code == backend_lib.E_PARAM and "1 <= M <= 64" in str(err.value)


# ---- replay on damaged sequences: validation outcomes ------------------------------------------------------------------------
def test_damaged_sequences_stop_where_and_how_the_one_wave_kernel_stops(dev):
    case = BY_NAME["markov-L6-M64"]
    seqs, lits = reference(T, C)[case["name"]]
    hist = np.arange(10, dtype=np.uint8)
    full = len(hist) + len(case["window"])
    seen = set()
    for name, bad, cap in damage_cases(seqs, lits, len(hist)):
        seen.add(assert_replay(hist, bad, lits, full if cap is None else cap, dev, name))
    assert 0 not in seen and len(seen) == 3


def test_the_deepest_copy_chains(dev):
    """L = 1, M = 1: every match copies the most recent occurrence of one byte, mostly a byte that was itself copied"""
    w = markov1_stream(6 * T + 5, 12)
    case = dict(name="deep", window=w, start=0, L=1, M=1)
    wide, batch = parse_both(case, dev)
    assert_same_store(wide, batch, "deep")
    seqs, lits = wide["rows"][: wide["n_seq"]], wide["literals"][: wide["n_lit"]]
    assert wide["status"] == 0 and wide["n_seq"] > len(w) // 8
    assert assert_replay(w[:0], seqs, lits, len(w), dev, "deep") == 0


# ---- the carries of the scans (csrc/scl_scan.h): 2048 entries a scan block, 256 entries a trip of one workgroup ----------------
SCAN_BLOCK, SCAN_TRIP = 2048, 256
NOISE_TILES = ((255, 258), (2047, 2049))  # first and last tile of the stretches without a match


def test_parse_across_the_carries_of_the_tile_scans(dev):
    """2050 tiles: the sum scans of the per-tile sequence counts and matched bytes span two scan blocks, the running maximum
    of the match ends takes nine trips.  The tiles on either side of trip border 256 and of scan block border 2048 have no
    sequence of their own (noise over the Markov source), so what the tiles behind a border see -- where their literals
    go, what the totals are -- can only be the carried prefix.  (There is no tile behind the second stretch: the window ends
    in it, so the literal run to the end of the block and entry n_tiles, the totals, are what reads the second carry.)"""
    n = (SCAN_BLOCK + 1) * T + 1
    w = markov1_long_stream(n, 17)
    rng = np.random.default_rng(44)
    for first, last in NOISE_TILES:
        w[first * T: (last + 1) * T] = _noise(rng, min((last + 1) * T, n) - first * T)
    case = dict(name="carries", window=w, start=0, L=6, M=64)
    wide, batch = parse_both(case, dev)
    assert wide["status"] == 0 and batch["status"] == 0
    assert_same_store(wide, batch, "carries")
    n_seq, n_lit = wide["n_seq"], wide["n_lit"]
    seqs, lits = wide["rows"][:n_seq], wide["literals"][:n_lit]
    # the fixture: sequences on either side of both borders, none in the noise
    assert n_seq > SCAN_BLOCK
    ends = np.cumsum(seqs[:, 0] + seqs[:, 1])
    tiles = (ends - seqs[:, 1]) // T  # the tile every sequence starts in
    (a0, a1), (b0, b1) = NOISE_TILES
    assert (tiles < SCAN_TRIP - 1).any() and ((tiles > a1) & (tiles < b0)).any()
    assert not ((tiles >= a0) & (tiles <= a1)).any() and not (tiles >= b0).any()
    assert n - int(ends[-1]) > (b1 - b0) * T and n_lit == n - int(seqs[:, 1].sum())
    (got, out_len, status), (one, one_len, one_status) = replay_both(w[:0], seqs, lits, n, dev)
    assert status == 0 and one_status == 0 and out_len == n and one_len == n
    assert np.array_equal(got, w) and np.array_equal(one, w)


def test_replay_across_the_carries_of_the_64_bit_scans(dev):
    """258 scan blocks of sequences: the one workgroup that scans the block sums of the two 64-bit position scans takes a
    second trip.  Every sequence is one literal and a match of 1..3 bytes at offset 1: the literal 2..4 times."""
    n_seq = SCAN_TRIP * SCAN_BLOCK + SCAN_BLOCK + 1
    lits = np.random.default_rng(45).integers(0, 256, n_seq).astype(np.uint8)
    length = 1 + np.arange(n_seq) % 3
    seqs = np.stack([np.ones(n_seq, np.int64), length, np.ones(n_seq, np.int64)], axis=1)
    want = np.repeat(lits, 1 + length)
    (got, out_len, status), (one, one_len, one_status) = replay_both(np.zeros(0, np.uint8), seqs, lits, want.size, dev)
    assert status == 0 and out_len == want.size and np.array_equal(got, want)
    assert one_status == 0 and one_len == want.size and np.array_equal(one, want)


# ---- reuse -----------------------------------------------------------------------------------------------------------------
def test_a_scratch_from_a_larger_call_and_a_second_block_on_the_first(dev):
    w = markov1_stream(5 * T + 9, 21)
    cut = 2 * T + 3
    big = dict(name="big", window=w, start=0, L=6, M=64)
    scratch = torch.empty(dev_lz77.wide_scratch_bytes(len(w)) + 512, dtype=torch.uint8, device=dev)
    first = dict(name="first", window=w[:cut], start=0, L=6, M=64)
    second = dict(name="second", window=w, start=cut, L=6, M=64)
    from lz77_helpers import parse_restated

    for case in (big, first, second, first):  # the same scratch, larger and smaller windows in turn
        wide, batch = parse_both(case, dev, scratch=scratch)
        assert_is_the_rule(wide, parse_restated(case["window"], case["start"], 6, 64), case["name"])
        assert_same_store(wide, batch, case["name"])
    # replay: the window stays on the device, the second block is appended to what the first left there
    slot = torch.full((len(w) + 7,), FILL, dtype=torch.uint8, device=dev)
    have = 0
    rscratch = torch.empty(dev_lz77.wide_replay_scratch_bytes(len(w), len(w) + 7), dtype=torch.uint8, device=dev)
    for case in (first, second):
        res = dev_lz77.parse_wide(torch.from_numpy(case["window"]).to(dev), case["start"], 6, 64)
        n_seq, n_lit = int(res.n_seq[0]), int(res.n_lit[0])
        out_len, status = dev_lz77.replay_wide(slot, have, res.literal_count, res.match_length, res.match_offset, n_seq,
                                               res.literals[case["start"]:], n_lit, scratch=rscratch)
        assert int(status[0]) == 0 and int(out_len[0]) == len(case["window"]) - case["start"]
        have += int(out_len[0])
    host = slot.cpu().numpy()
    assert host[: len(w)].tolist() == w.tolist() and (host[len(w):] == FILL).all()


# ---- dispatch: the host calls and the classes on either side of the threshold --------------------------------------------------
@pytest.mark.parametrize("below", [0, 1], ids=["at-the-threshold", "one-byte-below"])
def test_host_calls_and_classes_give_the_one_wave_results_on_either_side_of_the_threshold(below, dev):
    from stanford_compression_library_amd.compressors.lz77 import LZ77Decoder, LZ77Encoder
    from stanford_compression_library_amd.core.data_block import DataBlock

    n = dev_lz77.wide_threshold() - below
    w = markov1_stream(n, 31)
    cap = dev_lz77.default_seq_cap(n, 6)
    win = torch.from_numpy(w).to(dev)
    res = dev_lz77.parse_batch(win, torch.tensor([0, n], dtype=torch.int64, device=dev),
                               torch.zeros(1, dtype=torch.int32, device=dev), 6, 64, cap)
    want = unpack(res, 0)
    assert want["status"] == 0
    rows, lits = want["rows"][: want["n_seq"]], want["literals"][: want["n_lit"]]
    lc, ml, mo, literals = dev_lz77.parse_host(w, 0, 6, 64)
    assert np.stack([lc, ml, mo], axis=1).tolist() == rows.tolist() and literals.tolist() == lits.tolist()
    back = dev_lz77.replay_host(np.zeros(0, np.uint8), lc, ml, mo, literals)
    assert back.tolist() == w.tolist()
    slot = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_len, status = dev_lz77.replay_batch(slot, torch.tensor([0, n], dtype=torch.int64, device=dev),
                                            torch.zeros(1, dtype=torch.int32, device=dev), res.literal_count, res.match_length,
                                            res.match_offset, res.n_seq, res.literals, res.lit_off, res.n_lit)
    assert int(status[0]) == 0 and int(out_len[0]) == n and torch.equal(slot, win)
    if below == 0:  # the wide calls themselves on the same stream
        wide = unpack(dev_lz77.parse_wide(win, 0, 6, 64, seq_cap=cap), 0)
        assert wide["n_seq"] == want["n_seq"] and wide["n_lit"] == want["n_lit"] and wide["status"] == 0
        assert np.array_equal(wide["rows"], want["rows"]) and np.array_equal(wide["literals"], want["literals"])
    enc = LZ77Encoder(min_match_length=6, max_num_matches_considered=64)
    sequences, class_literals = enc.lz77_parse_and_generate_sequences(DataBlock(w.tolist()))
    assert [[s.literal_count, s.match_length, s.match_offset] for s in sequences] == rows.tolist()
    assert class_literals == lits.tolist()
    bits = LZ77Encoder(min_match_length=6, max_num_matches_considered=64).encode_block(DataBlock(w.tolist()))
    block, used = LZ77Decoder().decode_block(bits)
    assert used == len(bits) and block.data_list == w.tolist()


def test_the_named_kernels_are_in_the_library():
    blob = open(backend_lib.LIB_PATH, "rb").read()
    names = dev_lz77.wide_kernel_names()
    assert len(names) == 3 and all(name.encode() in blob for name in names)
