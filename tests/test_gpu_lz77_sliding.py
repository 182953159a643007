"""Sliding-window LZ77 on the GPU: the hash-bucket index, the lazy parse and the windowed replay against the reference's
goldens and against the restatement of the rule in lz77_sliding_helpers -- through the classes and the batch calls.

The batch is lz77_helpers.ragged_batch(): 130 streams (four to a workgroup, the last workgroup partial) of 0..3000 bytes at
odd offsets; the five parameter sets take every path of the parse: one bucket for everything (m = 1) and one per gram,
chains shorter and longer than the candidates there are, windows shorter than the streams, lazy and not, hash_length 1
and 8, minimum_match_length below and above hash_length."""
import ctypes

import numpy as np
import pytest

from lz77_helpers import ST_CAPACITY, ST_STATE, ST_TRUNCATED, edge_batch, pack_windows, ragged_batch, with_garbage
from lz77_helpers import parse_restated as greedy_parse_restated
from lz77_helpers import replay_restated as greedy_replay_restated
from lz77_sliding_helpers import case_params, golden_blocks, goldens, parse_restated, ragged_reference, replay_restated
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from stanford_compression_library_amd.compressors.lz77 import LZ77Sequence
from stanford_compression_library_amd.compressors.lz77_sliding_window import (HashBasedMatchFinder, LZ77SlidingWindowDecoder,
                                                                              LZ77SlidingWindowEncoder)
from stanford_compression_library_amd.core.data_block import DataBlock
from stanford_compression_library_amd.utils.bitarray_utils import BitArray

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLIDING = [c for c in goldens() if c.kind == "sliding"]
FILL = 0xA5
PARAMS = [(4, 1000000, 64, 1000000, 1, 4), (2, 1, 2, 16, 1, 4), (4, 3, 64, 100, 0, 4), (1, 256, 5, 50, 1, 1),
          (8, 65536, 64, 1000, 1, 6)]  # (hl, m, C, W, lazy, mml)


def helper_params(p):
    hl, m, C, W, lazy, mml = p
    return (hl, m, C, lazy, mml, W)


def device_params(p):
    hl, m, C, W, lazy, mml = p
    return dev_lz77.SlidingParams(hl, m, C, bool(lazy), mml, W)


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def make_coders(case, init):
    finder = HashBasedMatchFinder(case.hl, case.m, case.C, case.lazy, case.mml)
    return (LZ77SlidingWindowEncoder(finder, window_size=case.W, initial_window=init),
            LZ77SlidingWindowDecoder(window_size=case.W, initial_window=init))


# ---- the goldens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SLIDING, ids=repr)
def test_goldens_through_the_classes(case, dev):
    init = case.arr("init").tolist()
    enc, dec = make_coders(case, init)
    for b, (window, data, seq, lit, out, nbits, consumed) in enumerate(golden_blocks(case)):
        if case.reset_before[b]:
            enc.reset()
            dec = LZ77SlidingWindowDecoder(window_size=case.W)
        assert enc.window.get_window_as_list() == window.tolist()
        twin, _ = make_coders(case, window.tolist())
        sequences, literals = twin.lz77_parse_and_generate_sequences(data.tolist())
        assert sequences == [LZ77Sequence(*row) for row in seq.tolist()] and literals == lit.tolist()
        bits = enc.encode_block(DataBlock(data.tolist()))
        assert len(bits) == nbits and np.array_equal(bits.packed(), out)
        for fed, i in with_garbage(case, out, nbits):
            fresh = LZ77SlidingWindowDecoder(window_size=case.W, initial_window=window.tolist())
            block, used = fresh.decode_block(BitArray._wrap(fed.copy()))
            assert block.data_list == data.tolist() and used == consumed[i]
        block, used = dec.decode_block(bits)
        assert block.data_list == data.tolist() and used == nbits
        assert dec.window.get_window_as_list() == enc.window.get_window_as_list()
        assert (dec.window.start, dec.window.end) == (enc.window.start, enc.window.end)


def test_file_golden_byte_for_byte(dev, tmp_path):
    case = [c for c in goldens() if c.kind == "file"][0]
    init = case.arr("init").tolist()
    src, coded, back = (str(tmp_path / f) for f in ("in.bin", "coded.bin", "back.bin"))
    case.arr("data").tofile(src)
    LZ77SlidingWindowEncoder(HashBasedMatchFinder(), window_size=case.W, initial_window=init).encode_file(
        src, coded, block_size=case.block_size)
    assert np.array_equal(np.fromfile(coded, np.uint8), case.arr("encoded"))
    LZ77SlidingWindowDecoder(window_size=case.W, initial_window=init).decode_file(coded, back)
    assert np.array_equal(np.fromfile(back, np.uint8), case.arr("data"))


def test_decoder_refuses_an_offset_beyond_the_window(dev):
    dec = LZ77SlidingWindowDecoder(window_size=8, initial_window=list(range(20)))
    assert dec.execute_lz77_sequences([1, 2], [LZ77Sequence(2, 3, 8), LZ77Sequence(0, 0, 0)]) == [1, 2, 14, 15, 16]
    with pytest.raises(backend_lib.SclHipError):
        dec.execute_lz77_sequences([], [LZ77Sequence(0, 3, 9)])


# ---- the batch calls ---------------------------------------------------------------------------------------------------------
def parse_device(batch, params, dev, seq_cap=None, scratch=None):
    """-> ([(sequences [k, 3], literals)] per stream, status array, the ParsedBatch)"""
    win = torch.from_numpy(batch["buf"]).to(dev)
    win_off = torch.from_numpy(batch["win_off"]).to(dev)
    start = torch.from_numpy(batch["start"]).to(dev)
    res = dev_lz77.sliding_parse_batch(win, win_off, start, params, seq_cap, scratch=scratch)
    torch.cuda.synchronize()
    n_seq, n_lit = res.n_seq.cpu().numpy(), res.n_lit.cpu().numpy()
    rows = [t.cpu().numpy().view(np.uint32).astype(np.int64) for t in (res.literal_count, res.match_length, res.match_offset)]
    lits, lit_off = res.literals.cpu().numpy(), res.lit_off.cpu().numpy()
    out = []
    for s in range(len(batch["windows"])):
        k = int(n_seq[s])
        out.append((np.stack([r[s, :k] for r in rows], axis=1), lits[lit_off[s]: lit_off[s] + int(n_lit[s])]))
    return out, res.status.cpu().numpy(), res


def assert_parse_equal(got, want, what=""):
    for s, ((seq, lit), (ref_seq, ref_lit)) in enumerate(zip(got, want)):
        assert seq.tolist() == ref_seq.tolist(), f"{what} stream {s}: sequences differ"
        assert lit.tolist() == ref_lit.tolist(), f"{what} stream {s}: literals differ"


@pytest.mark.parametrize("p", PARAMS, ids=str)
def test_parse_of_a_ragged_batch_equals_the_restatement_and_round_trips(p, dev):
    batch = ragged_batch()
    assert len(batch["windows"]) == 130
    got, status, parsed = parse_device(batch, device_params(p), dev)
    assert not status.any()
    assert_parse_equal(got, ragged_reference(helper_params(p)), str(p))
    # the same entropy stage as the greedy coder's, then decode + windowed replay into slots that hold the histories
    encoded = dev_lz77.encode_batch(parsed)
    assert not encoded.status.cpu().numpy().any()
    windows, start = batch["windows"], batch["start"]
    slots = pack_windows([np.concatenate([w[:s], np.full(len(w) - s, FILL, np.uint8)]) for w, s in zip(windows, start)], start)
    win = torch.from_numpy(slots["buf"]).to(dev)
    out_len, st, _ = dev_lz77.sliding_decompress_batch(encoded.bits, encoded.bit_offset, encoded.nbits, win,
                                                       torch.from_numpy(slots["win_off"]).to(dev),
                                                       torch.from_numpy(start).to(dev), parsed.seq_cap, window_size=p[3])
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    assert out_len.cpu().numpy().tolist() == [len(w) - s for w, s in zip(windows, start)]
    assert np.array_equal(win.cpu().numpy(), batch["buf"])


@pytest.mark.parametrize("n_streams", [1, 255, 257])
def test_stream_counts_around_a_byte_with_empty_streams(n_streams, dev):
    """one stream has no stream-number pass in the index, 255 one, 257 two; the lead and the tail of the buffer belong to
    no stream but look like stream content, and from 8 streams on some in the middle and the last three are empty"""
    batch = edge_batch(n_streams)
    params = (3, 1000, 4, 1, 3, 60)
    want = [parse_restated(w, int(s), params) for w, s in zip(batch["windows"], batch["start"])]
    got, status, _ = parse_device(batch, dev_lz77.SlidingParams(3, 1000, 4, True, 3, 60), dev)
    assert not status.any()
    assert_parse_equal(got, want, f"{n_streams} streams")


def test_parse_writes_nothing_outside_its_rows_and_literal_ranges(dev):
    batch = ragged_batch()
    p = PARAMS[1]
    want = ragged_reference(helper_params(p))
    n_streams, total = len(batch["windows"]), len(batch["buf"])
    longest = max(len(w) - int(s) for w, s in zip(batch["windows"], batch["start"]))
    full_cap = dev_lz77.sliding_seq_cap(longest, p[5])
    assert max(len(seq) for seq, _ in want) <= full_cap
    win = torch.from_numpy(batch["buf"]).to(dev)
    win_off, start = torch.from_numpy(batch["win_off"]).to(dev), torch.from_numpy(batch["start"]).to(dev)
    for seq_cap in (full_cap, 7):  # 7: many rows run full
        rows = lambda: torch.full((n_streams, seq_cap), 0x5A5A5A5A, dtype=torch.int32, device=dev)  # noqa: E731
        words = lambda: torch.full((n_streams,), -1, dtype=torch.int32, device=dev)  # noqa: E731
        out = dev_lz77.ParsedBatch(rows(), rows(), rows(), torch.full((total,), FILL, dtype=torch.uint8, device=dev), words(),
                                   words(), words(), win_off[:-1] + start.to(torch.int64), seq_cap)
        dev_lz77.sliding_parse_batch(win, win_off, start, device_params(p), out=out)
        torch.cuda.synchronize()
        n_seq, n_lit, status = (t.cpu().numpy() for t in (out.n_seq, out.n_lit, out.status))
        lits = out.literals.cpu().numpy()
        expect_lits = np.full(total, FILL, np.uint8)
        full = 0
        for s, (seq, lit) in enumerate(want):
            k = min(len(seq), seq_cap)
            over = len(seq) > seq_cap
            full += over
            assert status[s] == (ST_CAPACITY if over else 0) and n_seq[s] == k
            for field, t in enumerate((out.literal_count, out.match_length, out.match_offset)):
                row = t[s].cpu().numpy().view(np.uint32).astype(np.int64)
                assert row[:k].tolist() == seq[:k, field].tolist() and (row[k:] == 0x5A5A5A5A).all()
            kept = int(seq[:k, 0].sum())
            assert n_lit[s] == kept
            at = int(batch["win_off"][s]) + int(batch["start"][s])
            expect_lits[at: at + kept] = lit[:kept]
        assert np.array_equal(lits, expect_lits)
        assert (full > 0) == (seq_cap == 7)


def test_scratch_of_a_larger_batch_is_reused(dev):
    big, small = ragged_batch(), edge_batch(9)
    p = PARAMS[0]
    scratch = torch.empty(dev_lz77.sliding_scratch_bytes(len(big["buf"]), 130), dtype=torch.uint8, device=dev)
    got, status, _ = parse_device(big, device_params(p), dev, scratch=scratch)
    assert not status.any()
    assert_parse_equal(got, ragged_reference(helper_params(p)))
    want = [parse_restated(w, int(s), helper_params(p)) for w, s in zip(small["windows"], small["start"])]
    got, status, _ = parse_device(small, device_params(p), dev, scratch=scratch)
    assert not status.any()
    assert_parse_equal(got, want, "reused scratch")


# ---- replay statuses ---------------------------------------------------------------------------------------------------------
def replay_device(dev, histories, caps, seqs, lits, window_size, call=None):
    """slots of caps[s] bytes holding histories[s], between sentinel bytes -> (slot contents, out_len, status).  ``call``:
    what replays the tensors, ``sliding_replay_batch`` with ``window_size`` unless given"""
    call = call or (lambda *tensors: dev_lz77.sliding_replay_batch(*tensors, window_size=window_size))
    n = len(histories)
    slots = pack_windows([np.concatenate([h, np.full(c - len(h), FILL, np.uint8)]) for h, c in zip(histories, caps)],
                         [len(h) for h in histories], lead=np.full(3, 0x77, np.uint8), tail=np.full(5, 0x77, np.uint8))
    seq_cap = max(len(q) for q in seqs)
    rows = np.zeros((3, n, seq_cap), np.int64)
    for s, q in enumerate(seqs):
        rows[:, s, :len(q)] = np.asarray(q, np.int64).reshape(-1, 3).T
    lit_off = np.concatenate([[0], np.cumsum([len(x) for x in lits])]).astype(np.int64)
    literals = np.concatenate([np.asarray(x, np.uint8) for x in lits] + [np.zeros(1, np.uint8)])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)  # noqa: E731
    win = t(slots["buf"], np.uint8)
    out_len, status = call(
        win, t(slots["win_off"], np.int64), t(slots["start"], np.int32), t(rows[0], np.int32), t(rows[1], np.int32),
        t(rows[2], np.int32), t(np.array([len(q) for q in seqs]), np.int32), t(literals, np.uint8), t(lit_off[:-1], np.int64),
        t(np.array([len(x) for x in lits]), np.int32))
    torch.cuda.synchronize()
    return win.cpu().numpy(), slots, out_len.cpu().numpy(), status.cpu().numpy()


def test_replay_statuses_and_sentinels(dev):
    W = 8
    hist = np.arange(20, dtype=np.uint8)
    cases = [  # (history, slot bytes, sequences, literals, expected status)
        (hist, 40, [(2, 3, W + 1)], [1, 2], ST_STATE),           # W + 1 with more than W bytes present
        (hist, 40, [(2, 3, W)], [1, 2], 0),                      # W itself is allowed
        (hist[:3], 40, [(1, 2, 5)], [9], ST_STATE),              # beyond the bytes so far (4), inside W
        (hist[:3], 40, [(1, 2, 4)], [9], 0),
        (hist, 40, [(2, 0, 0), (1, 0, 77), (0, 4, 2)], [1, 2, 3], 0),  # (k, 0, 0): nothing copied, the offset not looked at
        (hist, 40, [(1, 2, 1), (3, 2, 1)], [1, 2, 3], ST_TRUNCATED),   # the literals run out
        (hist, 24, [(2, 3, 2)], [1, 2], ST_CAPACITY),            # the match does not fit
        (hist, 21, [(2, 0, 0)], [1, 2], ST_CAPACITY),            # the literals do not fit
        (hist, 27, [(2, 5, 1)], [1, 2], 0),                      # fits exactly
        (np.zeros(0, np.uint8), 10, [(0, 3, 1)], [], ST_STATE),  # nothing to copy from
    ]
    got, slots, out_len, status = replay_device(dev, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                                [c[3] for c in cases], W)
    expect = slots["buf"].copy()
    for s, (h, cap, seq, lit, want_status) in enumerate(cases):
        new, st = replay_restated(h, seq, lit, window_size=W, cap=cap)
        assert st == want_status and status[s] == want_status, f"case {s}"
        assert out_len[s] == len(new), f"case {s}"
        at = int(slots["win_off"][s]) + len(h)
        expect[at: at + len(new)] = new
    # what a stream stored before its fault is there, and nothing else changed: fill bytes, the lead and the tail
    assert np.array_equal(got, expect)
    # no window bound: the first case passes
    _, _, out_len, status = replay_device(dev, [hist], [40], [[(2, 3, W + 1)]], [[1, 2]], 0)
    assert status[0] == 0 and out_len[0] == 5


# ---- the two coders share their replay frame and their host frame: what must still differ, and what must not ------------------
TWO_RULES = [[(2, 0, 0), (0, 4, 2)], [(1, 0, 77), (0, 3, 1)], [(2, 3, 9)], [(2, 3, 8)]]
TWO_RULES_LITS = [[1, 2], [3], [4, 5], [6, 7]]


def test_same_sequences_under_the_two_replay_rules(dev):
    """a match length of 0 ends a greedy stream (offset 0, or beyond the bytes so far) and is skipped by the windowed rule;
    offset 9 is fine without a window and ST_STATE at window_size 8, offset 8 is fine under both"""
    hist = np.arange(20, dtype=np.uint8)
    args = (dev, [hist] * 4, [64] * 4, TWO_RULES, TWO_RULES_LITS)
    for name, restated, call, want_status, want_len in (
            ("greedy", greedy_replay_restated, dev_lz77.replay_batch, [ST_STATE, ST_STATE, 0, 0], [2, 1, 5, 5]),
            ("sliding", lambda h, q, x, cap: replay_restated(h, q, x, window_size=8, cap=cap), None, [0, 0, ST_STATE, 0],
             [6, 4, 2, 5])):
        got, slots, out_len, status = replay_device(*args, 8, call=call)
        assert status.tolist() == want_status and out_len.tolist() == want_len, name
        expect = slots["buf"].copy()
        for s in range(4):
            new, st = restated(hist, TWO_RULES[s], TWO_RULES_LITS[s], cap=64)
            assert st == want_status[s] and len(new) == want_len[s], f"{name} stream {s}"
            at = int(slots["win_off"][s]) + len(hist)
            expect[at: at + len(new)] = new
        assert np.array_equal(got, expect), name


def test_reserved_of_the_greedy_replay_is_not_a_window(dev):
    def raw(reserved):
        def call(win, win_off, have, lc, ml, mo, n_seq, literals, lit_off, n_lit):
            out_len, status = (torch.zeros(have.numel(), dtype=torch.int32, device=dev) for _ in range(2))
            a = backend_lib.Lz77ReplayArgs(win.data_ptr(), win_off.data_ptr(), have.data_ptr(), int(have.numel()),
                                           int(win.numel()), int(lc.shape[1]), reserved, lc.data_ptr(), ml.data_ptr(),
                                           mo.data_ptr(), n_seq.data_ptr(), literals.data_ptr(), int(literals.numel()),
                                           lit_off.data_ptr(), n_lit.data_ptr(), out_len.data_ptr(), status.data_ptr())
            rc = backend_lib.load().scl_lz77_replay_batch(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
            backend_lib.check(rc, "scl_lz77_replay_batch")
            return out_len, status
        return call

    hist = np.arange(20, dtype=np.uint8)
    got5, _, out_len5, status5 = replay_device(dev, [hist], [40], [[(2, 3, 9)]], [[1, 2]], 0, call=raw(5))
    got0, _, out_len0, status0 = replay_device(dev, [hist], [40], [[(2, 3, 9)]], [[1, 2]], 0, call=raw(0))
    assert status5[0] == 0 and status0[0] == 0 and out_len5[0] == 5 and out_len0[0] == 5
    assert np.array_equal(got5, got0)
    new, _ = greedy_replay_restated(hist, [(2, 3, 9)], [1, 2], cap=40)
    assert got5[3 + 20: 3 + 25].tolist() == new.tolist() == [1, 2, 13, 14, 15]


HOST_SLIDING = (4, 1000, 64, 1, 4, 64)  # (hl, m, C, lazy, mml, W) as lz77_sliding_helpers takes them
HOST_PAIRS = {
    "greedy": (lambda w, s: dev_lz77.parse_host(w, s, 4, 64), dev_lz77.replay_host,
               lambda w, s: greedy_parse_restated(w, s, 4, 64), greedy_replay_restated, "scl_lz77_replay_host", ()),
    "sliding": (lambda w, s: dev_lz77.sliding_parse_host(w, s, dev_lz77.SlidingParams(4, 1000, 64, True, 4, 64)),
                lambda *a: dev_lz77.sliding_replay_host(*a, window_size=64),
                lambda w, s: parse_restated(w, s, HOST_SLIDING),
                lambda h, q, x, cap: replay_restated(h, q, x, window_size=64, cap=cap), "scl_lz77_sliding_replay_host", (64,)),
}


@pytest.mark.parametrize("coder", sorted(HOST_PAIRS))
def test_one_host_frame_both_directions(coder, dev):
    parse, replay, parse_ref, replay_ref, entry, extra = HOST_PAIRS[coder]
    data = np.random.default_rng(11).integers(0, 4, 400).astype(np.uint8)
    for window, start in ((data[:300], 0), (data, 100), (data[:100], 100)):  # no history, history, the empty block
        lc, ml, mo, lits = parse(window, start)
        ref_seq, ref_lit = parse_ref(window, start)
        assert np.stack([lc, ml, mo], axis=1).astype(np.int64).tolist() == ref_seq.tolist(), (coder, start)
        assert lits.tolist() == ref_lit.tolist(), (coder, start)
        assert len(lits) + int(ml.sum()) == len(window) - start, (coder, start)
        assert replay(window[:start], lc, ml, mo, lits).tolist() == window[start:].tolist(), (coder, start)
    # a replay that faults at sequence 2: the bytes in front of the fault come back with SCL_E_CHUNK
    hist = np.arange(20, dtype=np.uint8)
    seqs, lits = np.array([(1, 2, 1), (1, 2, 1), (0, 3, 0)], np.uint32), np.array([5, 6], np.uint8)
    new, st = replay_ref(hist, seqs, lits, cap=29)
    assert st == ST_STATE and len(new) == 6
    with pytest.raises(backend_lib.SclHipError) as err:
        replay(hist, seqs[:, 0], seqs[:, 1], seqs[:, 2], lits)
    assert err.value.code == backend_lib.E_CHUNK
    buf = np.concatenate([hist, np.full(9, FILL, np.uint8)])
    rows = [np.ascontiguousarray(seqs[:, k]) for k in range(3)]
    out_len = ctypes.c_uint64(0)
    rc = getattr(backend_lib.load(), entry)(backend_lib.u8_ptr(buf), 20, 29, *extra, *(backend_lib.u32_ptr(r) for r in rows), 3,
                                            backend_lib.u8_ptr(lits), 2, ctypes.byref(out_len))
    assert rc == backend_lib.E_CHUNK and out_len.value == 6
    assert buf.tolist() == hist.tolist() + new.tolist() + [FILL] * 3
