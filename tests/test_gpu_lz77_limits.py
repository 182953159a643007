"""LZ77 on the GPU past the shapes of test_gpu_lz77.py: the index at a scale that needs every stream-number pass of the
sort and the carry of the block-sum scan, bytes around and between the streams that look like stream content, empty streams,
the `phases` / `scratch=` / `out=` arguments of parse_batch, what the parse must leave alone, and the host calls on nothing.

Everything is compared bit for bit with the restatements in lz77_helpers: the parse with parse_restated, the index itself
with index_restated.  A round trip is no check of the index: the parse re-checks every entry it reads from order[] and
replay restores the input from any valid parse, so a misplaced entry only changes which matches are found.  Every test
asserts the shape that takes it down the path it names."""

import numpy as np
import pytest

from lz77_helpers import (ST_CAPACITY, ST_SIZE, edge_batch, edge_reference, index_restated, index_shape, pack_windows,
                          parse_restated, ragged_batch, ragged_reference, tiled_batch, tiled_reference)
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from test_gpu_lz77 import FILL, assert_parse_equal, parse_device, replay_device

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0x5A5A5A5A  # in every sequence row entry the parse does not own


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def fresh_out(batch, seq_cap, dev):
    """a ParsedBatch the caller owns: sequence rows full of SENTINEL, literals full of FILL, the counts of -1"""
    n_streams, total = len(batch["windows"]), len(batch["buf"])
    rows = lambda: torch.full((n_streams, seq_cap), SENTINEL, dtype=torch.int32, device=dev)  # noqa: E731
    words = lambda: torch.full((n_streams,), -1, dtype=torch.int32, device=dev)  # noqa: E731
    lit_off = torch.from_numpy(batch["win_off"][:-1] + batch["start"].astype(np.int64)).to(dev)
    return dev_lz77.ParsedBatch(rows(), rows(), rows(), torch.full((max(total, 1),), FILL, dtype=torch.uint8, device=dev),
                                words(), words(), words(), lit_off, int(seq_cap))


def default_cap(batch, L):
    return dev_lz77.default_seq_cap(max((len(w) for w in batch["windows"]), default=0), L)


def parse_into(batch, L, M, dev, out=None, scratch=None, phases=0, seq_cap=None):
    """parse_batch with the arguments parse_device leaves at their defaults -> the ParsedBatch (synchronized)"""
    win = torch.from_numpy(batch["buf"]).to(dev)
    win_off = torch.from_numpy(batch["win_off"]).to(dev)
    start = torch.from_numpy(batch["start"]).to(dev)
    res = dev_lz77.parse_batch(win, win_off, start, L, M, seq_cap or default_cap(batch, L), scratch=scratch, out=out,
                               phases=phases)
    torch.cuda.synchronize()
    return res


def host_arrays(res):
    """-> (rows [3, n_streams, seq_cap] as int64 of the uint32 values, n_seq, n_lit, status, literals, lit_off)"""
    rows = np.stack([t.cpu().numpy().view(np.uint32).astype(np.int64)
                     for t in (res.literal_count, res.match_length, res.match_offset)])
    return (rows, res.n_seq.cpu().numpy(), res.n_lit.cpu().numpy(), res.status.cpu().numpy(), res.literals.cpu().numpy(),
            res.lit_off.cpu().numpy())


def per_stream(res):
    """the ParsedBatch as parse_device returns it: ([(sequences [k, 3], literals)], status)"""
    rows, n_seq, n_lit, status, lits, lit_off = host_arrays(res)
    return [(rows[:, s, : int(n_seq[s])].T, lits[lit_off[s]: lit_off[s] + int(n_lit[s])]) for s in range(len(n_seq))], status


def assert_nothing_else_stored(res, what=""):
    """row entries at and beyond n_seq[s] keep SENTINEL, literal bytes outside every [lit_off[s], lit_off[s] + n_lit[s])
    keep FILL (`res` came from fresh_out)"""
    rows, n_seq, n_lit, _, lits, lit_off = host_arrays(res)
    beyond = np.arange(rows.shape[2])[None, :] >= n_seq[:, None]
    for name, r in zip(("literal_count", "match_length", "match_offset"), rows):
        bad = np.argwhere(beyond & (r != SENTINEL))
        assert bad.size == 0, f"{what} {name}: stream {bad[0][0]} stored entry {bad[0][1]} with n_seq = {n_seq[bad[0][0]]}"
    owned = np.zeros(lits.size + 1, np.int64)
    np.add.at(owned, lit_off, 1)
    np.add.at(owned, lit_off + n_lit, -1)
    free = np.cumsum(owned)[:-1] == 0
    bad = np.flatnonzero(free & (lits != FILL))
    assert bad.size == 0, f"{what} literals: byte {bad[:1]} outside every stream's literals was stored"
    assert (~free).sum() == int(n_lit.sum())


# ---- scale -------------------------------------------------------------------------------------------------------------------
def first_stream_that_differs(res, batch, ref):
    """compares every stream of the tiled batch with its template's entry of `ref`, one template at a time
    -> None, or (stream, what differs) of the first stream that differs"""
    rows, n_seq, n_lit, status, lits, lit_off = host_arrays(res)
    bad = {}
    for t, (seq, lit) in enumerate(ref):
        idx = np.flatnonzero(batch["ids"] == t)
        k = len(seq)
        wrong = {"status": status[idx] != 0, "n_seq": n_seq[idx] != k, "n_lit": n_lit[idx] != len(lit)}
        if k:
            wrong["sequences"] = (rows[:, idx, :k] != seq.T[:, None, :]).any(axis=(0, 2))
        if len(lit):
            at = np.minimum(lit_off[idx, None] + np.arange(len(lit))[None, :], lits.size - 1)
            wrong["literals"] = (lits[at] != lit[None, :]).any(axis=1)
        for what, w in wrong.items():
            if w.any():
                s = int(idx[np.argmax(w)])
                bad[s] = bad.get(s, []) + [what]
    return (min(bad), bad[min(bad)]) if bad else None


@pytest.mark.parametrize("L,M", [(3, 0), (6, 64)])
def test_tiled_batch_equals_the_restatement_and_replays(L, M, dev):
    """70 000 streams, about 9 MB.  Reaches: all three stream-number passes of the sort (n_streams >= 65 536; the digit
    n_streams of the lead byte needs the third), passes = L + 3 = 6 and 9 (both parities of the ping-pong between
    order_a and order_b), the carry of lz77_scan_block_sums across its 256-entry trips (more than 256 scan blocks), and
    lz77_parse / lz77_replay over 17 500 workgroups.  Periodic templates tie all candidates, so the newest wins only under
    a stable sort; identical neighbouring streams share every gram, so a match that crossed a stream boundary would show."""
    batch = tiled_batch()
    n_streams, N = len(batch["windows"]), len(batch["buf"])
    sh = index_shape(N)
    assert n_streams >= 65536 and sh.n_scan_blocks > 256 and sh.n_tiles > 2048
    assert (batch["ids"][1:] == batch["ids"][:-1]).any() and {(k + 3) % 2 for k in (3, 6)} == {0, 1}
    res = parse_into(batch, L, M, dev)
    assert first_stream_that_differs(res, batch, tiled_reference(L, M)) is None
    out = torch.full((N,), FILL, dtype=torch.uint8, device=dev)
    out_len, status = dev_lz77.replay_batch(out, torch.from_numpy(batch["win_off"]).to(dev),
                                            torch.zeros(n_streams, dtype=torch.int32, device=dev), res.literal_count,
                                            res.match_length, res.match_offset, res.n_seq, res.literals, res.lit_off,
                                            res.n_lit)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    assert np.array_equal(out_len.cpu().numpy(), np.diff(batch["win_off"]))
    assert np.array_equal(out.cpu().numpy(), batch["buf"])


# ---- the index against its definition ------------------------------------------------------------------------------------------
def check_index(batch, L, dev):
    N = len(batch["buf"])
    sh = index_shape(N)
    assert sh.total == dev_lz77.scratch_bytes(N, len(batch["windows"]))
    scratch = torch.full((sh.total,), FILL, dtype=torch.uint8, device=dev)
    parse_into(batch, L, 64, dev, scratch=scratch)
    raw = scratch.cpu().numpy()
    order = raw[sh.order_a: sh.order_a + 4 * N].view(np.uint32)
    rank = raw[sh.rank: sh.rank + 4 * N].view(np.uint32)
    bitmap = raw[sh.bitmap: sh.bitmap + 8 * sh.n_words].view(np.uint64).copy()
    want_order, want_rank, want_bitmap = index_restated(batch["buf"], batch["win_off"], L)
    bad = np.flatnonzero(order != want_order)
    assert bad.size == 0, f"L={L}: order[] differs from entry {bad[0]} on ({bad.size} entries): the sort"
    bad = np.flatnonzero(rank != want_rank)
    assert bad.size == 0, f"L={L}: rank[] differs at position {bad[0]} with order[] right: the last scatter pass"
    if N % 64:  # only bits below N
        bitmap[-1] &= np.uint64((1 << (N % 64)) - 1)
    bad = np.flatnonzero(bitmap != want_bitmap)
    assert bad.size == 0, f"L={L}: bitmap word {bad[0]} differs with order[] and rank[] right: lz77_candidate_bitmap"


@pytest.mark.parametrize("L", [1, 6, 8])
def test_index_of_the_ragged_batch_equals_its_definition(L, dev):
    """WHITE BOX: reads order[] (the order_a part), rank[] and the bitmap out of the scratch at the offsets of
    lz77_helpers.index_shape, which restates csrc/scl_lz77_internal.h (pinned to the library by
    test_lz77_host.test_restated_scratch_layout_equals_the_library), and compares them with index_restated.  It depends on
    that layout on purpose: where the parse tests only say "sequences differ", this one names the stage -- sort, inverse
    or bitmap.  Reaches lz77_sort_histogram / lz77_sort_scatter with L + 1 = 2, 7 and 9 passes (130 streams: one
    stream-number pass), the result in order_a after an even and an odd count, and lz77_candidate_bitmap at streams with
    histories, at empty streams and at L = 8 (the whole 64-bit key)."""
    batch = ragged_batch()
    assert 1 < len(batch["windows"]) < 256 and index_shape(len(batch["buf"])).n_tiles > 1
    check_index(batch, L, dev)


def test_index_of_the_tiled_batch_equals_its_definition(dev):
    """WHITE BOX, as above, at the scale of the tiled batch and L = 6: nine passes, three of them over the stream number,
    2181 tiles and more than 256 scan blocks, so that a lost carry in lz77_scan_block_sums, which would move whole tiles
    of a digit, shows as a wrong order[] and not only as other matches."""
    batch = tiled_batch()
    assert len(batch["windows"]) >= 65536 and index_shape(len(batch["buf"])).n_scan_blocks > 256
    check_index(batch, 6, dev)


# ---- stream-count edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("n_streams", [1, 2, 255, 256, 257])
def test_stream_count_edges_with_lookalike_bytes_around(n_streams, L, M, dev):
    """The stream-number passes of the sort (lz_stream_passes) at their edges: none for one stream (the lead is sorted
    among the stream's own positions and only the `c >= base` checks of lz77_candidate_bitmap and lz77_parse keep it
    out), one up to 255 streams (the digit n_streams = 255 of the bytes outside still fits), two from 256 on.  A lead
    that copies the start of stream 0, a tail that copies the last stream, identical neighbours, and runs of three
    empty streams in the middle and at the end (lz_stream_of: the last s with win_off[s] <= v): the parse equals the
    restatement of every stream on its own, so no match reaches into the lead, the tail or a neighbour."""
    batch = edge_batch(n_streams)
    lens = np.diff(batch["win_off"])
    assert len(lens) == n_streams and batch["win_off"][0] == 40 and len(batch["buf"]) == batch["win_off"][-1] + 40
    assert batch["buf"][:40].tolist() == batch["windows"][0][:40].tolist()
    if n_streams >= 8:
        assert (lens[-3:] == 0).all() and (lens[n_streams // 2: n_streams // 2 + 3] == 0).all()
        assert any(np.array_equal(a, b) and len(a) for a, b in zip(batch["windows"], batch["windows"][1:]))
    want = edge_reference(n_streams, L, M)
    assert sum(len(seq) for seq, _ in want) >= n_streams
    got, status, _ = parse_device(batch, L, M, dev)
    assert not status.any()
    assert_parse_equal(got, want, f"n_streams={n_streams} L={L} M={M}")
    # and replay of these sequences fills every slot, the empty ones included, with its window and nothing else
    streams = [(w[: int(st)], seq, lit, len(w)) for w, st, (seq, lit) in zip(batch["windows"], batch["start"], got)]
    _, status, after, win_off = replay_device(streams, dev, lead=40)
    assert not status.any() and (after[:40] == FILL).all()
    assert after[40:].tolist() == batch["buf"][40: int(batch["win_off"][-1])].tolist() and win_off[-1] == batch["win_off"][-1]


# ---- phases, scratch=, out= ------------------------------------------------------------------------------------------------------
def test_index_and_parse_in_two_calls_on_a_used_scratch(dev):
    """scl_lz77_parse_batch with phases = SCL_LZ77_INDEX, then SCL_LZ77_PARSE, on a scratch that the larger ragged batch
    has filled (the layout of the small batch puts every part elsewhere, over the large one's leftovers) and into an
    `out=` that holds an earlier result: the index call stores no result, the parse call finds the index of the call
    before, and nothing depends on what scratch or result held."""
    big, small = ragged_batch(), edge_batch(257)
    scratch = torch.full((dev_lz77.scratch_bytes(len(big["buf"]), 130),), FILL, dtype=torch.uint8, device=dev)
    assert scratch.numel() > 4 * dev_lz77.scratch_bytes(len(small["buf"]), 257)
    got, status = per_stream(parse_into(big, 6, 64, dev, scratch=scratch))
    assert not status.any()
    assert_parse_equal(got, ragged_reference(6, 64), "the large batch")
    cap = default_cap(small, 2)
    out = fresh_out(small, cap, dev)
    got, status = per_stream(parse_into(small, 2, 0, dev, out=out, scratch=scratch, seq_cap=cap))  # an earlier result
    assert not status.any()
    assert_parse_equal(got, edge_reference(257, 2, 0), "the small batch, one call")
    before = [a.copy() for a in host_arrays(out)]
    res = parse_into(small, 3, 2, dev, out=out, scratch=scratch, phases=backend_lib.LZ77_INDEX, seq_cap=cap)
    assert res is out and all(np.array_equal(a, b) for a, b in zip(before, host_arrays(out))), "the index call stored a result"
    res = parse_into(small, 3, 2, dev, out=out, scratch=scratch, phases=backend_lib.LZ77_PARSE, seq_cap=cap)
    got, status = per_stream(res)
    assert not status.any()
    assert_parse_equal(got, edge_reference(257, 3, 2), "the small batch, two calls")


# ---- what the parse leaves alone ---------------------------------------------------------------------------------------------------
def test_parse_of_the_ragged_batch_stores_nothing_it_does_not_own(dev):
    """lz77_parse stores sequences [0, n_seq[s]) of row s and literals [lit_off[s], lit_off[s] + n_lit[s]) and nothing
    else: every other row entry keeps its sentinel and every other literal byte (the histories, the lead) its fill."""
    batch = ragged_batch()
    assert any(batch["start"]) and any(len(w) == 0 for w in batch["windows"])
    res = parse_into(batch, 3, 64, dev, out=fresh_out(batch, default_cap(batch, 3), dev))
    got, status = per_stream(res)
    assert not status.any()
    assert_parse_equal(got, ragged_reference(3, 64))
    assert_nothing_else_stored(res)


def test_parse_that_runs_out_of_row_stores_nothing_it_does_not_own(dev):
    """the SCL_ST_CAPACITY exit of lz77_parse (seq_cap = 8, streams with more sequences): the row is exactly full, the
    ninth sequence lands nowhere -- not in the next stream's row -- and its literal run is not stored either"""
    rng = np.random.default_rng(3)
    windows = [rng.integers(0, 2, 300).astype(np.uint8), rng.integers(0, 256, 300).astype(np.uint8),
               rng.integers(0, 2, 300).astype(np.uint8)]
    batch = pack_windows(windows, [0, 0, 0])
    want = [parse_restated(w, 0, 2, 64) for w in windows]
    assert len(want[0][0]) > 8 and len(want[1][0]) <= 8 and len(want[2][0]) > 8
    res = parse_into(batch, 2, 64, dev, out=fresh_out(batch, 8, dev), seq_cap=8)
    got, status = per_stream(res)
    assert status.tolist() == [ST_CAPACITY, 0, ST_CAPACITY]
    for s in (0, 2):
        assert got[s][0].tolist() == want[s][0][:8].tolist()
        assert got[s][1].tolist() == want[s][1][: int(want[s][0][:8, 0].sum())].tolist()
    assert_parse_equal(got[1:2], want[1:2])
    assert_nothing_else_stored(res)


def test_a_last_stream_that_ends_past_the_buffer_is_refused_alone(dev):
    """win_off[n_streams] > N: lz77_parse answers SCL_ST_SIZE for the last stream and stores nothing for it;
    lz77_candidate_bitmap clamps that stream's end to N, and every other stream is parsed as if nothing were wrong"""
    rng = np.random.default_rng(8)
    windows = [rng.integers(0, 3, n).astype(np.uint8) for n in (60, 0, 75, 130, 64)]
    batch = pack_windows(windows, [0, 0, 5, 0, 0])
    batch["win_off"] = batch["win_off"].copy()
    batch["win_off"][-1] += 5
    assert batch["win_off"][-1] > len(batch["buf"]) > batch["win_off"][-2]
    want = [parse_restated(w, int(s), 3, 64) for w, s in zip(windows, batch["start"])]
    assert all(len(seq) for seq, _ in want[2:])
    res = parse_into(batch, 3, 64, dev, out=fresh_out(batch, default_cap(batch, 3), dev))
    got, status = per_stream(res)
    assert status.tolist() == [0, 0, 0, 0, ST_SIZE]
    assert len(got[4][0]) == 0 and len(got[4][1]) == 0
    assert_parse_equal(got[:4], want[:4])
    assert_nothing_else_stored(res)


# ---- the host calls on nothing -------------------------------------------------------------------------------------------------------
def test_host_calls_on_nothing(dev):
    """scl_lz77_parse_host with n = 0 (no index kernels, lz77_parse on an empty window) and with start == n (an index,
    and a parse that begins at the end); scl_lz77_replay_host with no sequences and no literals, without and with a
    history (a slot of 0 bytes, and one that is full before the first byte)"""
    for window, start in ((np.zeros(0, np.uint8), 0), (np.arange(50, dtype=np.uint8) % 3, 50)):
        lc, ml, mo, lit = dev_lz77.parse_host(window, start, 6, 64)
        assert lc.size == 0 and ml.size == 0 and mo.size == 0 and lit.size == 0
    none = np.zeros(0, np.uint32)
    for history in (np.zeros(0, np.uint8), np.arange(10, dtype=np.uint8)):
        back = dev_lz77.replay_host(history, none, none, none, np.zeros(0, np.uint8))
        assert back.dtype == np.uint8 and back.size == 0
