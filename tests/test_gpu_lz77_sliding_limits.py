"""Sliding-window LZ77 on the GPU past the shapes of test_gpu_lz77_sliding.py: the bucket index against its definition at
every pass count of the sort and at the edges of key_passes, a batch that needs every stream-number pass and the carry of
the block-sum scan, the stream-count edges, one stream long enough for several steps of lz_next_bit, a block of 100 000
bytes through the classes, the `phases` / `scratch=` / `out=` arguments, the SCL_ST_SIZE exits and the host calls on nothing.

Everything is compared exactly with the restatements in lz77_sliding_helpers: the parse with parse_restated, key[], order[],
rank[] and the bitmap with sliding_index_restated.  A round trip is no check of the index: the parse re-checks every entry it
reads from order[], so a misplaced entry only changes which matches are found.  The properties of the inputs that take a
test down the path it names are asserted in test_lz77_sliding_host.py on the restatement, and the shapes here.

Sort passes = key_passes(m) + lz_stream_passes(n_streams), reached by:
  1  one stream, m = 256                                   (index; parse of 1 stream, m = 256)
  2  130 streams, m = 1 and 256; 2 and 255 streams, m = 256
  3  130 streams, m = 257 and 65 536; 1 stream, m = 65 537; 256 and 257 streams, m = 256
  4  one stream, m = 2^32 - 1; 70 000 streams, m = 1; 2 and 255 streams, m = 65 537
  5  130 streams, m = 2^24 + 1 and 2^32 - 1; 257 streams, m = 65 537 and 2^24; 256 streams, m = 65 537
  6  257 streams, m = 2^24 + 1
  7  70 000 streams, m = 2^24 + 1
The passes ping-pong between order_a and order_b and end in order_a: an odd count writes its first pass to order_a, an
even one to order_b."""
import numpy as np
import pytest

from lz77_helpers import ST_SIZE, edge_batch, pack_windows, ragged_batch, tiled_batch
from lz77_sliding_helpers import (INDEX_CASES, LONG_N, LONG_PARAMS, LONG_STEP, ONE_STREAM_HL, ONE_STREAM_SEED,
                                  assert_index_equal, class_block, index_batch, key_passes, long_batch, long_gaps,
                                  long_reference, parse_restated, ragged_reference, replay_restated, sliding_index_restated,
                                  sliding_index_shape, sort_passes, stream_passes)
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from stanford_compression_library_amd.compressors.lz77 import LZ77Sequence
from stanford_compression_library_amd.compressors.lz77_sliding_window import (HashBasedMatchFinder, LZ77SlidingWindowDecoder,
                                                                              LZ77SlidingWindowEncoder)
from stanford_compression_library_amd.core.data_block import DataBlock
from test_gpu_lz77_limits import (SENTINEL, assert_nothing_else_stored, first_stream_that_differs, fresh_out, host_arrays,
                                  per_stream)
from test_gpu_lz77_sliding import FILL, assert_parse_equal, device_params, helper_params

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def block_cap(batch, p):
    """sliding_seq_cap of the longest block of the batch, p = (hl, m, C, W, lazy, mml)"""
    longest = max((len(w) - int(s) for w, s in zip(batch["windows"], batch["start"])), default=0)
    return dev_lz77.sliding_seq_cap(max(longest, 0), p[5])


def parse_into(batch, p, dev, out=None, scratch=None, phases=0, seq_cap=None):
    """sliding_parse_batch of the batch with p = (hl, m, C, W, lazy, mml) -> the ParsedBatch (synchronized)"""
    win = torch.from_numpy(batch["buf"]).to(dev)
    win_off = torch.from_numpy(batch["win_off"]).to(dev)
    start = torch.from_numpy(batch["start"]).to(dev)
    res = dev_lz77.sliding_parse_batch(win, win_off, start, device_params(p), seq_cap or block_cap(batch, p), scratch=scratch,
                                       out=out, phases=phases)
    torch.cuda.synchronize()
    return res


def assert_replay_restores(batch, res, W, dev):
    """sliding_replay_batch of the parse into slots that hold the histories, FILL where the blocks go: every status 0,
    every block whole, and the buffer -- the bytes outside every stream included -- byte for byte"""
    buf, win_off, start = batch["buf"], batch["win_off"], batch["start"].astype(np.int64)
    N, n_streams = len(buf), len(start)
    edge = np.zeros(N + 1, np.int64)
    np.add.at(edge, win_off[:-1] + start, 1)
    np.add.at(edge, win_off[1:], -1)
    slots = buf.copy()
    slots[np.cumsum(edge)[:-1] > 0] = FILL
    assert n_streams == 0 or (slots != buf).any()
    win = torch.from_numpy(slots).to(dev)
    out_len, status = dev_lz77.sliding_replay_batch(win, torch.from_numpy(win_off).to(dev),
                                                    torch.from_numpy(batch["start"]).to(dev), res.literal_count,
                                                    res.match_length, res.match_offset, res.n_seq, res.literals, res.lit_off,
                                                    res.n_lit, window_size=W)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    assert np.array_equal(out_len.cpu().numpy(), np.diff(win_off) - start)
    assert np.array_equal(win.cpu().numpy(), buf)


# ---- the index against its definition ------------------------------------------------------------------------------------------
def check_sliding_index(batch, p, dev):
    """WHITE BOX: runs the parse on a scratch full of 0xA5, reads key[], order[] (the order_a part), rank[] and the bitmap
    at the offsets of sliding_index_shape -- pinned to the library by
    test_lz77_sliding_host.test_restated_sliding_scratch_layout_equals_the_library -- and compares them with
    sliding_index_restated.  Where the parse tests only say "sequences differ", the message names the stage: keys, sort,
    inverse or bitmap."""
    hl, m, C, W, lazy, mml = p
    N, n_streams = len(batch["buf"]), len(batch["windows"])
    sh = sliding_index_shape(N)
    assert sh.total == dev_lz77.sliding_scratch_bytes(N, n_streams)
    scratch = torch.full((sh.total,), FILL, dtype=torch.uint8, device=dev)
    res = parse_into(batch, p, dev, scratch=scratch)
    raw = scratch.cpu().numpy()
    got = (raw[sh.key: sh.key + 4 * N].view(np.uint32), raw[sh.order_a: sh.order_a + 4 * N].view(np.uint32),
           raw[sh.rank: sh.rank + 4 * N].view(np.uint32), raw[sh.bitmap: sh.bitmap + 8 * sh.n_words].view(np.uint64))
    assert_index_equal(got, sliding_index_restated(batch["buf"], batch["win_off"], hl, m, W), N,
                       f"hl={hl} m={m} W={W}, {n_streams} streams")
    return res


@pytest.mark.parametrize("name,hl,m,W,passes", INDEX_CASES, ids=lambda v: str(v))
def test_bucket_index_equals_its_definition(name, hl, m, W, passes, dev):
    """lz77_sliding_keys, lz77_sort_positions over LzKeyDigit and lz77_sliding_bitmap against their definition.
    ragged (130 streams, one stream-number pass): m = 1, 256 -> 2 passes (even: the result arrives in order_a from
    order_b), 257 and 65 536 -> 3, 2^24 + 1 and 2^32 - 1 -> 5; at 256 and 65 536 the positions without a gram sort, inside
    their stream, under the digits of the largest bucket; W = 16 and 50 are shorter than most streams, W = 0 is no bound;
    hl = 1 (every position of a stream has a gram) and hl = 8 (the last seven of a stream have none).
    one (one stream, no stream-number pass; the lead and the tail copy stream content): m = 256 -> ONE pass, and the lead,
    the tail and the stream's last bytes share the digit 0xFF with bucket 255, which the batch holds; m = 2^32 - 1 -> 4.
    edge257 (257 streams, empty ones, two stream-number passes): m = 65 537 and 2^24 -> 5, 2^24 + 1 -> 6.
    tiled (70 000 streams, about 9 MB, more than 256 scan blocks, three stream-number passes): m = 2^24 + 1 -> 7 (odd),
    m = 1 -> 4 (even; every position of a stream in one bucket, so order[] within a stream is the positions in order)."""
    batch = index_batch(name)
    n_streams = len(batch["windows"])
    assert sort_passes(m, n_streams) == key_passes(m) + stream_passes(n_streams) == passes
    if name == "tiled":
        assert n_streams >= 65536 and sliding_index_shape(len(batch["buf"])).n_scan_blocks > 256 and stream_passes(n_streams) == 3
    if name == "one":
        assert n_streams == 1 and stream_passes(1) == 0 and batch["win_off"][0] == 40
    res = check_sliding_index(batch, (hl, m, 64, W, 1, 4), dev)
    assert not res.status.cpu().numpy().any()


# ---- scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [(4, (1 << 24) + 1, 64, 1000000, 1, 4), (3, 1, 2, 40, 1, 3)], ids=str)
def test_tiled_batch_equals_the_restatement_and_replays(p, dev):
    """70 000 streams, about 9 MB: lz77_sliding_keys and lz77_sliding_bitmap over 35 000 workgroups, the sort with 4 + 3 = 7
    passes (m = 2^24 + 1) and 1 + 3 = 4 (m = 1), the carry of the block-sum scan across more than 256 scan blocks, and
    lz77_sliding_parse / lz77_sliding_replay over 17 500 workgroups.  m = 1 with C = 2 and W = 40: every position is a
    bucket-mate, so the chain cap and the window decide.  Identical neighbouring streams share every bucket: a candidate
    taken from the neighbour would show."""
    batch = tiled_batch()
    n_streams, N = len(batch["windows"]), len(batch["buf"])
    assert n_streams >= 65536 and sliding_index_shape(N).n_scan_blocks > 256
    assert (batch["ids"][1:] == batch["ids"][:-1]).any() and sort_passes(p[1], n_streams) == (7 if p[1] > 1 else 4)
    ref = [parse_restated(t, 0, helper_params(p)) for t in batch["templates"]]
    assert sum((seq[:, 1] > 0).sum() for seq, _ in ref) > len(ref)
    res = parse_into(batch, p, dev)
    assert first_stream_that_differs(res, batch, ref) is None
    assert_replay_restores(batch, res, p[3], dev)


# ---- stream-count edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [256, 65537])
@pytest.mark.parametrize("n_streams", [1, 2, 255, 256, 257])
def test_stream_count_edges_with_lookalike_bytes_around(n_streams, m, dev):
    """lz_stream_passes at its edges, crossed with one and three key passes: 1 stream -> 1 and 3 passes (no stream-number
    pass: the lead and the tail sort among the stream's own positions, at m = 256 next to bucket 255), 2 and 255 streams ->
    2 and 4 (the digit n_streams = 255 of the bytes outside still fits one byte), 256 and 257 -> 3 and 5.  A lead that
    copies the start of stream 0, a tail that copies the last stream, identical neighbours and runs of empty streams: the
    parse equals the restatement of every stream on its own, so no candidate comes from the lead, the tail or a neighbour."""
    one = n_streams == 1
    batch = edge_batch(1, ONE_STREAM_SEED) if one else edge_batch(n_streams)
    p = (ONE_STREAM_HL if one else 3, m, 4, 60, 1, 3)
    lens = np.diff(batch["win_off"])
    assert len(lens) == n_streams and batch["win_off"][0] == 40 and len(batch["buf"]) == batch["win_off"][-1] + 40
    assert batch["buf"][:40].tolist() == batch["windows"][0][:40].tolist()
    assert sort_passes(m, n_streams) == {1: 0, 2: 1, 255: 1, 256: 2, 257: 2}[n_streams] + {256: 1, 65537: 3}[m]
    if n_streams >= 8:
        assert (lens[-3:] == 0).all() and (lens[n_streams // 2: n_streams // 2 + 3] == 0).all()
    want = [parse_restated(w, int(s), helper_params(p)) for w, s in zip(batch["windows"], batch["start"])]
    assert sum(int((seq[:, 1] > 0).sum()) for seq, _ in want) >= n_streams
    res = parse_into(batch, p, dev)
    got, status = per_stream(res)
    assert not status.any()
    assert_parse_equal(got, want, f"n_streams={n_streams} m={m}")
    assert_replay_restores(batch, res, p[3], dev)


# ---- one long stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("between", [False, True], ids=["alone", "between"])
@pytest.mark.parametrize("p", LONG_PARAMS, ids=str)
def test_long_stream_equals_the_restatement_and_replays(p, between, dev):
    """One stream of 40 170 bytes, alone (base 1) and between two short streams (base 91).  W = 0, m = 2^32 - 1: three
    literal runs of more than 3 * 4096 bytes, so lz_next_bit walks several of its 64-word steps over clear words, from a
    `from & 63` that is not 0, and finds the match behind; the last match sits at the last position of the range, in the
    word the `to & 63` mask cuts (test_lz77_sliding_host.py asserts all that on the restated bitmap).  W = 1000: repeats 400,
    430, 450 and exactly 1000 back are taken, those 1001 and more than 12 000 back refused.  m = 65 536, W = 5000: thousands
    of bitmap bits from bucket collisions that lead to no match of mml bytes, each a call of lz_sliding_best."""
    batch = long_batch(between)
    s = 1 if between else 0
    assert len(batch["windows"][s]) == LONG_N > 9 * LONG_STEP and batch["win_off"][s] % 2 == 1
    assert (p[3] == 0) == (len(long_gaps(long_reference(p)[0])) == 3)
    want = [long_reference(p) if k == s else parse_restated(w, int(st), helper_params(p))
            for k, (w, st) in enumerate(zip(batch["windows"], batch["start"]))]
    res = parse_into(batch, p, dev)
    got, status = per_stream(res)
    assert not status.any()
    assert_parse_equal(got, want, f"{p}")
    assert_replay_restores(batch, res, p[3], dev)


# ---- through the classes ---------------------------------------------------------------------------------------------------------
def test_block_of_100000_bytes_through_the_classes(dev):
    """LZ77SlidingWindowEncoder with the default match finder, window_size = 1000 and an initial window of 1500 bytes: the
    coder keeps the last 1000, scl_lz77_sliding_parse_host parses 101 000 bytes on one wavefront, and the sequences equal
    the restatement; encode_block -> decode_block returns the block"""
    history, block = class_block()
    assert len(history) > 1000 and len(block) == 100000
    want_seq, want_lit = parse_restated(np.concatenate([history[-1000:], block]), 1000, (4, 1000000, 64, 1, 4, 1000))
    enc = LZ77SlidingWindowEncoder(HashBasedMatchFinder(), window_size=1000, initial_window=history.tolist())
    sequences, literals = enc.lz77_parse_and_generate_sequences(block.tolist())
    assert sequences == [LZ77Sequence(*row) for row in want_seq.tolist()]
    assert literals == want_lit.tolist()
    bits = LZ77SlidingWindowEncoder(HashBasedMatchFinder(), window_size=1000,
                                    initial_window=history.tolist()).encode_block(DataBlock(block.tolist()))
    back, used = LZ77SlidingWindowDecoder(window_size=1000, initial_window=history.tolist()).decode_block(bits)
    assert used == len(bits) and np.array_equal(np.array(back.data_list, np.uint8), block)


# ---- phases, scratch=, out= ------------------------------------------------------------------------------------------------------
def test_index_and_parse_in_two_calls_on_a_used_scratch(dev):
    """scl_lz77_sliding_parse_batch with phases = SCL_LZ77_INDEX, then SCL_LZ77_PARSE, on a scratch that the larger ragged
    batch has filled (the layout of the small batch puts every part elsewhere, over the large one's leftovers) and into an
    `out=` that holds an earlier result: the index call stores no result, the parse call finds the index of the call
    before, and nothing depends on what scratch or result held."""
    big, small = ragged_batch(), edge_batch(257)
    p_big, p_first, p = (4, 1000000, 64, 1000000, 1, 4), (3, 1000, 4, 60, 1, 3), (3, 65537, 2, 25, 0, 3)
    scratch = torch.full((dev_lz77.sliding_scratch_bytes(len(big["buf"]), 130),), FILL, dtype=torch.uint8, device=dev)
    assert scratch.numel() > 4 * dev_lz77.sliding_scratch_bytes(len(small["buf"]), 257)
    got, status = per_stream(parse_into(big, p_big, dev, scratch=scratch))
    assert not status.any()
    assert_parse_equal(got, ragged_reference(helper_params(p_big)), "the large batch")
    restated = lambda q: [parse_restated(w, int(s), helper_params(q)) for w, s in zip(small["windows"], small["start"])]  # noqa: E731
    cap = block_cap(small, p)
    assert cap == block_cap(small, p_first)
    out = fresh_out(small, cap, dev)
    got, status = per_stream(parse_into(small, p_first, dev, out=out, scratch=scratch))  # an earlier result
    assert not status.any()
    assert_parse_equal(got, restated(p_first), "the small batch, one call")
    want = restated(p)
    assert any(a[0].tolist() != b[0].tolist() for a, b in zip(want, got))
    before = [a.copy() for a in host_arrays(out)]
    res = parse_into(small, p, dev, out=out, scratch=scratch, phases=backend_lib.LZ77_INDEX)
    assert res is out and all(np.array_equal(a, b) for a, b in zip(before, host_arrays(out))), "the index call stored a result"
    res = parse_into(small, p, dev, out=out, scratch=scratch, phases=backend_lib.LZ77_PARSE)
    got, status = per_stream(res)
    assert not status.any()
    assert_parse_equal(got, want, "the small batch, two calls")
    one_call, status = per_stream(parse_into(small, p, dev))
    assert not status.any()
    assert_parse_equal(got, one_call, "two calls against one")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusal_batch():
    rng = np.random.default_rng(8)
    windows = [rng.integers(0, 3, n).astype(np.uint8) for n in (60, 0, 75, 130, 64)]
    return pack_windows(windows, [0, 0, 5, 0, 0])


def test_a_last_stream_that_ends_past_the_buffer_is_refused_alone(dev):
    """win_off[n_streams] > N: lz77_sliding_parse answers SCL_ST_SIZE for the last stream and stores nothing for it;
    lz77_sliding_keys clamps that stream's end to N, so the index is the definition's, and every other stream is parsed
    as if nothing were wrong"""
    batch = refusal_batch()
    p = (3, 257, 64, 40, 1, 3)
    batch["win_off"] = batch["win_off"].copy()
    batch["win_off"][-1] += 5
    assert batch["win_off"][-1] > len(batch["buf"]) > batch["win_off"][-2]
    want = [parse_restated(w, int(s), helper_params(p)) for w, s in zip(batch["windows"], batch["start"])]
    assert all((seq[:, 1] > 0).any() for seq, _ in want[2:])
    scratch = torch.full((dev_lz77.sliding_scratch_bytes(len(batch["buf"]), 5),), FILL, dtype=torch.uint8, device=dev)
    cap = block_cap(batch, p)
    res = parse_into(batch, p, dev, out=fresh_out(batch, cap, dev), scratch=scratch)
    got, status = per_stream(res)
    assert status.tolist() == [0, 0, 0, 0, ST_SIZE]
    assert len(got[4][0]) == 0 and len(got[4][1]) == 0
    assert_parse_equal(got[:4], want[:4])
    assert_nothing_else_stored(res)
    N, sh = len(batch["buf"]), sliding_index_shape(len(batch["buf"]))
    raw = scratch.cpu().numpy()
    index = (raw[sh.key: sh.key + 4 * N].view(np.uint32), raw[sh.order_a: sh.order_a + 4 * N].view(np.uint32),
             raw[sh.rank: sh.rank + 4 * N].view(np.uint32), raw[sh.bitmap: sh.bitmap + 8 * sh.n_words].view(np.uint64))
    restated = sliding_index_restated(batch["buf"], batch["win_off"], p[0], p[1], p[3])
    assert (restated[0][batch["win_off"][-2]: N - p[0] + 1] != 0xFFFFFFFF).all()  # keys up to the clamped end
    assert_index_equal(index, restated, N, "a last stream past the buffer")


def test_a_stream_that_starts_behind_its_end_is_refused_alone(dev):
    """start[s] > the stream's length: SCL_ST_SIZE for that stream alone, its sequence row and the literal buffer keep their
    sentinels, the streams around it equal the restatement"""
    batch = refusal_batch()
    p = (3, 257, 64, 40, 1, 3)
    batch["start"] = batch["start"].copy()
    batch["start"][2] = len(batch["windows"][2]) + 3
    want = [parse_restated(w, int(s), helper_params(p)) for w, s in zip(batch["windows"], batch["start"])]
    res = parse_into(batch, p, dev, out=fresh_out(batch, dev_lz77.sliding_seq_cap(130, p[5]), dev))
    got, status = per_stream(res)
    assert status.tolist() == [0, 0, ST_SIZE, 0, 0]
    assert len(got[2][0]) == 0 and len(got[2][1]) == 0
    rows = host_arrays(res)[0]
    assert (rows[:, 2, :] == SENTINEL).all()
    for s in (0, 1, 3, 4):
        assert_parse_equal(got[s: s + 1], want[s: s + 1], f"stream {s}")
    assert_nothing_else_stored(res)


def test_replay_refuses_counts_and_offsets_beyond_its_buffers(dev):
    """the SCL_ST_SIZE exit of lz77_sliding_replay: n_seq[s] > seq_cap, have[s] > the slot's size, lit_off[s] > lit_bytes
    and n_lit[s] > lit_bytes - lit_off[s] each refuse that stream alone -- out_len 0, the slot untouched -- and the
    streams between them are replayed"""
    n, slot, W = 9, 40, 8
    history = (np.arange(10) * 7 % 5).astype(np.uint8)
    seqs, lits = [(2, 3, 2), (1, 4, 8)], [7, 8, 9]
    new, st = replay_restated(history, seqs, lits, window_size=W, cap=slot)
    assert st == 0 and len(new) == 10
    slots = pack_windows([np.concatenate([history, np.full(slot - 10, FILL, np.uint8)])] * n, [10] * n,
                         lead=np.full(3, 0x77, np.uint8), tail=np.full(5, 0x77, np.uint8))
    seq_cap, lit_bytes = 3, 3 * n
    rows = np.zeros((3, n, seq_cap), np.int64)
    rows[:, :, :2] = np.array(seqs, np.int64).T[:, None, :]
    have, n_seq = np.full(n, 10, np.int64), np.full(n, 2, np.int64)
    lit_off, n_lit = 3 * np.arange(n, dtype=np.int64), np.full(n, 3, np.int64)
    n_seq[1] = seq_cap + 1
    have[3] = slot + 1
    lit_off[5] = lit_bytes + 1
    lit_off[7], n_lit[7] = lit_bytes - 2, 3
    bad = [1, 3, 5, 7]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)  # noqa: E731
    win = t(slots["buf"], np.uint8)
    out_len, status = dev_lz77.sliding_replay_batch(
        win, t(slots["win_off"], np.int64), t(have, np.int32), t(rows[0], np.int32), t(rows[1], np.int32),
        t(rows[2], np.int32), t(n_seq, np.int32), t(np.tile(np.array(lits, np.uint8), n), np.uint8), t(lit_off, np.int64),
        t(n_lit, np.int32), window_size=W)
    torch.cuda.synchronize()
    expect = slots["buf"].copy()
    for s in range(n):
        if s not in bad:
            at = int(slots["win_off"][s]) + 10
            expect[at: at + len(new)] = new
    assert status.cpu().numpy().tolist() == [ST_SIZE if s in bad else 0 for s in range(n)]
    assert out_len.cpu().numpy().tolist() == [0 if s in bad else len(new) for s in range(n)]
    assert np.array_equal(win.cpu().numpy(), expect)


# ---- the host calls on nothing -------------------------------------------------------------------------------------------------------
def test_host_calls_on_nothing(dev):
    """scl_lz77_sliding_parse_host with n = 0 (no index kernels, lz77_sliding_parse on an empty window) and with start == n
    (an index, and a parse that begins at the end); scl_lz77_sliding_replay_host with no sequences and no literals,
    without and with a history"""
    for window, start in ((np.zeros(0, np.uint8), 0), (np.arange(50, dtype=np.uint8) % 3, 50)):
        lc, ml, mo, lit = dev_lz77.sliding_parse_host(window, start)
        assert lc.size == 0 and ml.size == 0 and mo.size == 0 and lit.size == 0
    none = np.zeros(0, np.uint32)
    for history in (np.zeros(0, np.uint8), np.arange(10, dtype=np.uint8)):
        for W in (0, 4):
            back = dev_lz77.sliding_replay_host(history, none, none, none, np.zeros(0, np.uint8), window_size=W)
            assert back.dtype == np.uint8 and back.size == 0
