"""Sliding-window LZ77 without a GPU: the bucket function, the restated rule against the reference's goldens, the wrong
variants the goldens tell apart, the window class, the parameters the C ABI refuses, and a user's own match finder."""
import ctypes

import numpy as np
import pytest

from lz77_helpers import use_host_prefix_coder
from lz77_sliding_helpers import (VARIANTS, bucket, case_params, golden_blocks, goldens, parse_restated, replay_restated)
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev
from stanford_compression_library_amd.compressors.lz77 import LZ77StreamsDecoder
from stanford_compression_library_amd.compressors.lz77_sliding_window import (HashBasedMatchFinder, LZ77SlidingWindowEncoder,
                                                                              LZ77Window, MatchFinderBase)
from stanford_compression_library_amd.core.data_block import DataBlock

SLIDING = [c for c in goldens() if c.kind == "sliding"]


def test_bucket_is_the_interpreters_tuple_hash_and_the_librarys():
    rng = np.random.default_rng(1)
    for _ in range(4000):
        hl = int(rng.integers(1, 9))
        m = int(rng.choice([1, 2, 3, 255, 256, 257, 65536, 1000000, (1 << 31) + 11, (1 << 32) - 1]))
        gram = rng.integers(0, 256, hl).astype(np.uint8)
        if rng.random() < 0.2:
            gram[:] = rng.choice([0, 255])
        want = hash(tuple(gram.tolist())) % m
        assert bucket(gram.tolist(), m) == want
        assert dev.sliding_bucket(gram, m) == want


def test_golden_file_holds_the_cases_of_the_design():
    groups = {c.group for c in goldens()}
    assert {"grid", "word_text", "long_run", "short_block", "short_block_with_window", "long_initial_window",
            "blocks_then_reset", "mml", "ladder", "encode_file"} <= groups
    grid = [c for c in SLIDING if c.group == "grid"]
    assert len(grid) == 48 and {(c.W, c.m, c.C, c.hl) for c in grid} == {
        (W, m, C, hl) for W in (16, 100, 100000) for m in (1, 3, 1000000) for C in (2, 64) for hl in (2, 4)}
    assert any(len(c.arr("init")) > c.W for c in SLIDING if c.group == "long_initial_window")
    assert any(int(c.arr("b0_seq")[:, 1].max()) > c.W for c in SLIDING if c.group == "long_run")


@pytest.mark.parametrize("case", SLIDING, ids=repr)
def test_restated_rule_gives_the_goldens(case):
    for window, data, seq, lit, _, _, _ in golden_blocks(case):
        got_seq, got_lit = parse_restated(np.concatenate([window, data]), len(window), case_params(case))
        assert np.array_equal(got_seq, seq) and np.array_equal(got_lit, lit)
        back, status = replay_restated(window, seq, lit, window_size=case.W)
        assert status == 0 and np.array_equal(back, data)


@pytest.mark.parametrize("variant", VARIANTS)
def test_goldens_tell_the_wrong_variants_apart(variant):
    differing = 0
    for case in SLIDING:
        for window, data, seq, lit, _, _, _ in golden_blocks(case):
            got_seq, got_lit = parse_restated(np.concatenate([window, data]), len(window), case_params(case), variant)
            if not (np.array_equal(got_seq, seq) and np.array_equal(got_lit, lit)):
                differing += 1
                break
    assert differing >= 1, f"no golden case tells the variant '{variant}' from the rule"


def test_ladder_walks_lazily_past_a_wavefront_of_steps():
    lazy, greedy = [c for c in SLIDING if c.group == "ladder"]
    assert lazy.lazy and not greedy.lazy
    window, data, seq, _, _, _, _ = golden_blocks(lazy)[0]
    assert seq[0].tolist()[:2] == [79, 83]
    walks = []
    parse_restated(np.concatenate([window, data]), len(window), case_params(lazy), walks=walks)
    assert walks[0] == 79 and walks[0] > 64
    assert golden_blocks(greedy)[0][2][0].tolist()[:2] == [0, 4]


def test_window_keeps_the_last_bytes_by_absolute_position():
    w = LZ77Window(4)
    for b in (65, 66, 67):
        w.append(b)
    assert (w.start, w.end, w.size) == (0, 3, 4) and w.get_byte(1) == 66 and w.get_window_as_list() == [65, 66, 67]
    w.append(68)
    w.append(69)
    assert (w.start, w.end) == (1, 5) and w.get_byte(4) == 69 and w.get_window_as_list() == [66, 67, 68, 69]
    assert w.get_byte_window_plus_lookahead(4, [1, 2]) == 69 and w.get_byte_window_plus_lookahead(6, [1, 2]) == 2
    for outside in (0, 5):
        with pytest.raises(IndexError):
            w.get_byte(outside)
    long = LZ77Window(3, initial_window=[1, 2, 3, 4, 5])
    assert (long.start, long.end) == (2, 5) and long.get_window_as_list() == [3, 4, 5]


def _parse_host_rc(hl=4, m=1000000, C=64, mml=4, window=b"abcdabcd"):
    L = backend_lib.load()
    buf = np.frombuffer(window, np.uint8).copy()
    cap = len(buf) + 2
    seq = np.zeros((3, cap), np.uint32)
    lit = np.zeros(len(buf), np.uint8)
    n_seq, n_lit = ctypes.c_uint64(0), ctypes.c_uint64(0)
    return L.scl_lz77_sliding_parse_host(backend_lib.u8_ptr(buf), len(buf), 0, hl, m, C, 1, mml, 100,
                                         backend_lib.u32_ptr(seq[0]), backend_lib.u32_ptr(seq[1]), backend_lib.u32_ptr(seq[2]),
                                         cap, ctypes.byref(n_seq), backend_lib.u8_ptr(lit), len(buf), ctypes.byref(n_lit))


@pytest.mark.parametrize("bad, word", [(dict(hl=0), "hash_length"), (dict(hl=9), "hash_length"),
                                       (dict(m=0), "hash_table_size"), (dict(m=1 << 32), "hash_table_size"),
                                       (dict(C=0), "max_chain_length"), (dict(C=65), "max_chain_length"),
                                       (dict(mml=0), "min_match_length")])
def test_refused_parameters_are_e_param_before_any_device_call(bad, word):
    assert _parse_host_rc(**bad) == backend_lib.E_PARAM
    assert backend_lib.last_error().startswith("lz77_sliding_parse_host:") and word in backend_lib.last_error()
    a = backend_lib.Lz77SlidingParseArgs(256, 256, 256, 1, 8, 1000000, 4, 64, 1, 4, 100, 4, 0, 0, 256, 256, 256, 256, 256, 256,
                                         256, 256, 1 << 20)
    a.hash_length, a.hash_table_size = bad.get("hl", 4), bad.get("m", 1000000)
    a.max_chain_length, a.min_match_length = bad.get("C", 64), bad.get("mml", 4)
    assert backend_lib.load().scl_lz77_sliding_parse_batch(ctypes.byref(a), None) == backend_lib.E_PARAM
    assert word in backend_lib.last_error()


def test_null_pointers_and_bad_scratch_are_e_param_before_any_device_call():
    L = backend_lib.load()
    fields = [f for f, _ in backend_lib.Lz77SlidingParseArgs._fields_]

    def args(**over):
        a = backend_lib.Lz77SlidingParseArgs(256, 256, 256, 1, 8, 1000000, 4, 64, 1, 4, 100, 4, 0, 0, 256, 256, 256, 256,
                                             256, 256, 256, 256, 1 << 20)
        for k, v in over.items():
            assert k in fields
            setattr(a, k, v)
        return a

    assert L.scl_lz77_sliding_parse_batch(None, None) == backend_lib.E_PARAM
    for name in ("d_win", "d_win_off", "d_start", "d_lit_count", "d_match_len", "d_match_off", "d_literals", "d_n_seq",
                 "d_n_lit", "d_status", "d_scratch"):
        assert L.scl_lz77_sliding_parse_batch(ctypes.byref(args(**{name: None})), None) == backend_lib.E_PARAM, name
        assert "null pointer" in backend_lib.last_error()
    need = dev.sliding_scratch_bytes(8, 1)
    assert need > dev.scratch_bytes(8, 1)  # the greedy index's parts and the keys
    assert L.scl_lz77_sliding_parse_batch(ctypes.byref(args(scratch_bytes=need - 1)), None) == backend_lib.E_PARAM
    assert L.scl_lz77_sliding_parse_batch(ctypes.byref(args(d_scratch=257)), None) == backend_lib.E_PARAM
    assert "scl_lz77_sliding_scratch_bytes" in backend_lib.last_error()
    r = backend_lib.Lz77SlidingReplayArgs(256, 256, 256, 1, 8, 4, 100, 256, 256, 256, 256, 256, 8, 256, 256, 256, 256)
    r.d_status = None
    assert L.scl_lz77_sliding_replay_batch(ctypes.byref(r), None) == backend_lib.E_PARAM
    out_len = ctypes.c_uint64(0)
    assert L.scl_lz77_sliding_replay_host(None, 0, 8, 0, None, None, None, 1, None, 0, ctypes.byref(out_len)) \
        == backend_lib.E_PARAM


def test_classes_name_the_limit_they_refuse():
    for kwargs, word in ((dict(hash_length=9), "hash_length"), (dict(hash_table_size=1 << 32), "hash_table_size"),
                         (dict(max_chain_length=65), "max_chain_length"), (dict(minimum_match_length=0), "minimum_match_length")):
        with pytest.raises(NotImplementedError, match=word):
            HashBasedMatchFinder(**kwargs)
    finder = HashBasedMatchFinder(hash_length=3, hash_table_size=1000)
    assert finder._hash([7, 8, 9, 10]) == hash((7, 8, 9)) % 1000
    assert dev.sliding_seq_cap(10, 4) == 4 and dev.sliding_seq_cap(0, 4) == 2
    assert dev.sliding_kernel_names() == ("lz77_sort_scatter", "lz77_sliding_parse", "lz77_sliding_replay")


class NewestPairFinder(MatchFinderBase):
    """a finder of the user's own: the newest earlier occurrence of the next two bytes, scanned for, right-extended only"""

    def find_best_match(self, lookahead_buffer):
        for i in range(len(lookahead_buffer) - 1):
            pair = list(lookahead_buffer[i:i + 2])
            for pos in range(self.window.end + i - 1, self.window.start - 1, -1):
                if [self.window.get_byte_window_plus_lookahead(pos + k, lookahead_buffer) for k in range(2)] == pair:
                    lits, pos, length = self.extend_match(i, pos, lookahead_buffer, left_extension=False)
                    return lits, pos, length
        return len(lookahead_buffer), 0, 0


def test_a_users_match_finder_runs_the_host_loop_and_round_trips(monkeypatch):
    use_host_prefix_coder(monkeypatch)
    rng = np.random.default_rng(3)
    init = [1, 2, 3, 1, 2]
    enc = LZ77SlidingWindowEncoder(NewestPairFinder(), window_size=32, initial_window=init)
    history = np.array(init, np.uint8)
    for n in (0, 1, 90, 40):
        data = rng.integers(0, 3, n).astype(np.uint8)
        bits = enc.encode_block(DataBlock(data.tolist()))
        (sequences, literals), used = LZ77StreamsDecoder().decode_block(bits)
        assert used == len(bits)
        seq = np.array([[s.literal_count, s.match_length, s.match_offset] for s in sequences], np.int64).reshape(-1, 3)
        assert n < 10 or (seq[:, 1] > 0).sum() > 3
        back, status = replay_restated(history, seq, literals, window_size=32)
        assert status == 0 and np.array_equal(back, data)
        history = np.concatenate([history, data])[-32:]
        assert enc.window.get_window_as_list() == history.tolist()
