"""The wide LZ77 path, host side (no GPU): the C ABI refuses bad arguments before it touches a device, the shape and
scratch-size functions behave, and the fixtures of tests/test_gpu_lz77_wide.py are what they claim to be -- every planted
edge produces the intended match at the intended place under lz77_helpers.parse_restated, and the pure-Python restatement
of the scheme (lz77_wide_helpers.parse_wide_restated / replay_wide_restated) equals parse_restated / replay_restated on all
of them."""
import ctypes

import numpy as np
import pytest

from lz77_helpers import ST_CAPACITY, markov1_long_stream, markov1_stream, parse_restated, replay_restated
from lz77_wide_helpers import (all_cases, cap_cases, damage_cases, parse_wide_restated, reference, replay_wide_restated,
                               sequence_positions, tile_cases)
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77

T, C = dev_lz77.wide_shape()
CASES = all_cases(T, C)


def test_shape_threshold_and_names():
    assert T <= C and T & (T - 1) == 0 and C & (C - 1) == 0 and T >= 64
    assert dev_lz77.wide_threshold() >= T
    names = dev_lz77.wide_kernel_names()
    assert len(names) == 3 and all(name.startswith("lz77w_") for name in names)
    blob = open(backend_lib.LIB_PATH, "rb").read()
    assert all(name.encode() in blob for name in names)


def test_scratch_sizes_are_monotone():
    L = backend_lib.load()
    sizes = [L.scl_lz77_wide_scratch_bytes(n) for n in (0, 1, T - 1, T, T + 1, 4096, 4097, 1 << 20, 1 << 24)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert all(size > L.scl_lz77_scratch_bytes(n, 1) for size, n in zip(sizes, (0, 1, T - 1, T, T + 1, 4096, 4097, 1 << 20)))
    assert sizes[-2] >= (3 + 3) * 4 * (1 << 20)  # the index, and three words per position for the tables
    assert dev_lz77.wide_scratch_bytes(4097) == sizes[6]
    grid = [[L.scl_lz77_wide_replay_scratch_bytes(k, g) for g in (0, 1, 4096, 1 << 20)] for k in (0, 1, 2048, 2049, 1 << 20)]
    assert grid[0][0] > 0 and all(row == sorted(row) for row in grid) and all(list(col) == sorted(col) for col in zip(*grid))
    assert grid[-1][-1] >= 16 * (1 << 20) + 4 * (1 << 20)
    assert dev_lz77.wide_replay_scratch_bytes(2049, 4096) == grid[3][2]


def _parse_args(**over):
    one = 0x1000  # never dereferenced: validation comes first
    fields = dict(d_win=one, n=64, start=0, min_match_length=6, max_matches=64, seq_cap=8, d_lit_count=one, d_match_len=one,
                  d_match_off=one, d_literals=one, d_n_seq=one, d_n_lit=one, d_status=one, d_scratch=one << 8,
                  scratch_bytes=1 << 30)
    fields.update(over)
    return backend_lib.Lz77WideParseArgs(**fields)


def _replay_args(**over):
    one = 0x1000
    fields = dict(d_win=one, have=4, cap=64, d_lit_count=one, d_match_len=one, d_match_off=one, n_seq=3, d_literals=one,
                  n_lit=5, d_out_len=one, d_status=one, d_scratch=one << 8, scratch_bytes=1 << 30)
    fields.update(over)
    return backend_lib.Lz77WideReplayArgs(**fields)


def test_parse_wide_refuses_bad_arguments_before_any_device_call():
    L, E = backend_lib.load(), backend_lib.E_PARAM
    assert L.scl_lz77_parse_wide(None, None) == E and backend_lib.last_error().startswith("lz77_parse_wide:")
    for name in ("d_win", "d_lit_count", "d_match_len", "d_match_off", "d_literals", "d_n_seq", "d_n_lit", "d_status",
                 "d_scratch"):
        assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(**{name: None})), None) == E, name
        assert "null pointer" in backend_lib.last_error()
    for bad in (0, 9, 1 << 31):
        assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(min_match_length=bad)), None) == E
        assert "1 <= L <= 8" in backend_lib.last_error()
    for bad in (0, 65, 1 << 31):
        assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(max_matches=bad)), None) == E
        assert "1 <= M <= 64" in backend_lib.last_error()
    assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(n=1 << 32)), None) == E and "2^32" in backend_lib.last_error()
    assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(start=65)), None) == E
    assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(d_scratch=0x100010)), None) == E  # misaligned
    assert "256-byte aligned" in backend_lib.last_error()
    short = L.scl_lz77_wide_scratch_bytes(64) - 1
    assert L.scl_lz77_parse_wide(ctypes.byref(_parse_args(scratch_bytes=short)), None) == E
    assert "scl_lz77_wide_scratch_bytes" in backend_lib.last_error()


def test_replay_wide_refuses_bad_arguments_before_any_device_call():
    L, E = backend_lib.load(), backend_lib.E_PARAM
    assert L.scl_lz77_replay_wide(None, None) == E and backend_lib.last_error().startswith("lz77_replay_wide:")
    for name in ("d_win", "d_lit_count", "d_match_len", "d_match_off", "d_literals", "d_out_len", "d_status", "d_scratch"):
        assert L.scl_lz77_replay_wide(ctypes.byref(_replay_args(**{name: None})), None) == E, name
        assert "null pointer" in backend_lib.last_error()
    for over in (dict(cap=1 << 32), dict(have=65), dict(n_seq=1 << 32), dict(n_lit=1 << 32)):
        assert L.scl_lz77_replay_wide(ctypes.byref(_replay_args(**over)), None) == E, over
        assert "2^32" in backend_lib.last_error()
    assert L.scl_lz77_replay_wide(ctypes.byref(_replay_args(d_scratch=0x100010)), None) == E
    short = L.scl_lz77_wide_replay_scratch_bytes(3, 60) - 1
    assert L.scl_lz77_replay_wide(ctypes.byref(_replay_args(scratch_bytes=short)), None) == E
    assert "scl_lz77_wide_replay_scratch_bytes" in backend_lib.last_error()


# ---- the fixtures of the GPU tests ---------------------------------------------------------------------------------------------
def test_case_names_are_unique_and_windows_small():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) and len(names) >= 50
    assert all(len(c["window"]) <= 8 * T + 3 * C for c in CASES)


@pytest.mark.parametrize("case", cap_cases(T, C) + tile_cases(T, C), ids=lambda c: c["name"])
def test_every_planted_edge_is_in_the_parse(case):
    seqs, _ = reference(T, C)[case["name"]]
    got = sequence_positions(seqs, case["start"])
    assert case["expect"] and all(e in got for e in case["expect"]), (case["expect"], got)


def test_the_planted_edges_lie_where_the_kernel_has_its_edges():
    by_name = {c["name"]: c for c in CASES}
    lengths = sorted(by_name[f"match{m}"]["expect"][0][1] for m in (C - 1, C, C + 1))
    assert lengths == [C - 1, C, C + 1] and by_name["older" + str(C)]["expect"][1][1] == C
    ends = [sum(by_name[f"ends-at-tile-end{d:+d}"]["expect"][0]) - 2 * T for d in (-1, 0, 1)]
    assert ends == [-1, 0, 1]
    p, m = by_name["enters-at-a-last-position"]["expect"][0]
    assert (p + m) % T == T - 1 and (p + m) // T > p // T
    p, m = by_name["tiles-without-entry"]["expect"][0]
    assert (p + m) // T - p // T >= 3
    w = by_name["long-to-the-last-byte"]
    assert sum(w["expect"][0]) == len(w["window"]) and w["expect"][0][1] >= C
    w = by_name["short-of-the-cap-at-the-window-end"]
    assert sum(w["expect"][0]) == len(w["window"]) and w["expect"][0][1] < C
    p, m = by_name["literal-run-over-three-tiles"]["expect"][0]
    seqs, _ = reference(T, C)["literal-run-over-three-tiles"]
    assert seqs[0, 0] >= 3 * T + T // 2 and p // T == 4
    (p1, m1), (p2, m2) = by_name["entry-is-long"]["expect"]
    assert p1 + m1 == p2 and p2 // T == p1 // T + 1 and m2 >= C


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_the_restated_scheme_equals_the_rule(case):
    want_seq, want_lit = reference(T, C)[case["name"]]
    seq, lit, status, info = parse_wide_restated(case["window"], case["start"], case["L"], case["M"], T, C)
    assert status == 0 and seq.tolist() == want_seq.tolist() and lit.tolist() == want_lit.tolist()
    if case["name"] == "tiles-without-entry":
        assert info["skipped"] >= 2 and info["resolved"]
    if case["name"] in ("entry-is-long", "long-to-the-last-byte", f"match{C}", f"match{C + 1}", f"older{C}"):
        assert info["resolved"], "the case is there for a LONG position on the chain"
    if case["name"] in (f"match{C - 1}", f"older{C - 1}", "short-of-the-cap-at-the-window-end"):
        assert not info["resolved"]
    if len(want_seq) >= 2:  # one sequence too few: what the one-wave kernel leaves (the first seq_cap sequences and their runs)
        cap = len(want_seq) - 1
        seq, lit, status, _ = parse_wide_restated(case["window"], case["start"], case["L"], case["M"], T, C, seq_cap=cap)
        n_lit = int(want_seq[:cap, 0].sum())
        assert status == ST_CAPACITY and seq.tolist() == want_seq[:cap].tolist() and lit.tolist() == want_lit[:n_lit].tolist()
    back, status, _ = replay_wide_restated(case["window"][: case["start"]], want_seq, want_lit)
    assert status == 0 and back.tolist() == case["window"][case["start"]:].tolist()


def test_the_restated_replay_names_the_faults_as_the_rule_does():
    case = next(c for c in CASES if c["name"] == "markov-L6-M64")
    seqs, lits = reference(T, C)[case["name"]]
    hist = np.arange(10, dtype=np.uint8)
    damaged = damage_cases(seqs, lits, len(hist))
    assert len(damaged) == 16 and len({name for name, _, _ in damaged}) == 16
    seen = set()
    for name, bad, cap in damaged:
        want, want_status = replay_restated(hist, bad, lits, cap)
        got, status, _ = replay_wide_restated(hist, bad, lits, cap)
        assert want_status != 0 and status == want_status and got.tolist() == want.tolist(), name
        seen.add(want_status)
    assert len(seen) == 3  # ST_STATE, ST_TRUNCATED, ST_CAPACITY
    deep_seq, deep_lit = reference(T, C)["markov-L1-M1"]
    back, status, rounds = replay_wide_restated([], deep_seq, deep_lit)
    assert status == 0 and back.tolist() == next(c for c in CASES if c["name"] == "markov-L1-M1")["window"].tolist()
    assert rounds >= 3, "the deepest copy chains of the suite"


def test_the_long_markov_source_is_the_markov_source():
    """test_gpu_lz77_wide.py draws its 1 MiB window from markov1_long_stream: the same bytes, past a piece border too"""
    n = (1 << 16) + 4097
    assert np.array_equal(markov1_long_stream(n, 17), markov1_stream(n, 17))
    assert np.array_equal(markov1_long_stream(300, 3), markov1_stream(300, 3))
