"""The wide sliding-window LZ77 path without a GPU: the scheme restated in lz77_sliding_wide_helpers --
speculate, walk, emit -- gives the rule's parse, sequence for sequence and literal for literal, on every fixture and on
the reference's own goldens; every fixture has the edge it is named for, so that no GPU test silently misses its path; and
the new entry points refuse bad arguments before any device call."""
import ctypes

import numpy as np
import pytest

from lz77_sliding_helpers import case_params, golden_blocks, goldens, parse_restated
from lz77_sliding_wide_helpers import DONE, OPEN, WALK, all_cases, check_edges, reference, scheme_restated
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev

SMALL_SHAPE = (256, 64)
SLIDING = [c for c in goldens() if c.kind == "sliding"]


def library_shape():
    return dev.sliding_wide_shape()


def _check(case, S, CAP):
    want_seq, want_lit = reference(S, CAP)[case["name"]]
    seq, lit, info = scheme_restated(case["window"], case["start"], case["params"], S, CAP)
    assert seq.tolist() == want_seq.tolist(), case["name"]
    assert lit.tolist() == want_lit.tolist(), case["name"]
    check_edges(case, want_seq, info, S)
    return info


@pytest.mark.parametrize("name", [c["name"] for c in all_cases(*SMALL_SHAPE)])
def test_scheme_gives_the_rule_at_a_small_shape(name):
    _check({c["name"]: c for c in all_cases(*SMALL_SHAPE)}[name], *SMALL_SHAPE)


def test_scheme_gives_the_rule_at_the_library_shape():
    S, CAP = library_shape()
    infos = {c["name"]: _check(c, S, CAP) for c in all_cases(S, CAP)}
    # the paths the GPU tests rely on, at the shape the kernels have
    assert OPEN not in infos["markov-defaults"].state.values() or infos["markov-defaults"].computed
    nomatch = infos["nomatch-defaults"]
    # one sequence over all segments (and the last hl - 1 bytes behind it)
    assert nomatch.state[0] == WALK and nomatch.computed[0] == 0 and not set(nomatch.entry) & {1, 2}
    assert set(infos["equal-defaults"].entry) == {0}
    assert any(len(i.computed) > 0 and DONE in i.state.values() for i in infos.values())


@pytest.mark.parametrize("shape", [SMALL_SHAPE, "library"], ids=["small", "library"])
def test_the_walk_resynchronises_on_every_source(shape):
    """a chain that enters a segment off its speculated orbit meets it after a few sequences (the merging the scheme's
    speed rests on; its exactness does not)"""
    S, CAP = library_shape() if shape == "library" else shape
    by_name = {c["name"]: c for c in all_cases(S, CAP)}
    for name in ("markov-defaults", "text-defaults", "random4-defaults", "markov-nonlazy", "markov-small"):
        c = by_name[name]
        seq, _, info = scheme_restated(c["window"], c["start"], c["params"], S, CAP)
        assert len(info.computed) < len(seq) / 2, (name, len(info.computed), len(seq))


@pytest.mark.parametrize("case", SLIDING, ids=repr)
def test_scheme_gives_the_goldens(case):
    for window, data, seq, lit, _, _, _ in golden_blocks(case):
        for S, CAP in (SMALL_SHAPE, (64, 16)):
            got_seq, got_lit, _ = scheme_restated(np.concatenate([window, data]), len(window), case_params(case), S, CAP)
            assert np.array_equal(got_seq, seq) and np.array_equal(got_lit, lit), (S, CAP)


def test_ladder_fixture_walks_lazily_past_a_wavefront_of_steps():
    S, CAP = library_shape()
    ladder = {c["name"]: c for c in all_cases(S, CAP)}["ladder"]
    walks = []
    parse_restated(ladder["window"], ladder["start"], ladder["params"], walks=walks)
    assert walks[0] > 64


def test_shape_threshold_scratch_and_names():
    S, CAP = library_shape()
    assert S >= 64 and S & (S - 1) == 0 and CAP >= 8
    assert dev.sliding_wide_threshold() >= S
    n = 1 << 20
    per_byte = dev.sliding_wide_scratch_bytes(n) / n
    assert dev.sliding_wide_scratch_bytes(n) > dev.sliding_scratch_bytes(n, 1) + 13 * n and 29 < per_byte < 30
    assert dev.sliding_wide_kernel_names() == ("lz77sw_speculate", "lz77sw_walk", "lz77sw_emit")


def _parse_args(**over):
    a = backend_lib.Lz77SlidingWideParseArgs(256, 8, 0, 1000000, 4, 64, 1, 4, 100, 4, 0, 0, 256, 256, 256, 256, 256, 256, 256,
                                             256, 1 << 20)
    fields = [f for f, _ in backend_lib.Lz77SlidingWideParseArgs._fields_]
    for k, v in over.items():
        assert k in fields
        setattr(a, k, v)
    return a


def _replay_args(**over):
    a = backend_lib.Lz77SlidingWideReplayArgs(256, 0, 8, 256, 256, 256, 1, 256, 4, 256, 256, 256, 1 << 20, 100, 0)
    fields = [f for f, _ in backend_lib.Lz77SlidingWideReplayArgs._fields_]
    for k, v in over.items():
        assert k in fields
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("bad, word", [(dict(hash_length=0), "hash_length"), (dict(hash_length=9), "hash_length"),
                                       (dict(hash_table_size=0), "hash_table_size"),
                                       (dict(hash_table_size=1 << 32), "hash_table_size"),
                                       (dict(max_chain_length=0), "max_chain_length"),
                                       (dict(max_chain_length=65), "max_chain_length"),
                                       (dict(min_match_length=0), "min_match_length"), (dict(n=1 << 32), "2^32"),
                                       (dict(start=9), "start"), (dict(phases=16), "phases")])
def test_parse_wide_refuses_parameters_before_any_device_call(bad, word):
    L = backend_lib.load()
    assert L.scl_lz77_sliding_parse_wide(ctypes.byref(_parse_args(**bad)), None) == backend_lib.E_PARAM
    assert backend_lib.last_error().startswith("lz77_sliding_parse_wide:") and word in backend_lib.last_error()


def test_null_pointers_and_bad_scratch_are_e_param_before_any_device_call():
    L = backend_lib.load()
    assert L.scl_lz77_sliding_parse_wide(None, None) == backend_lib.E_PARAM
    for name in ("d_win", "d_lit_count", "d_match_len", "d_match_off", "d_literals", "d_n_seq", "d_n_lit", "d_status", "d_scratch"):
        assert L.scl_lz77_sliding_parse_wide(ctypes.byref(_parse_args(**{name: None})), None) == backend_lib.E_PARAM, name
        assert "null pointer" in backend_lib.last_error()
    need = dev.sliding_wide_scratch_bytes(8)
    assert L.scl_lz77_sliding_parse_wide(ctypes.byref(_parse_args(scratch_bytes=need - 1)), None) == backend_lib.E_PARAM
    assert L.scl_lz77_sliding_parse_wide(ctypes.byref(_parse_args(d_scratch=257)), None) == backend_lib.E_PARAM
    assert "scl_lz77_sliding_wide_scratch_bytes" in backend_lib.last_error()
    assert L.scl_lz77_sliding_replay_wide(None, None) == backend_lib.E_PARAM
    for name in ("d_win", "d_lit_count", "d_match_len", "d_match_off", "d_literals", "d_out_len", "d_status", "d_scratch"):
        assert L.scl_lz77_sliding_replay_wide(ctypes.byref(_replay_args(**{name: None})), None) == backend_lib.E_PARAM, name
        assert backend_lib.last_error().startswith("lz77_sliding_replay_wide:")
    for bad in (dict(cap=1 << 32), dict(have=9), dict(n_seq=1 << 32), dict(n_lit=1 << 32), dict(d_scratch=257),
                dict(scratch_bytes=dev.wide_replay_scratch_bytes(1, 8) - 1)):
        assert L.scl_lz77_sliding_replay_wide(ctypes.byref(_replay_args(**bad)), None) == backend_lib.E_PARAM, bad
