"""CPU: the yardstick of tests/test_gpu_aec_rare_paths.py (aec_rare_helpers.py), pinned before any kernel is compared
with it, and the conditions on its inputs that make the GPU test reach the branches it is named after.

The literal-loop encoder of the helper must give the CPU oracle's streams bit for bit (the oracle is pinned to the
reference's goldens by test_oracle_goldens.py).  Every case's prefix must reach k + pending > 32 -- the value each was
found with is asserted, so a change of the inputs shows here and not as a GPU test that quietly stopped taking the
fallback -- and the batch the GPU test runs must reach it in every chunk and hold strict-comparison corners with a
nonzero low."""
import numpy as np
import pytest

import scl_oracle as orc
from aec_rare_helpers import CASES, CORNER_CHUNKS, N_CHUNKS, batch, encode, oracle_args


def _literal(case, symbols):
    return encode(symbols, case.kind, case.K, case.k, case.f_init)


def _oracle_bits(case, symbols):
    rb, rn = orc.aec_encode(np.asarray(symbols), **oracle_args(case))
    return np.unpackbits(rb)[:rn]


def test_model_kinds_match_the_oracles():
    assert (orc.MODEL_FIXED, orc.MODEL_IID, orc.MODEL_ORDERK) == (0, 1, 2)


@pytest.mark.parametrize("name", list(CASES))
def test_prefix_reaches_the_long_field_fallback(name):
    case = CASES[name]
    got = _literal(case, case.prefix)
    assert np.array_equal(got.bits, _oracle_bits(case, case.prefix))
    assert got.max_k_pending == case.max_k_pending and got.max_k_pending > 32
    # the closed form agrees with the loops on that symbol: `k + pending > 32` alone sends it through them
    assert got.long_fields == 1


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_batch_matches_the_oracle_and_reaches_both_branches(name):
    case = CASES[name]
    sym, lens = batch(name)
    p = len(case.prefix)
    assert sym.shape[0] == N_CHUNKS and int(lens.min()) == p and (sym[:, :p] == case.prefix).all()
    corners = 0
    for c in range(N_CHUNKS):
        got = _literal(case, sym[c, :lens[c]])
        assert np.array_equal(got.bits, _oracle_bits(case, sym[c, :lens[c]])), f"chunk {c}"
        assert got.max_k_pending > 32 and got.long_fields >= 1, f"chunk {c}"
        assert got.corners > 0 or c not in CORNER_CHUNKS, f"chunk {c}"
        corners += got.corners
    assert corners > 0
