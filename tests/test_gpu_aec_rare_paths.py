"""GPU test of the tuned arithmetic-coder kernels' rare renormalisation paths: the literal loops of the reference that a
symbol takes when its closed-form field does not fit (`k + pending > 32`) or when it sits on a strict-comparison corner
(quirk Q1), the decoders' mirror of them, the decoders' exit on the last symbol, and the chunk's two ends (header,
termination, consumed-bit count).  One model per family -- static, fast/split (i.i.d. and order-1; the encoder as shipped
and under SCL_AEC_ENC=lane), iid, sparse and, under SCL_AEC_WIDE=dense in a child process, wide.

Inputs: aec_rare_helpers.batch -- 130 chunks (two full waves and a partial one) of at most 64 symbols, each starting with
the case's prefix.  tests/test_aec_rare_reference.py shows on the CPU that every chunk reaches k + pending > 32 and that
the batch holds strict corners with a nonzero low.  Expectations: the CPU oracle on every chunk, and the any-parameter
kernels (csrc/scl_aec.hip), which hold none of the code under test.

Which family runs a case: the C ABI reports no kernel names, so the test checks model.fast_path -- some tuned family serves
the model -- and takes the family from the row conditions of the dispatch table in csrc/scl_aec.hip (aec_families): FIXED
-> static; IID / order-1 on a small alphabet (aec_fast_ok) -> fast (decoder) and split or, under SCL_AEC_ENC=lane, fast
(encoder); IID on a larger one -> iid; order-1 on a larger one -> sparse or, under SCL_AEC_WIDE=dense, wide.  A change of
those conditions that sent a case to another tuned family would not show here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import scl_oracle as orc
from aec_rare_helpers import CASES, CHUNK_LEN, N_CHUNKS, batch, oracle_args
from stanford_compression_library_amd.backend import models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    from stanford_compression_library_amd.backend import lib as backend_lib

    backend_lib.require_device()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(symbols, lens, [stream bits per chunk], [bits the oracle's decoder consumed per chunk])"""
    case = CASES[name]
    sym, lens = batch(name)
    kw = oracle_args(case)
    kind, K = kw.pop("model_kind"), kw.pop("K")
    bits, used = [], []
    for c in range(N_CHUNKS):
        rb, rn = orc.aec_encode(sym[c, :lens[c]], kind, K, **kw)
        o_sym, u = orc.aec_decode(rb, rn, kind, K, **kw)
        assert np.array_equal(np.asarray(o_sym), sym[c, :lens[c]])
        bits.append(np.unpackbits(rb)[:rn])
        used.append(u)
    return sym, lens, bits, np.array(used)


def _stream_bits(data_np, bit_off, nbits):
    first = int(bit_off) // 8
    bits = np.unpackbits(data_np[first:(int(bit_off) + int(nbits) + 7) // 8 + 1])
    lo = int(bit_off) - 8 * first
    return bits[lo:lo + int(nbits)]


def _model(case):
    f = list(case.f_init) if case.f_init is not None else (None if case.kind == orc.MODEL_ORDERK else [1] * case.K)
    return models.AecModel(case.kind, f, case.K, case.k, 1 << 30, 32, 32)


def _check_case(name, dev):
    case = CASES[name]
    sym, lens, ref_bits, ref_used = _expected(name)
    model = _model(case)
    # The ABI reports no kernel names: that a tuned family serves the model is checked, WHICH family is inferred from the
    # dispatch table of csrc/scl_aec.hip (aec_families), not checked.
    assert model.fast_path(CHUNK_LEN), "the model must be served by a tuned family, or the test compares nothing"
    d_sym, d_lens = torch.from_numpy(sym).to(dev), torch.from_numpy(lens).to(dev)

    def encoded(**kw):
        enc = model.encode_batch(d_sym, lens=d_lens, **kw)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0
        data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
        return enc, [_stream_bits(data, offs[c], nbits[c]) for c in range(N_CHUNKS)]

    enc, bits = encoded()
    _, bits_any = encoded(any_parameter_kernels=True)
    for c in range(N_CHUNKS):
        assert np.array_equal(bits[c], ref_bits[c]), f"chunk {c} (length {lens[c]}): stream differs from the oracle's"
        assert np.array_equal(bits_any[c], ref_bits[c]), f"chunk {c}: the any-parameter kernels differ from the oracle"

    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, CHUNK_LEN)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert np.array_equal(dlens.cpu().numpy(), lens)
    assert np.array_equal(used.cpu().numpy(), ref_used), "consumed-bit counts differ from the oracle's"
    got = dec.cpu().numpy()
    for c in range(N_CHUNKS):
        assert np.array_equal(got[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c} (length {lens[c]})"


# "order1_k39": scl_aec_sparse.hip runs it here, scl_aec_wide.hip in the child process below
@pytest.mark.parametrize("name", list(CASES))
def test_rare_paths(name, dev):
    _check_case(name, dev)


@pytest.mark.parametrize("name", ["fast_iid", "fast_order1"])
def test_rare_paths_one_lane_encoder(name, dev, monkeypatch):
    """the fast models' encoder is scl_aec_split.hip as shipped (above); SCL_AEC_ENC=lane selects scl_aec_fast.hip's"""
    monkeypatch.setenv("SCL_AEC_ENC", "lane")
    _check_case(name, dev)


def test_rare_paths_with_dense_rows_forced():
    """SCL_AEC_WIDE=dense puts scl_aec_wide.hip in charge of the order-k models on large alphabets"""
    env = dict(os.environ, SCL_AEC_WIDE="dense")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "test_rare_paths and order1_k39 and not forced", "-p", "no:cacheprovider"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout
