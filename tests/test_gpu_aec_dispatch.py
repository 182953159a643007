"""GPU test of the arithmetic coder's kernel dispatch (csrc/scl_aec.hip: the table of tuned kernel families): one model
per family -- static, iid, fast/split (i.i.d. and order-1 on 16 symbols), sparse and, under SCL_AEC_WIDE=dense, wide --
on rows the tuned kernels take as they are, on rows at an odd address with an odd stride (re-laid through the row relay)
and on an input the tuned readers must decline.  Every layout gives the same streams and the same symbols, the first
eight chunks are checked against the CPU oracle, and nothing is written outside the decoded symbols.

130 chunks (two full waves and a partial one) of up to 208 symbols; the lengths 0, 1, 207 and 208 are among the first
eight chunks, so the oracle sees them all."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scl_oracle as orc
from stanford_compression_library_amd import bench_data
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_CHUNKS, CHUNK_LEN, ODD_STRIDE, FILL, N_ORACLE = 130, 208, 211, 0xA5, 8
F16 = np.arange(1, 17, dtype=np.int64)  # a skewed 16-symbol table, for the symbols of the K = 16 models


def _t256():
    return bench_data.t256_table()


# name -> (model, table the symbols are drawn from, the oracle's arguments)
CASES = {
    "static_fixed_t256": (lambda: models.AecModel(backend_lib.MODEL_FIXED, _t256().tolist(), 256, 0, 1 << 30, 32, 32), _t256,
                          lambda: dict(model_kind=orc.MODEL_FIXED, K=256, f_init=_t256())),
    "iid256": (lambda: models.AecModel(backend_lib.MODEL_IID, [1] * 256, 256, 0, 1 << 30, 32, 32), _t256,
               lambda: dict(model_kind=orc.MODEL_IID, K=256, f_init=np.ones(256))),
    "fast_iid16": (lambda: models.AecModel(backend_lib.MODEL_IID, [1] * 16, 16, 0, 1 << 30, 32, 32), lambda: F16,
                   lambda: dict(model_kind=orc.MODEL_IID, K=16, f_init=np.ones(16))),
    "fast_orderk16": (lambda: models.AecModel(backend_lib.MODEL_ORDERK, None, 16, 1, 1 << 30, 32, 32), lambda: F16,
                      lambda: dict(model_kind=orc.MODEL_ORDERK, K=16, k=1)),
    # sparse by default, wide in the child process of test_orderk256_with_dense_rows_forced
    "orderk256": (lambda: models.AecModel(backend_lib.MODEL_ORDERK, None, 256, 1, 1 << 30, 32, 32), _t256,
                  lambda: dict(model_kind=orc.MODEL_ORDERK, K=256, k=1)),
}


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def _lens():
    lens = np.random.default_rng(31).integers(0, CHUNK_LEN + 1, N_CHUNKS).astype(np.int32)
    lens[:N_ORACLE] = [0, 1, 207, 208, 100, 64, 17, 150]
    return lens


def _stream_bits(data_np, bit_off, nbits):
    first = int(bit_off) // 8
    bits = np.unpackbits(data_np[first:(int(bit_off) + int(nbits) + 7) // 8 + 1])
    lo = int(bit_off) - 8 * first
    return bits[lo:lo + int(nbits)]


def _odd_rows(dev):
    """(buffer pre-filled with FILL, its N_CHUNKS x ODD_STRIDE rows starting at byte 1)"""
    buf = torch.full((1 + N_CHUNKS * ODD_STRIDE + 64,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[1:1 + N_CHUNKS * ODD_STRIDE].view(N_CHUNKS, ODD_STRIDE)


def _encoded(model, d_sym, d_lens, **kw):
    enc = model.encode_batch(d_sym, lens=d_lens, **kw)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    return enc, nbits, [_stream_bits(data, offs[c], nbits[c]) for c in range(N_CHUNKS)]


@pytest.mark.parametrize("name", list(CASES))
def test_aec_family_on_aligned_odd_and_declined_rows(name, dev):
    make_model, table, oracle_args = CASES[name]
    model = make_model()
    assert model.fast_path(CHUNK_LEN), "the model must be served by a tuned family, or the test compares nothing"
    lens = _lens()
    sym = bench_data.iid_chunks_host(table(), N_CHUNKS, CHUNK_LEN, seed=41)
    d_lens = torch.from_numpy(lens).to(dev)

    # encode: (A) aligned rows, (B) the same symbols at base + 1 with stride 211, (R) the any-parameter kernels on A
    sym_a = torch.from_numpy(sym).to(dev)
    assert sym_a.data_ptr() % 16 == 0 and sym_a.stride(0) % 16 == 0
    _, rows_b = _odd_rows(dev)
    rows_b[:, :CHUNK_LEN] = sym_a
    sym_b = rows_b[:, :CHUNK_LEN]
    assert sym_b.data_ptr() % 2 == 1 and sym_b.stride(0) == ODD_STRIDE
    enc_a, nbits_a, bits_a = _encoded(model, sym_a, d_lens)
    _, nbits_b, bits_b = _encoded(model, sym_b, d_lens)
    _, nbits_r, bits_r = _encoded(model, sym_a, d_lens, any_parameter_kernels=True)
    assert np.array_equal(nbits_a, nbits_b) and np.array_equal(nbits_a, nbits_r)
    for c in range(N_CHUNKS):
        assert np.array_equal(bits_a[c], bits_b[c]), f"chunk {c}: odd rows give another stream"
        assert np.array_equal(bits_a[c], bits_r[c]), f"chunk {c}: the any-parameter kernels give another stream"

    # the oracle on the first eight chunks (lengths 0, 1, 207, 208 among them)
    okw = oracle_args()
    kind, K = okw.pop("model_kind"), okw.pop("K")
    ref_used = {}
    for c in range(N_ORACLE):
        rb, rn = orc.aec_encode(sym[c, :lens[c]], kind, K, **okw)
        assert int(nbits_a[c]) == rn, f"chunk {c}: {nbits_a[c]} bits vs oracle {rn}"
        assert np.array_equal(bits_a[c], np.unpackbits(rb)[:rn]), f"chunk {c}: stream differs from the oracle's"
        if lens[c] > 0:  # (the reference never terminates on an empty arithmetic-coded block)
            o_sym, ref_used[c] = orc.aec_decode(rb, rn, kind, K, **okw)
            assert np.array_equal(np.asarray(o_sym), sym[c, :lens[c]])

    def check(dec, dlens, used, status, what):
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0, what
        assert np.array_equal(dlens.cpu().numpy(), lens), what
        used = used.cpu().numpy()
        assert np.array_equal(used, nbits_a), what
        for c, u in ref_used.items():
            assert used[c] == u, f"{what}: chunk {c} consumed {used[c]} bits, the oracle {u}"
        got = dec.cpu().numpy()
        for c in range(N_CHUNKS):
            assert np.array_equal(got[c, :lens[c]], sym[c, :lens[c]]), f"{what}: chunk {c}"

    # decode the A streams into (a) aligned rows
    check(*model.decode_batch(enc_a.data, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN), "aligned rows")
    # (b) rows at an odd base and an odd stride inside a buffer of sentinels
    buf, rows = _odd_rows(dev)
    outs = tuple(torch.zeros(N_CHUNKS, dtype=torch.int32, device=dev) for _ in range(3))
    check(*model.decode_batch(enc_a.data, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN, out=(rows,) + outs), "odd rows")
    got = rows.cpu().numpy()
    for c in range(N_CHUNKS):
        assert (got[c, lens[c]:] == FILL).all(), f"chunk {c}: bytes behind the decoded symbols were written"
    assert (buf[:1].cpu().numpy() == FILL).all() and (buf[1 + N_CHUNKS * ODD_STRIDE:].cpu().numpy() == FILL).all()
    # (c) aligned rows from an input that is 4-byte but not 16-byte aligned: the tuned readers that load lines decline it.
    # (The streams are copied to base + 4 and keep their bit offsets: chunk 0 starts at bit 0 of the encoder's buffer, so
    # reading that buffer from byte 4 on with every offset lowered by 32 would ask for bit -32.)
    moved = torch.zeros(enc_a.data.numel() + 16, dtype=torch.uint8, device=dev)[4:4 + enc_a.data.numel()]
    moved.copy_(enc_a.data)
    assert moved.data_ptr() % 16 == 4
    check(*model.decode_batch(moved, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN), "input at base + 4")
    # (d) both at once: the families whose readers load words take the moved input once the odd rows are re-laid, the others
    # leave the call to the any-parameter kernels
    buf, rows = _odd_rows(dev)
    outs = tuple(torch.zeros(N_CHUNKS, dtype=torch.int32, device=dev) for _ in range(3))
    check(*model.decode_batch(moved, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN, out=(rows,) + outs), "input at base + 4, odd rows")
    got = rows.cpu().numpy()
    for c in range(N_CHUNKS):
        assert (got[c, lens[c]:] == FILL).all(), f"chunk {c}: bytes behind the decoded symbols were written"
    assert (buf[:1].cpu().numpy() == FILL).all() and (buf[1 + N_CHUNKS * ODD_STRIDE:].cpu().numpy() == FILL).all()


def test_orderk256_with_dense_rows_forced():
    """order-1 on 256 symbols runs scl_aec_sparse.hip by default; once more under SCL_AEC_WIDE=dense, i.e. on the
    two-level-row kernels of scl_aec_wide.hip"""
    env = dict(os.environ, SCL_AEC_WIDE="dense")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "orderk256 and not forced", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout
