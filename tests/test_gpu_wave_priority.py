"""The wave-priority code of the two headline kernels (csrc/scl_ans_frame.h, scl_wave_prio_*): control flow keyed on a line
counter and on a hardware register (the wave's slot on its SIMD), in the line loops of rans_encode_fast_kernel (striped
writer) and of the 1024-lane rans_decode_fast_kernel.  Priority may only steer the scheduler, so every result must be bit
for bit what it was: every encode case is held against the C oracle's streams, every decode case against the input.

Shapes: chunk lengths with no line, one line, a ragged head plus one line, four lines (every rotation value occurs) and the
workload's 32; chunk counts with partial waves, partial workgroups and more workgroups than one CU holds, on linear and on
striped slots; a ragged batch whose neighbouring lanes differ by whole lines (the waves of a SIMD then run different line
counts); the smallest batch that takes the 1024-lane decoder and puts four waves on every SIMD; tANS at RANGE_FACTOR 1 and
rANS at NUM_BITS_OUT 8, which run on the same kernels."""
import numpy as np
import pytest

import scl_oracle as orc
from stanford_compression_library_amd import bench_data
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import models

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FREQ = bench_data.t256_table()
CAP = 4096
LAYOUTS = ["linear", "striped"]
# the smallest batch that takes the 1024-lane decoder (ans_wide_workgroups: more than 131 072 chunks)
BIG_CHUNKS, BIG_LEN = 131136, 512

# name -> (model factory, oracle encode)
CODERS = {
    "rans": (lambda: models.RansModel(FREQ.tolist(), 1 << 16, 1, 32), lambda s: orc.rans_encode(s, FREQ, RF=1 << 16, b=1)),
    "tans_rf1": (lambda: models.TansModel(FREQ.tolist(), 1, 32), lambda s: orc.tans_encode(s, FREQ, RF=1)),
    "rans_b8": (lambda: models.RansModel(FREQ.tolist(), 1 << 8, 8, 32), lambda s: orc.rans_encode(s, FREQ, RF=1 << 8, b=8)),
}


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pool(dev):
    """1025 rows of 4096 i.i.d. symbols from the headline's table; every small case reads a corner of it (never written)"""
    d = bench_data.iid_chunks_device(FREQ, 1025, CAP, seed=11, device=dev)
    return d, d.cpu().numpy()


def _bits(data_np, bit_off, nbits):
    first = int(bit_off) // 8
    b = np.unpackbits(data_np[first:(int(bit_off) + int(nbits) + 7) // 8 + 1])
    lo = int(bit_off) - 8 * first
    return b[lo:lo + int(nbits)]


def _check(model, o_enc, d_sym, h_sym, h_lens, layout, oracle_chunks):
    """encode on `layout`, the streams of `oracle_chunks` against the oracle, decode, everything against the input.
    h_lens: None (every row whole) or the int32 lengths."""
    n, cap = d_sym.shape
    d_lens = None if h_lens is None else torch.from_numpy(h_lens).to(d_sym.device)
    enc = model.encode_batch(d_sym, lens=d_lens, layout=layout)
    assert enc.layout == layout and int(enc.status.abs().sum()) == 0
    want = np.full(n, cap, dtype=np.int32) if h_lens is None else h_lens
    data = (enc.linear_data() if layout == "striped" else enc.data).cpu().numpy()
    offs, nbits = enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in oracle_chunks:
        rb, rn = o_enc(h_sym[c, :want[c]])
        assert int(nbits[c]) == rn, f"chunk {c}: {int(nbits[c])} bits, the oracle has {rn}"
        assert np.array_equal(_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}: stream differs from the oracle"
    dec, dlens, used, status = model.decode_encoded(enc, cap)
    assert int(status.abs().sum()) == 0
    d_want = torch.from_numpy(want).to(d_sym.device)
    assert torch.equal(dlens, d_want) and torch.equal(used, enc.nbits)
    inside = torch.arange(cap, device=d_sym.device)[None, :] < d_want[:, None]
    assert not bool(((dec != d_sym) & inside).any())


def _sample(n, k, seed):
    some = set(np.random.default_rng(seed).choice(n, min(n, k), replace=False).tolist()) | {0, n - 1, min(n - 1, 63), min(n - 1, 64)}
    return sorted(some)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("chunk_len", [0, 1, 127, 128, 129, 512, 4096])
def test_chunk_lengths(chunk_len, layout, pool, dev):
    """200 equally long chunks (three waves and a partial one): no line, one line, a ragged head plus one line, four lines,
    the workload's 32"""
    make, o_enc = CODERS["rans"]
    d, h = pool
    n = 200
    if chunk_len == 0:  # (a tensor without columns carries no rows: the lengths say 0)
        _check(make(), o_enc, d[:n, :128], h[:n, :128], np.zeros(n, dtype=np.int32), layout, range(n))
    else:
        _check(make(), o_enc, d[:n, :chunk_len], h[:n, :chunk_len], None, layout, range(n) if chunk_len <= 512 else _sample(n, 40, 1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_chunks", [1, 63, 65, 255, 257, 1025])
def test_chunk_counts(n_chunks, layout, pool, dev):
    """partial waves, partial workgroups, more workgroups than one CU holds; four lines per chunk"""
    make, o_enc = CODERS["rans"]
    d, h = pool
    _check(make(), o_enc, d[:n_chunks, :512], h[:n_chunks, :512], None, layout, _sample(n_chunks, 48, n_chunks))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_neighbouring_lanes_differ_by_whole_lines(layout, pool, dev):
    """257 chunks of 0..32 whole lines, neighbours 7 lines apart (mod 33), every fifth with a ragged head on top: the lanes
    of a wave leave the line loop at different counts, and the waves of a SIMD run different numbers of lines"""
    make, o_enc = CODERS["rans"]
    d, h = pool
    c = np.arange(257)
    lens = 128 * ((7 * c) % 33) + np.where(c % 5 == 0, (c * 13) % 128, 0)
    lens = np.minimum(lens, CAP).astype(np.int32)
    assert {int(x) >> 7 for x in lens} == set(range(33)) and np.all(np.abs(np.diff(lens >> 7)) >= 7)
    _check(make(), o_enc, d[:257], h[:257], lens, layout, range(257))


def test_four_waves_on_every_simd(dev):
    """131 136 chunks x 512 symbols on striped slots: the 1024-lane decoder and the striped encoder with four waves on every
    SIMD, the only configuration in which arbitration matters; the whole round trip and 64 sampled streams against the oracle"""
    make, o_enc = CODERS["rans"]
    model = make()
    enc_k, dec_k = model.kernel_names(BIG_CHUNKS, "striped")
    assert enc_k == "rans_encode_fast_kernel<AnsBackWriterT<256>, 0, 10, 16, 1>", enc_k
    assert dec_k == "rans_decode_fast_kernel<12, 3, 1024, 1, true>", dec_k
    d_sym = bench_data.iid_chunks_device(FREQ, BIG_CHUNKS, BIG_LEN, seed=12, device=dev)
    sample = sorted(set(np.random.default_rng(5).choice(BIG_CHUNKS, 58, replace=False).tolist())
                    | {0, 63, 64, 1023, 1024, 131071, 131072, BIG_CHUNKS - 1})[:64]
    rows = d_sym[torch.as_tensor(sample, device=dev)].cpu().numpy()

    class SampledRows:  # only the sampled rows come to the host
        def __getitem__(self, key):
            c, cols = key
            return rows[sample.index(c), cols]

    _check(model, o_enc, d_sym, SampledRows(), None, "striped", sample)


@pytest.mark.parametrize("name", ["tans_rf1", "rans_b8"])
def test_other_coders_on_the_same_kernels(name, pool, dev):
    """tANS at RANGE_FACTOR 1 and rANS at NUM_BITS_OUT 8, 257 chunks x 512 on striped slots"""
    make, o_enc = CODERS[name]
    model = make()
    assert model.striped_ok(), name
    enc_k, dec_k = model.kernel_names(257, "striped")
    assert enc_k.startswith("rans_encode_fast_kernel<AnsBackWriterT<256>") and dec_k.startswith("rans_decode_fast_kernel<")
    d, h = pool
    _check(model, o_enc, d[:257, :512], h[:257, :512], None, "striped", range(257))
