"""GPU parity, part 2: the batched C-ABI entry points (device buffers, one lane per chunk) against the CPU
oracle on seeded inputs -- ragged and empty chunks, trailing-garbage tolerance, stream compaction (dense and
EncodedBlockWriter framing) -- and size-independent round-trip properties at BASELINE.json configs[1] size."""
import os

import numpy as np
import pytest

import scl_oracle as orc
from stanford_compression_library_amd import bench_data
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def _stream_bits(data_np, bit_off, nbits):
    first = int(bit_off) // 8
    bits = np.unpackbits(data_np[first:(int(bit_off) + int(nbits) + 7) // 8 + 1])
    lo = int(bit_off) - 8 * first
    return bits[lo:lo + int(nbits)]


CODERS = {
    "rans_default": (lambda f: models.RansModel(f.tolist(), 1 << 16, 1, 32),
                     lambda s, f: orc.rans_encode(s, f), lambda p, n, f: orc.rans_decode(p, n, f)),
    "rans_b8": (lambda f: models.RansModel(f.tolist(), 1 << 8, 8, 32),
                lambda s, f: orc.rans_encode(s, f, RF=1 << 8, b=8), lambda p, n, f: orc.rans_decode(p, n, f, RF=1 << 8, b=8)),
    "rans_u64": (lambda f: models.RansModel(f.tolist(), 1 << 24, 16, 20),
                 lambda s, f: orc.rans_encode(s, f, RF=1 << 24, b=16, size_bits=20),
                 lambda p, n, f: orc.rans_decode(p, n, f, RF=1 << 24, b=16, size_bits=20)),
    "tans_rf1": (lambda f: models.TansModel(f.tolist(), 1, 32),
                 lambda s, f: orc.tans_encode(s, f, RF=1), lambda p, n, f: orc.tans_decode(p, n, f, RF=1)),
    "tans_rf16": (lambda f: models.TansModel(f.tolist(), 16, 32),
                  lambda s, f: orc.tans_encode(s, f, RF=16), lambda p, n, f: orc.tans_decode(p, n, f, RF=16)),
    "range32": (lambda f: models.RangeModel(f.tolist(), 32, 32),
                lambda s, f: orc.range_encode(s, f), lambda p, n, f: orc.range_decode(p, n, f)),
    "range48": (lambda f: models.RangeModel(f.tolist(), 48, 17),
                lambda s, f: orc.range_encode(s, f, precision=48, size_bits=17),
                lambda p, n, f: orc.range_decode(p, n, f, precision=48, size_bits=17)),
    "aec_fixed": (lambda f: models.AecModel(0, f.tolist(), f.size, 0, 1 << 30, 32, 32),
                  lambda s, f: orc.aec_encode(s, orc.MODEL_FIXED, f.size, f_init=f),
                  lambda p, n, f: orc.aec_decode(p, n, orc.MODEL_FIXED, f.size, f_init=f)),
    "aec_iid": (lambda f: models.AecModel(1, [1] * f.size, f.size, 0, 1 << 30, 32, 32),
                lambda s, f: orc.aec_encode(s, orc.MODEL_IID, f.size, f_init=np.ones(f.size)),
                lambda p, n, f: orc.aec_decode(p, n, orc.MODEL_IID, f.size, f_init=np.ones(f.size))),
}


@pytest.mark.parametrize("name", list(CODERS))
def test_batch_ragged_vs_oracle(name, dev):
    """20 chunks of different lengths (incl. 0 and 1) in one launch; every stream equals the oracle's, every
    decode (with 0 or 37 garbage bits after the stream) returns the symbols and the exact bit count."""
    make_model, o_enc, o_dec = CODERS[name]
    freq = bench_data.t256_table()
    model = make_model(freq)
    rng = np.random.default_rng(11)
    lens = np.array([0, 1, 2, 3, 7, 64, 65, 100, 255, 256, 257, 300, 301, 302, 303, 304, 305, 511, 512, 333], dtype=np.int32)
    cap = 512
    sym = bench_data.iid_chunks_host(freq, len(lens), cap, seed=12)
    d_sym = torch.from_numpy(sym).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)
    enc = model.encode_batch(d_sym, lens=d_lens)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    data = enc.data.cpu().numpy()
    offs, nbits = enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    ref = [o_enc(sym[c, :lens[c]], freq) for c in range(len(lens))]
    for c, (rb, rn) in enumerate(ref):
        assert int(nbits[c]) == rn, f"chunk {c}: {nbits[c]} bits vs oracle {rn}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
    # decode straight from the encoder's slots
    skip_empty_aec = name.startswith("aec")
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert np.array_equal(dlens.cpu().numpy(), lens)
    assert np.array_equal(used.cpu().numpy(), nbits)
    dec = dec.cpu().numpy()
    for c in range(len(lens)):
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]])
    # decode from a dense buffer where 37 garbage bits follow every stream (streams are bit-adjacent)
    pieces, new_off, new_avail, pos = [], [], [], 0
    for c, (rb, rn) in enumerate(ref):
        g = rng.integers(0, 2, 37).astype(np.uint8)
        pieces += [np.unpackbits(rb)[:rn], g]
        new_off.append(pos)
        new_avail.append(rn + 37)
        pos += rn + 37
    packed = np.packbits(np.concatenate(pieces))
    buf = torch.zeros(packed.size + 32, dtype=torch.uint8, device=dev)
    buf[:packed.size] = torch.from_numpy(packed).to(dev)
    dec2, dlens2, used2, status2 = model.decode_batch(buf, torch.tensor(new_off, dtype=torch.int64, device=dev),
                                                      torch.tensor(new_avail, dtype=torch.int32, device=dev), cap)
    torch.cuda.synchronize()
    assert int(status2.abs().sum()) == 0
    used2 = used2.cpu().numpy()
    for c, (rb, rn) in enumerate(ref):
        if lens[c] == 0 and skip_empty_aec:
            continue  # quirk Q5: the reference never terminates on an empty arithmetic-coded block
        o_sym, o_used = o_dec(np.packbits(np.concatenate([np.unpackbits(rb)[:rn], pieces[2 * c + 1]])), rn + 37, freq)
        assert used2[c] == o_used == rn
        assert np.array_equal(dec2[c, :lens[c]].cpu().numpy(), sym[c, :lens[c]])


@pytest.mark.parametrize("K,k", [(4, 1), (16, 1), (3, 2), (256, 1), (5, 0), (100, 1), (40, 2), (33, 1), (256, 0), (17, 1), (31, 1), (32, 1), (20, 2), (5, 3), (16, 2), (7, 2)])
def test_batch_aec_orderk_vs_oracle(K, k, dev):
    """order-k adaptive arithmetic coding with the any-parameter kernels (global-memory / LDS16 / two-level
    models of scl_aec.hip), private model per lane"""
    n_chunks, n = 12, 700
    sym = np.stack([bench_data.markov1_host(K, n, seed=100 + c) for c in range(n_chunks)])
    model = models.AecModel(2, None, K, k, 1 << 30, 32, 32)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), any_parameter_kernels=True)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, n, any_parameter_kernels=True)
    dec_t, _, used_t, status_t = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, n)  # tuned, where they apply
    torch.cuda.synchronize()
    assert int(status_t.abs().sum()) == 0 and torch.equal(dec_t, dec) and torch.equal(used_t, used)
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in range(n_chunks):
        rb, rn = orc.aec_encode(sym[c], orc.MODEL_ORDERK, K, k=k)
        assert int(nbits[c]) == rn
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn])
    assert np.array_equal(dec.cpu().numpy(), sym) and np.array_equal(used.cpu().numpy(), nbits)


@pytest.mark.parametrize("K,k", [(32, 1), (256, 1), (40, 2), (255, 1), (100, 1), (17, 1), (20, 2), (5, 3), (16, 2)])
def test_batch_aec_large_alphabet_line_to_row_transitions(K, k, dev):
    """scl_aec_sparse.hip keeps a context in one 64-byte line (the symbols seen in it) for its first 30 (encoder) / 28 (decoder) symbols and moves
    it to its dense row with the next: runs of one symbol (the context repeats while its line is still in flight: the
    patch path, also across the move), a few hot contexts that cross the boundary early and many cold ones, symbol
    K - 1, chunks that end exactly on the 28th .. 33rd symbol of a context.  Streams, symbols and consumed bits
    against the oracle."""
    rng = np.random.default_rng(900 + K + k)
    model = models.AecModel(2, None, K, k, 1 << 30, 32, 32)
    assert model.fast_path(4096)
    cap = 4096
    rows = []
    hot = rng.choice(K, 3, replace=False)
    for c in range(24):
        kind = c % 4
        if kind == 0:    # runs: the same symbol 1..70 times in a row
            x = np.concatenate([np.full(int(rng.integers(1, 71)), int(rng.integers(0, K))) for _ in range(200)])
        elif kind == 1:  # three hot symbols (hot contexts) with rare excursions over the whole alphabet
            x = np.where(rng.random(cap) < 0.9, rng.choice(hot, cap), rng.integers(0, K, cap))
        elif kind == 2:  # uniform: every context stays cold for K = 256
            x = rng.integers(0, K, cap)
        else:            # one symbol only, incl. the last of the alphabet
            x = np.full(cap, K - 1 if c % 8 == 3 else 0)
        rows.append(np.resize(x, cap))
    sym = np.stack(rows).astype(np.uint8)
    lens = np.array([28, 29, 30, 31, 32, 33, 61, 62] + [int(v) for v in rng.integers(0, cap + 1, 15)] + [cap], dtype=np.int32)
    sym[:8] = sym[3]  # the single-symbol row: its one context takes exactly lens[i] symbols
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    dec, used = dec.cpu().numpy(), used.cpu().numpy()
    assert np.array_equal(dlens.cpu().numpy(), lens)
    for c in range(lens.size):
        rb, rn = orc.aec_encode(sym[c, :lens[c]], orc.MODEL_ORDERK, K, k=k)
        assert int(nbits[c]) == rn, f"chunk {c}: {nbits[c]} bits vs oracle {rn}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        if lens[c] > 0:
            assert used[c] == orc.aec_decode(rb, rn, orc.MODEL_ORDERK, K, k=k)[1], f"chunk {c}"


def test_large_alphabet_order_k_tests_with_dense_rows_forced():
    """order-k models on 32..256 symbols run scl_aec_sparse.hip by default; the same tests once more with SCL_AEC_WIDE=dense,
    i.e. on the two-level-row kernels of scl_aec_wide.hip"""
    import subprocess, sys
    env = dict(os.environ, SCL_AEC_WIDE="dense")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_batch.py"),
                        os.path.join(here, "test_gpu_goldens.py"), os.path.join(here, "test_gpu_guard_bands.py"), "-q", "-m",
                        "gpu", "-x", "-k", "(orderk or order1 or large_alphabet or aec or config4) and not forced and not "
                        "full_occupancy", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


AEC_FAST_CASES = [("orderk", 16, 1), ("orderk", 4, 1), ("orderk", 2, 1), ("orderk", 3, 2), ("orderk", 2, 3),
                  ("orderk", 5, 0), ("orderk", 16, 0), ("orderk", 7, 1), ("iid", 2, 0), ("iid", 11, 0), ("iid", 16, 0),
                  ("iid", 17, 0), ("iid", 100, 0), ("iid", 255, 0), ("iid", 256, 0)]


@pytest.mark.parametrize("kind,K,k", AEC_FAST_CASES)
def test_batch_aec_lds_table_kernels_vs_oracle(kind, K, k, dev):
    """scl_aec_fast.hip (configs[3]: per-lane context tables in LDS, closed-form renormalisation, binary64
    division) and, for i.i.d. models on more than 16 symbols, scl_aec_iid.hip (two-level cumulative table): 300 ragged chunks (two workgroups), every stream equal to the oracle's; decode from the slots and
    from a bit-adjacent buffer with garbage after every stream.  Power-of-two alphabets start every chunk on the
    reference's strict-comparison corner (low == HALF / QTR exactly), i.e. on the literal-loop fallback."""
    rng = np.random.default_rng(1000 + 17 * K + k)
    cap = 1024
    lens = np.concatenate([[0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1000],
                           rng.integers(0, cap + 1, 284)]).astype(np.int32)
    n_chunks = lens.size
    if kind == "iid":
        f_init = rng.integers(1, 40, K).astype(np.uint32)
        model = models.AecModel(1, f_init.tolist(), K, 0, 1 << 30, 32, 32)
        o_enc = lambda s: orc.aec_encode(s, orc.MODEL_IID, K, f_init=f_init)
        o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_IID, K, f_init=f_init)
    else:
        model = models.AecModel(2, None, K, k, 1 << 30, 32, 32)
        o_enc = lambda s: orc.aec_encode(s, orc.MODEL_ORDERK, K, k=k)
        o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_ORDERK, K, k=k)
    assert model.fast_path(cap), "this case must be served by the LDS-table kernels"
    sym = np.stack([bench_data.markov1_host(K, cap, seed=7000 + c) for c in range(n_chunks)])
    sym[5] = 0          # constant runs: the interval collapses towards low = 0 / high = 2^32
    sym[6] = K - 1
    sym[7, ::2] = 0
    sym[7, 1::2] = K - 1
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    ref = [o_enc(sym[c, :lens[c]]) for c in range(n_chunks)]
    for c, (rb, rn) in enumerate(ref):
        assert int(nbits[c]) == rn, f"chunk {c} (n={lens[c]}): {nbits[c]} bits vs oracle {rn}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert np.array_equal(dlens.cpu().numpy(), lens)
    dec, used = dec.cpu().numpy(), used.cpu().numpy()
    for c in range(n_chunks):
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        if lens[c] > 0:
            # the reference's own count (it can be one short of the stream on 1-symbol blocks whose interval
            # ends on a power of two -- the oracle, pinned to the reference, is the judge)
            assert used[c] == o_dec(ref[c][0], ref[c][1])[1], f"chunk {c}"
    assert np.mean(used[lens > 64] == nbits[lens > 64]) > 0.98  # ... and that is rare
    # bit-adjacent streams (arbitrary bit offsets), 0..70 garbage bits after each
    pieces, new_off, new_avail, pos = [], [], [], 0
    for c, (rb, rn) in enumerate(ref):
        g = rng.integers(0, 2, int(rng.integers(0, 71))).astype(np.uint8)
        pieces += [np.unpackbits(rb)[:rn], g]
        new_off.append(pos)
        new_avail.append(rn + g.size)
        pos += rn + g.size
    packed = np.packbits(np.concatenate(pieces))
    buf = torch.zeros((packed.size + 47) // 16 * 16, dtype=torch.uint8, device=dev)
    buf[:packed.size] = torch.from_numpy(packed).to(dev)
    dec2, dlens2, used2, status2 = model.decode_batch(buf, torch.tensor(new_off, dtype=torch.int64, device=dev),
                                                      torch.tensor(new_avail, dtype=torch.int32, device=dev), cap)
    torch.cuda.synchronize()
    assert int(status2.abs().sum()) == 0
    used2, dec2 = used2.cpu().numpy(), dec2.cpu().numpy()
    for c, (rb, rn) in enumerate(ref):
        if lens[c] == 0:
            continue  # quirk Q5
        assert np.array_equal(dec2[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        stream = np.packbits(np.concatenate([pieces[2 * c], pieces[2 * c + 1]]))
        o_sym, o_used = o_dec(stream, new_avail[c])
        assert used2[c] == o_used, f"chunk {c}: consumed {used2[c]} vs oracle {o_used} (stream {rn} bits)"


def test_batch_aec_lds_table_kernels_short_chunks(dev):
    """16 384 chunks of 48 symbols: pounds on the start-of-chunk corners (totals 2, 3, 4, ... are where low and
    high land exactly on HALF / QTR) -- every stream against the oracle."""
    for K in (2, 4):
        n_chunks, n = 1 << 14, 48
        rng = np.random.default_rng(31 + K)
        sym = rng.integers(0, K, (n_chunks, n), dtype=np.uint8)
        sym[:4096] = (rng.random((4096, n)) < 0.9).astype(np.uint8) * (K - 1)  # skewed: long E1/E2 runs
        model = models.AecModel(2, None, K, 1, 1 << 30, 32, 32)
        assert model.fast_path(n)
        enc = model.encode_batch(torch.from_numpy(sym).to(dev))
        dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, n)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
        assert np.array_equal(dec.cpu().numpy()[:, :n], sym) and np.array_equal(used.cpu().numpy(), enc.nbits.cpu().numpy())
        nbits = enc.nbits.cpu().numpy()
        data = enc.data.cpu().numpy()[:n_chunks * enc.stride].reshape(n_chunks, enc.stride)
        for c in range(n_chunks):
            rb, rn = orc.aec_encode(sym[c], orc.MODEL_ORDERK, K, k=1)
            assert int(nbits[c]) == rn, f"K={K} chunk {c}"
            nb = (rn + 7) // 8
            got = data[c, :nb].copy()
            if rn % 8:
                got[-1] &= (0xFF00 >> (rn % 8)) & 0xFF
            assert np.array_equal(got, rb), f"K={K} chunk {c}"


# model name -> (kind, K, k); "<name>+lane": the same model with SCL_AEC_ENC=lane, so that aec_fast_encode_kernel runs
LANE_FRAME_MODELS = {"order1_k16": ("orderk", 16, 1), "order2_k4": ("orderk", 4, 2), "iid_k11": ("iid", 11, 0),
                     "iid_k100": ("iid", 100, 0), "order1_k256": ("orderk", 256, 1)}
LANE_FRAME_CASES = list(LANE_FRAME_MODELS) + [m + "+lane" for m in ("order1_k16", "order2_k4", "iid_k11")]
LANE_FRAME_EDGES = [0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 63, 64, 65, 255, 256, 257, 1023, 1024]
_lane_frame_reference = {}


def _lane_frame_case(name):
    """lengths, symbols and the oracle's streams and decodes of one model: computed once, shared by its cases, never changed"""
    if name not in _lane_frame_reference:
        kind, K, k = LANE_FRAME_MODELS[name]
        o_kw = dict(f_init=np.ones(K)) if kind == "iid" else dict(k=k)
        o_kind = orc.MODEL_IID if kind == "iid" else orc.MODEL_ORDERK
        lens = np.array([1024] * 64 + [LANE_FRAME_EDGES[i % len(LANE_FRAME_EDGES)] for i in range(64)] + [1024] * 64
                        + [1024] * 19, dtype=np.int32)
        sym = np.random.default_rng(9000 + 31 * K + k).integers(0, K, (lens.size, 1040)).astype(np.uint8)
        streams = [orc.aec_encode(sym[c, :lens[c]], o_kind, K, **o_kw) for c in range(lens.size)]
        o_used = np.array([orc.aec_decode(rb, rn, o_kind, K, **o_kw)[1] for rb, rn in streams])  # empty chunks: header + 2
        for a in (lens, sym, o_used):
            a.setflags(write=False)
        _lane_frame_reference[name] = (lens, sym, streams, o_used)
    return _lane_frame_reference[name]


@pytest.mark.parametrize("case", LANE_FRAME_CASES)
def test_aec_lane_frames(case, dev, monkeypatch):
    """What stands around the symbol step of the lane-per-chunk arithmetic-coder kernels (scl_aec_frame.h: header exit,
    unchecked stretches with a wave-wide count, checked loop, peeled last symbol, epilogue; the encoders' word-ahead loop,
    drain and termination; the wide / sparse kernels' symbol feed and output word), on every kernel family that uses it.
    One launch of 64 x 3 + 19 chunks, cap 1040, uniform symbols: a wave of 64 equal chunks of 1024 (stretches with a
    wave-uniform count); a wave whose lengths sit on every loop boundary (lanes drop out one by one, stretches entered off
    a multiple of four); a wave of 64 equal chunks where one lane is given 10 bits (the header exit inside a full wave:
    af_wave_min's partial-wave path, the other 63 lanes still run unchecked); a partial wave of 19."""
    name, _, lane = case.partition("+")
    if lane:
        monkeypatch.setenv("SCL_AEC_ENC", "lane")
    kind, K, k = LANE_FRAME_MODELS[name]
    lens, sym, streams, o_used = _lane_frame_case(name)
    n_chunks, cap, cut = lens.size, 1040, 128 + 37
    # a stretch needs a wave-wide count of at least 16 symbols, i.e. at least 33 words left in every lane's stream
    short = [c for c in range(n_chunks) if lens[c] == 1024 and not 64 <= c < 128 and streams[c][1] < 1280]
    assert not short, f"streams too short for an unchecked stretch: chunks {short}"
    model = (models.AecModel(1, [1] * K, K, 0, 1 << 30, 32, 32) if kind == "iid"
             else models.AecModel(2, None, K, k, 1 << 30, 32, 32))
    assert model.fast_path(cap), "this case must be served by the tuned kernels"
    enc = model.encode_batch(torch.tensor(sym, device=dev), lens=torch.tensor(lens, device=dev))
    torch.cuda.synchronize()
    assert not enc.status.cpu().numpy().any()
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in sorted({0, 63, 127, 128, cut - 1, cut, cut + 1, 191, 192, n_chunks - 1} | set(range(64, 64 + len(LANE_FRAME_EDGES)))):
        rb, rn = streams[c]
        assert int(nbits[c]) == rn, f"chunk {c} (n={lens[c]}): {nbits[c]} bits vs oracle {rn}"
        assert np.array_equal(_stream_bits(data, offs[c], rn), np.unpackbits(rb)[:rn]), f"chunk {c}"
    avail = enc.nbits.clone()
    avail[cut] = 10
    got = []
    for generic in (False, True):
        out = model.alloc_decoded(n_chunks, cap, dev)
        out[0].fill_(0xA5)
        res = model.decode_batch(enc.data, enc.bit_offset, avail, cap, out=out, any_parameter_kernels=generic)
        torch.cuda.synchronize()
        got.append([out[0].cpu().numpy()] + [t.cpu().numpy() for t in res[1:]])
    dec, dlens, used, status = got[0]
    want_lens = lens.copy()
    want_lens[cut] = 0
    assert np.array_equal(dlens, want_lens)
    assert status[cut] == backend_lib.ST_TRUNCATED and not np.delete(status, cut).any()
    assert np.array_equal(np.delete(used, cut), np.delete(o_used, cut)), "consumed bits differ from the oracle's"
    assert used[cut] == 0, "a stream shorter than its header consumes nothing"
    for c in range(n_chunks):
        assert np.array_equal(dec[c, :want_lens[c]], sym[c, :want_lens[c]]), f"chunk {c}"
        assert (dec[c, (want_lens[c] + 3) & ~3:] == 0xA5).all(), f"chunk {c}: bytes beyond the chunk were written"
        assert np.array_equal(got[1][0][c, :want_lens[c]], dec[c, :want_lens[c]]), f"chunk {c}: any-parameter symbols differ"
    for what, a, b in zip(("lengths", "consumed bits", "status"), got[0][1:], got[1][1:]):
        assert np.array_equal(a, b), f"tuned and any-parameter decoders differ in {what}"


@pytest.mark.parametrize("K,T", [(2, 5), (17, 1000), (256, 4096), (100, 4097), (256, 65536), (3, 65536)])
def test_batch_aec_static_model_kernels_vs_oracle(K, T, dev):
    """scl_aec_static.hip (FixedFreqModel: shared table in LDS, line-granular I/O): 300 ragged chunks incl. whole
    128-symbol lines and every tail length, streams equal to the oracle's, decode from the slots and from a
    bit-adjacent buffer with garbage after every stream (exact consumed-bit counts).  Totals <= 4096 use the
    slot -> symbol table, larger ones the binary search."""
    rng = np.random.default_rng(77 * K + T)
    f = np.maximum(1, np.floor(rng.dirichlet(np.full(K, 0.5)) * (T - K)).astype(np.int64) + 1)
    f[np.argmax(f)] += T - f.sum()
    assert f.sum() == T and f.min() >= 1
    f = f.astype(np.uint32)
    cap = 700
    lens = np.concatenate([[0, 1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 383, 384, 640, 700],
                           rng.integers(0, cap + 1, 284)]).astype(np.int32)
    n_chunks = lens.size
    model = models.AecModel(0, f.tolist(), K, 0, 1 << 30, 32, 32)
    assert model.fast_path(cap)
    o_enc = lambda s: orc.aec_encode(s, orc.MODEL_FIXED, K, f_init=f)
    o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_FIXED, K, f_init=f)
    sym = rng.choice(K, (n_chunks, 704), p=f / f.sum()).astype(np.uint8)
    sym[5] = 0
    sym[6] = K - 1
    sym[7] = int(np.argmin(f))  # the rarest symbol over and over: longest renormalisations
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    ref = [o_enc(sym[c, :lens[c]]) for c in range(n_chunks)]
    for c, (rb, rn) in enumerate(ref):
        assert int(nbits[c]) == rn, f"chunk {c} (n={lens[c]}): {nbits[c]} bits vs oracle {rn}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert np.array_equal(dlens.cpu().numpy(), lens)
    dec, used = dec.cpu().numpy(), used.cpu().numpy()
    for c in range(n_chunks):
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        if lens[c] > 0:
            assert used[c] == o_dec(ref[c][0], ref[c][1])[1], f"chunk {c}"
    pieces, new_off, new_avail, pos = [], [], [], 0
    for c, (rb, rn) in enumerate(ref):
        g = rng.integers(0, 2, int(rng.integers(0, 71))).astype(np.uint8)
        pieces += [np.unpackbits(rb)[:rn], g]
        new_off.append(pos)
        new_avail.append(rn + g.size)
        pos += rn + g.size
    packed = np.packbits(np.concatenate(pieces))
    buf = torch.zeros((packed.size + 47) // 16 * 16, dtype=torch.uint8, device=dev)
    buf[:packed.size] = torch.from_numpy(packed).to(dev)
    buf[packed.size:] = 0xA5  # stale memory behind the last stream must not leak into any count
    dec2, dlens2, used2, status2 = model.decode_batch(buf, torch.tensor(new_off, dtype=torch.int64, device=dev),
                                                      torch.tensor(new_avail, dtype=torch.int32, device=dev), cap)
    torch.cuda.synchronize()
    assert int(status2.abs().sum()) == 0
    used2, dec2 = used2.cpu().numpy(), dec2.cpu().numpy()
    for c, (rb, rn) in enumerate(ref):
        if lens[c] == 0:
            continue  # quirk Q5
        assert np.array_equal(dec2[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        stream = np.packbits(np.concatenate([pieces[2 * c], pieces[2 * c + 1]]))
        assert used2[c] == o_dec(stream, new_avail[c])[1], f"chunk {c}"


def _frame_reference(bits):
    """EncodedBlockWriter.write_block on a bit vector (encoded_stream.py:23-46,94-103,150-175), in numpy"""
    n = bits.size
    pad = (8 - (n + 3) % 8) % 8
    payload = np.concatenate([np.unpackbits(np.array([pad], np.uint8))[5:], np.zeros(pad, np.uint8), bits])
    assert payload.size % 8 == 0
    nbytes = payload.size // 8
    return np.concatenate([np.frombuffer(int(nbytes).to_bytes(4, "big"), np.uint8), np.packbits(payload)])


@pytest.mark.parametrize("name", ["rans_default", "range32", "aec_iid"])
@pytest.mark.parametrize("framed", [False, True])
def test_compact_dense_and_framed(name, framed, dev):
    make_model, o_enc, _ = CODERS[name]
    freq = bench_data.t256_table()
    model = make_model(freq)
    lens = np.array([0, 1, 5, 13, 100, 101, 102, 103, 104, 105, 106, 107, 200, 17, 1, 0, 64, 1500, 1499, 777, 1024, 33],
                    dtype=np.int32)  # long streams take the 16-bytes-per-lane bulk path of cp_copy
    sym = bench_data.iid_chunks_host(freq, len(lens), 1500, seed=21)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dense, offsets = models.compact(enc, framed=framed)
    dense, offsets = dense.cpu().numpy(), offsets.cpu().numpy()
    expect = []
    for c in range(len(lens)):
        rb, rn = o_enc(sym[c, :lens[c]], freq)
        bits = np.unpackbits(rb)[:rn]
        expect.append(_frame_reference(bits) if framed else np.packbits(bits))
    sizes = np.array([e.size for e in expect])
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(sizes)]))
    for c, e in enumerate(expect):
        assert np.array_equal(dense[offsets[c]:offsets[c + 1]], e), f"record {c}"


def test_status_reporting(dev):
    freq = bench_data.t256_table()[:16].copy()
    freq[0] += 4096 - freq.sum()
    model = models.RansModel(freq.tolist(), 1 << 16, 1, 32)
    sym = np.full((3, 64), int(np.argmin(freq)), dtype=np.uint8)  # rare symbol: many bits per symbol
    sym[1, 10] = 200  # symbol outside the 16-entry alphabet -> KeyError in the reference
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), out_stride=16)  # far too small a slot
    torch.cuda.synchronize()
    st = enc.status.cpu().numpy()
    assert st[1] & backend_lib.ST_SYMBOL and all(s & backend_lib.ST_CAPACITY for s in st)
    # a corrupted stream must flag the final-state assert (rANS.py:295) or truncation, never crash
    enc = model.encode_batch(torch.from_numpy(sym[:1] * 0 + 3).to(dev))
    torch.cuda.synchronize()
    byte = int(enc.bit_offset[0].item()) // 8 + 9
    enc.data[byte] ^= 0x5A
    _, _, _, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, 64)
    torch.cuda.synchronize()
    assert int(status[0]) & (backend_lib.ST_STATE | backend_lib.ST_TRUNCATED)


@pytest.mark.parametrize("table", ["t256", "uniform"])
def test_config2_roundtrip_properties(table, dev):
    """BASELINE.json configs[1]: 64 Ki chunks x 4 KiB.  Size-independent properties: decode(encode(x)) == x for
    every chunk, consumed == produced bits, and byte-equality with the oracle on a fixed sample of chunks."""
    freq = bench_data.t256_table() if table == "t256" else bench_data.uniform256_table()
    n_chunks, chunk_len = 65536, 4096
    model = models.RansModel(freq.tolist(), 1 << 16, 1, 32)
    sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=2, device=dev)
    enc = model.encode_batch(sym)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, chunk_len)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    assert torch.equal(dec, sym) and torch.equal(used, enc.nbits)
    assert int(dlens.min()) == chunk_len == int(dlens.max())
    sample = [0, 1, 4095, 32768, n_chunks - 1]
    offs, nbits = enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in sample:
        rb, rn = orc.rans_encode(sym[c].cpu().numpy(), freq)
        assert int(nbits[c]) == rn
        lo = int(offs[c]) // 8
        window = enc.data[lo:lo + (rn + 7) // 8 + 2].cpu().numpy()
        bits = np.unpackbits(window)[int(offs[c]) % 8:][:rn]
        assert np.array_equal(bits, np.unpackbits(rb)[:rn])
    # the encoded size is what the model predicts: bits/symbol within 1 % of the cross-entropy + header
    p = freq / freq.sum()
    h = float(-(p * np.log2(p)).sum())
    got = float(enc.nbits.double().mean().item() - 61) / chunk_len
    assert abs(got - h) < 0.05, (got, h)


def test_rans_slot_writer_batch(dev):
    """196 608 chunks = 768 workgroups: the batch shape for which the encoder picks its three-workgroups-per-CU form
    (AnsBackWriterS, 192-byte slot rings; rf_use_slot_writer in scl_rans_fast.hip).  Every chunk round-trips, and the
    streams equal those of the any-parameter kernel word for word (which the goldens pin)."""
    freq = bench_data.t256_table()
    n_chunks, chunk_len = 196608, 4096
    model = models.RansModel(freq.tolist(), 1 << 16, 1, 32)
    sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=77, device=dev)
    enc = model.encode_batch(sym)
    ref = model.encode_batch(sym, any_parameter_kernels=True)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, chunk_len)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    assert torch.equal(dec, sym) and torch.equal(used, enc.nbits) and torch.equal(enc.nbits, ref.nbits)
    assert enc.stride == ref.stride
    # streams end at their slot end: compare the last whole words of every slot
    nwords = int((ref.nbits.max().item() + 31) // 32)
    a = enc.data[:n_chunks * enc.stride].view(n_chunks, enc.stride)[:, enc.stride - 4 * nwords:].contiguous().view(torch.int32)
    b = ref.data[:n_chunks * ref.stride].view(n_chunks, ref.stride)[:, ref.stride - 4 * nwords:].contiguous().view(torch.int32)
    col = torch.arange(a.shape[1], device=dev)[None, :]
    assert int(((a != b) & (col >= nwords - (ref.nbits.to(torch.int64)[:, None] // 32))).sum()) == 0
    _check_sample_against_oracle(enc, [0, 1, 777, n_chunks - 1], lambda row: orc.rans_encode(row, freq),
                                 [sym[c].cpu().numpy() for c in [0, 1, 777, n_chunks - 1]])


def test_rans_tests_with_slot_writer_forced():
    """every rANS test of this file and the rANS goldens once more with SCL_RANS_ENC_WRITER=S: small, ragged and
    odd-alphabet batches through the slot-ring writer (the variable is read once per process, hence the subprocess)"""
    import subprocess, sys
    env = dict(os.environ, SCL_RANS_ENC_WRITER="S")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_batch.py"),
                        os.path.join(here, "test_gpu_goldens.py"), "-q", "-m", "gpu", "-x", "-k",
                        "rans and not slot_writer and not full_occupancy", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_tans_tests_with_table_kernels_forced():
    """tANS models whose tables fit LDS run the table-free rANS kernels by default (same stream, faster here); every tANS
    test of the suite once more with SCL_TANS_KERNELS=table, i.e. on the lookup-table kernels of scl_tans_fast.hip"""
    import subprocess, sys
    env = dict(os.environ, SCL_TANS_KERNELS="table")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_batch.py"),
                        os.path.join(here, "test_gpu_goldens.py"), os.path.join(here, "test_gpu_guard_bands.py"),
                        os.path.join(here, "test_gpu_stream_goldens.py"), "-q", "-m", "gpu", "-x", "-k",
                        "tans and not table_kernels_forced and not slot_writer", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def _check_sample_against_oracle(enc, sample, o_enc, sym_rows):
    offs, nbits = enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c, row in zip(sample, sym_rows):
        rb, rn = o_enc(row)
        assert int(nbits[c]) == rn, f"chunk {c}"
        lo = int(offs[c]) // 8
        window = enc.data[lo:lo + (rn + 7) // 8 + 2].cpu().numpy()
        bits = np.unpackbits(window)[int(offs[c]) % 8:][:rn]
        assert np.array_equal(bits, np.unpackbits(rb)[:rn]), f"chunk {c}"


@pytest.mark.parametrize("f", [1, 2, 16, 256])
def test_range_uniform_table_kernels_vs_oracle(f, dev):
    """256 symbols of one power-of-two frequency (total 256 f, up to BOTTOM = 2^16): the table-free range-coder kernels
    (MODE 2 in scl_range_fast.hip; configs[2] is f = 1).  Ragged batch against the oracle, bit for bit."""
    freq = np.full(256, f, dtype=np.int64)
    rng = np.random.default_rng(300 + f)
    lens = [0, 1, 2, 3, 15, 16, 17, 127, 128, 129, 1000, 4096, 4097] + [int(x) for x in rng.integers(1, 3000, 19)]
    rows = [rng.integers(0, 256, n).astype(np.uint8) for n in lens]
    # a few rows that hug the ends of the alphabet (carry-less resets, long runs of equal bytes)
    rows += [np.zeros(777, np.uint8), np.full(777, 255, np.uint8), np.tile(np.array([255, 0], np.uint8), 400)]
    model = models.RangeModel(freq.tolist(), 32, 32)
    assert model.fast_path()
    cap = max(len(r) for r in rows)
    sym = np.zeros((len(rows), (cap + 15) // 16 * 16), dtype=np.uint8)
    for i, r in enumerate(rows):
        sym[i, :len(r)] = r
    lens_t = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=lens_t)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    offs, nbits = enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    dec_h, dl = dec.cpu().numpy(), dlens.cpu().numpy()
    for i, r in enumerate(rows):
        rb, rn = orc.range_encode(r, freq)
        assert int(nbits[i]) == rn, (i, len(r))
        lo = int(offs[i]) // 8
        window = enc.data[lo:lo + (rn + 7) // 8 + 2].cpu().numpy()
        bits = np.unpackbits(window)[int(offs[i]) % 8:][:rn]
        assert np.array_equal(bits, np.unpackbits(rb)[:rn]), (i, len(r))
        assert int(dl[i]) == len(r) and np.array_equal(dec_h[i, :len(r)], r), (i, len(r))
    assert torch.equal(used, enc.nbits)


def test_config3_range_coder_full_size_properties(dev):
    """BASELINE.json configs[2]: 32-bit range coder on 1 GiB of uniform bytes (f = 1, M = 256), 262 144 chunks of
    4 KiB.  decode(encode(x)) == x for every chunk, consumed == produced, every stream is the 32-bit header plus
    4096 + 3 bytes, a few more after a carry-less range reset (SURVEY 8a/a10 measured 32 824 bits), and a fixed sample equals the oracle bit for bit."""
    freq = np.ones(256, dtype=np.int64)
    n_chunks, chunk_len = 262144, 4096
    model = models.RangeModel(freq.tolist(), 32, 32)
    sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=3, device=dev)
    enc = model.encode_batch(sym)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, chunk_len)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    assert torch.equal(dec[:, :chunk_len], sym) and torch.equal(used, enc.nbits)
    assert int(dlens.min()) == chunk_len == int(dlens.max())
    nb = enc.nbits.cpu().numpy()
    assert np.all((nb - 32) % 8 == 0) and 4099 <= (nb.min() - 32) // 8 and (nb.max() - 32) // 8 <= 4104, np.unique(nb)
    assert np.mean(nb <= 32832) > 0.9  # 4099 or 4100 bytes almost always
    sample = [0, 1, 4095, 131072, n_chunks - 1]
    _check_sample_against_oracle(enc, sample, lambda s: orc.range_encode(s, freq), [sym[c].cpu().numpy() for c in sample])


def test_config4_order1_arithmetic_full_size_properties(dev):
    """BASELINE.json configs[3]: order-1 adaptive arithmetic coding of a Markov-1 source, K = 16, per-lane context
    tables in LDS, 65 536 chunks of 4 KiB: round trip for every chunk, consumed == produced, oracle equality on a
    sample, and the code length is within 3 % of the source's empirical conditional entropy + learning cost."""
    K, n_chunks, chunk_len = 16, 65536, 4096
    base = np.stack([bench_data.markov1_host(K, chunk_len, seed=400 + c) for c in range(128)])
    sym = torch.from_numpy(base).to(dev).repeat(n_chunks // 128, 1)
    model = models.AecModel(2, None, K, 1, 1 << 30, 32, 32)
    assert model.fast_path(chunk_len)
    enc = model.encode_batch(sym)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, chunk_len)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    assert torch.equal(dec[:, :chunk_len], sym) and torch.equal(used, enc.nbits)
    sample = [0, 1, 127, 128, 4095, n_chunks - 1]
    _check_sample_against_oracle(enc, sample, lambda s: orc.aec_encode(s, orc.MODEL_ORDERK, K, k=1),
                                 [base[c % 128] for c in sample])
    # identical inputs -> identical streams, whatever lane / workgroup coded them
    nb = enc.nbits.view(n_chunks // 128, 128)
    assert bool((nb == nb[0:1]).all())
    # adaptive code length: sum over symbols of -log2((count + 1) / (total + K)) computed on the host for chunk 0
    cnt = np.ones((K, K)); prev = 0; ideal = 0.0
    for x in base[0]:
        ideal -= np.log2(cnt[prev, x] / cnt[prev].sum()); cnt[prev, x] += 1; prev = int(x)
    got = int(enc.nbits[0].item()) - 32
    assert abs(got - ideal) < 0.002 * ideal + 8, (got, ideal)


def _random_pow2_table(rng, K, m_log2):
    """K frequencies >= 1 summing to 2^m_log2, from flat to extremely skewed"""
    M = 1 << m_log2
    alpha = float(rng.choice([0.05, 0.3, 1.0, 20.0]))
    w = rng.dirichlet(np.full(K, alpha))
    f = np.maximum(1, np.floor(w * (M - K)).astype(np.int64) + 1)
    while f.sum() > M:
        f[np.argmax(f)] -= 1
    f[np.argmax(f)] += M - f.sum()
    assert f.sum() == M and f.min() >= 1
    return f.astype(np.uint32)


def _also_on_striped_slots(model, d_sym, d_lens, enc, cap, tag):
    """the same batch on wave-striped slots (ABI 8) where the model is served: same descriptors, same dense and framed
    bytes as the linear batch `enc` (whose streams the caller has just compared with the oracle's), same decode"""
    if not model.striped_ok():
        return
    st = model.encode_batch(d_sym, lens=d_lens, layout="striped")
    assert int(st.status.abs().sum()) == 0 and torch.equal(st.nbits, enc.nbits) and torch.equal(st.bit_offset, enc.bit_offset), tag
    for framed in (False, True):
        a, ao = models.compact(enc, framed=framed)
        b, bo = models.compact(st, framed=framed)
        assert torch.equal(ao, bo) and torch.equal(a[:int(ao[-1])], b[:int(ao[-1])]), (tag, framed)
    dec, dlens, used, status = model.decode_encoded(st, cap)
    dec_l, dlens_l, used_l, _ = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    assert int(status.abs().sum()) == 0 and torch.equal(dlens, dlens_l) and torch.equal(used, used_l), tag
    keep = torch.arange(cap, device=dec.device)[None, :] < dlens[:, None]
    assert torch.equal(dec * keep, dec_l * keep), tag


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCL_RANDOM_SEEDS", 20))))
def test_random_models_fast_paths_vs_oracle(seed, dev):
    """Differential test of the tuned kernels (rANS / tANS / range fast paths) on random power-of-two tables:
    alphabets 2..256, totals 2^1..2^12, flat to extremely skewed, symbols drawn from the table and -- to hit the
    longest fields -- from a uniform distribution; 40 ragged chunks per model, every stream equal to the oracle's,
    every decode equal to the input with the exact bit count."""
    rng = np.random.default_rng(9000 + seed)
    K = int(rng.choice([2, 3, 5, 16, 17, 100, 255, 256]))
    m_log2 = int(rng.integers(max(1, int(np.ceil(np.log2(K)))), 13))
    if seed >= 12:  # small tables: totals 2..128 (m < 32 - NUM_STATE_BITS, the pre-shifted quotient of the encoder)
        K = int(rng.choice([2, 3, 5, 16, 17]))
        m_log2 = int(rng.integers(max(1, int(np.ceil(np.log2(K)))), 8))
    f = _random_pow2_table(rng, K, m_log2)
    cap = 640
    lens = np.concatenate([[0, 1, 127, 128, 129, 255, 256, 257, 640], rng.integers(0, cap + 1, 31)]).astype(np.int32)
    p = f / f.sum()
    sym = np.stack([rng.choice(K, cap, p=p) if c % 3 else rng.integers(0, K, cap) for c in range(lens.size)]).astype(np.uint8)
    d_sym, d_lens = torch.from_numpy(sym).to(dev), torch.from_numpy(lens).to(dev)
    cases = [("rans", models.RansModel(f.tolist(), 1 << 16, 1, 32), lambda s: orc.rans_encode(s, f)),
             ("range", models.RangeModel(f.tolist(), 32, 32), lambda s: orc.range_encode(s, f))]
    if m_log2 <= 12:
        cases.append(("tans", models.TansModel(f.tolist(), 1, 32), lambda s: orc.tans_encode(s, f, RF=1)))
    for name, model, o_enc in cases:
        enc = model.encode_batch(d_sym, lens=d_lens)
        dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0, name
        data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
        dec = dec.cpu().numpy()
        assert np.array_equal(dlens.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), nbits), name
        for c in range(lens.size):
            rb, rn = o_enc(sym[c, :lens[c]])
            assert int(nbits[c]) == rn, f"{name} K={K} M=2^{m_log2} chunk {c}"
            assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"{name} chunk {c}"
            assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"{name} chunk {c}"
        _also_on_striped_slots(model, d_sym, d_lens, enc, cap, f"{name} K={K} M=2^{m_log2}")


@pytest.mark.parametrize("mode", ["fixed", "order1", "iid", "rans", "tans", "range", "rans_total_3000"])
def test_tuned_kernels_full_occupancy_stress(mode, dev):
    """1 GiB batches, three times: every tuned kernel family against the any-parameter kernels word for word
    (encode) and against the input (decode).  A timing-dependent fault of about 3 wrong words per GiB in an
    earlier forward writer (64-bit shift with a just-computed amount, see SclFwdBits::put) was only visible at
    this scale; nothing smaller would have caught it."""
    n_chunks, chunk_len = 262144, 4096
    if mode == "fixed":
        freq = bench_data.t256_table()
        sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=5000, device=dev)
        model = models.AecModel(0, freq.tolist(), 256, 0, 1 << 30, 32, 32)
    elif mode in ("rans", "tans", "range", "rans_total_3000"):
        freq = bench_data.t256_table()
        if mode == "rans_total_3000":  # a total that is not a power of two: the binary64 division of the decoder
            freq = np.maximum(1, (freq.astype(np.int64) * 3000) // 4096)
            freq[np.argmax(freq)] += 3000 - freq.sum()
        sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=5002, device=dev)
        model = {"rans": lambda: models.RansModel(freq.tolist(), 1 << 16, 1, 32),
                 "rans_total_3000": lambda: models.RansModel(freq.tolist(), 1 << 16, 1, 32),
                 "tans": lambda: models.TansModel(freq.tolist(), 1, 32),
                 "range": lambda: models.RangeModel(freq.tolist(), 32, 32)}[mode]()
    elif mode == "iid":
        n_chunks = 65536
        freq = bench_data.t256_table()
        sym = bench_data.iid_chunks_device(freq, n_chunks, chunk_len, seed=5001, device=dev)
        model = models.AecModel(1, [1] * 256, 256, 0, 1 << 30, 32, 32)
    else:
        sym = bench_data.markov1_chunks_device(16, n_chunks, chunk_len, seed=900, device=dev)  # all chunks distinct
        model = models.AecModel(2, None, 16, 1, 1 << 30, 32, 32)
    if isinstance(model, models.AecModel):
        assert model.fast_path(chunk_len)
    ref = model.encode_batch(sym, any_parameter_kernels=True)
    torch.cuda.synchronize()
    # ... and the any-parameter kernels' own streams against the ORACLE on a sample of the distinct-data batch (VERDICT r5
    # weak #11: word-for-word agreement of two GPU implementations alone would not notice a shared misreading)
    sample = [0, 1, 63, 64, 255, 256, 4095, n_chunks // 2, n_chunks - 2, n_chunks - 1]
    o_enc = {"fixed": lambda s_: orc.aec_encode(s_, orc.MODEL_FIXED, 256, f_init=freq),
             "iid": lambda s_: orc.aec_encode(s_, orc.MODEL_IID, 256, f_init=np.ones(256)),
             "order1": lambda s_: orc.aec_encode(s_, orc.MODEL_ORDERK, 16, k=1),
             "rans": lambda s_: orc.rans_encode(s_, freq), "rans_total_3000": lambda s_: orc.rans_encode(s_, freq),
             "tans": lambda s_: orc.tans_encode(s_, freq, RF=1), "range": lambda s_: orc.range_encode(s_, freq)}[mode]
    host_rows = sym[sample].cpu().numpy()
    s_off, s_nb = ref.bit_offset[sample].cpu().numpy(), ref.nbits[sample].cpu().numpy()
    for j, c in enumerate(sample):
        rb, rn = o_enc(host_rows[j])
        assert int(s_nb[j]) == rn, f"{mode} chunk {c}: {s_nb[j]} bits vs oracle {rn}"
        lo = int(s_off[j]) // 8
        piece = ref.data[lo:lo + (int(s_off[j]) % 8 + rn + 7) // 8 + 1].cpu().numpy()
        assert np.array_equal(_stream_bits(piece, int(s_off[j]) % 8, rn), np.unpackbits(rb)[:rn]), f"{mode} chunk {c} vs oracle"
    stride = ref.stride
    nwords = int((ref.nbits.max().item() + 31) // 32)
    back = mode in ("rans", "tans", "rans_total_3000")  # ANS streams end at the slot end, the others start at its front

    def words(e):
        rows = e.data[:n_chunks * stride].view(n_chunks, stride)
        rows = rows[:, stride - 4 * nwords:] if back else rows[:, :4 * nwords]
        return rows.contiguous().view(torch.int32)

    b = words(ref)
    full = (ref.nbits.to(torch.int64)[:, None] // 32)
    col = torch.arange(nwords, device=dev)[None, :]
    whole = (col >= nwords - full) if back else (col < full)
    ref_nbits = ref.nbits.clone()
    del ref
    for rep in range(3):
        enc = model.encode_batch(sym)
        dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, chunk_len)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
        assert torch.equal(enc.nbits, ref_nbits)
        a = words(enc)
        assert int(((a != b) & whole).sum()) == 0, f"rep {rep}: stream words differ from the any-parameter kernel"
        assert torch.equal(dec[:, :chunk_len], sym), f"rep {rep}: decode"
        del enc, dec, a


@pytest.mark.parametrize("K", [2, 5, 127, 128, 129, 200, 255])
def test_symbol_range_check_boundaries(K, dev):
    """ST_SYMBOL (the reference's KeyError, prob_dist.py:208) from the tuned rANS encoder's four-symbols-at-a-time
    test: K - 1 is the last valid index, K the first invalid one, wherever it sits in a line, a 16-byte block or the
    ragged tail; chunks without an invalid symbol stay clean."""
    f = np.ones(K, dtype=np.int64)
    f[0] += 4096 - K
    model = models.RansModel(f.tolist(), 1 << 16, 1, 32)
    n = 128 * 3 + 16 * 2 + 7
    rng = np.random.default_rng(K)
    positions = [0, 1, 2, 3, 63, 127, 128, 255, 383, 384, 399, 400, 415, 416, 422]
    sym = rng.integers(0, K, (2 * len(positions) + 2, n)).astype(np.uint8)
    expect = np.zeros(sym.shape[0], dtype=bool)
    for i, p in enumerate(positions):
        sym[2 * i, p] = K - 1                    # largest valid symbol: no flag
        sym[2 * i + 1, p] = K                    # first invalid symbol
        expect[2 * i + 1] = True
    sym[-1, 200] = 255
    expect[-1] = K <= 255
    enc = model.encode_batch(torch.from_numpy(sym).to(dev))
    torch.cuda.synchronize()
    flagged = (enc.status.cpu().numpy() & backend_lib.ST_SYMBOL) != 0
    assert np.array_equal(flagged, expect), np.nonzero(flagged != expect)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCL_RANDOM_SEEDS", 12))))
def test_random_arithmetic_models_vs_oracle(seed, dev):
    """Differential test of the three tuned arithmetic-coder kernel families on random models: static tables
    (any total up to 2^16), adaptive i.i.d. models with random initial counts (alphabets 2..256) and order-k models
    (K^k <= 16 contexts in LDS, more than 256 cells in device-memory lines / rows); 24 ragged chunks each, streams and consumed-bit counts against the oracle.
    SCL_RANDOM_SEEDS=300 turns this (and the ANS / range twin above) into a campaign."""
    rng = np.random.default_rng(40000 + seed)
    cap = 400
    lens = np.concatenate([[0, 1, 2, 127, 128, 129, 400], rng.integers(0, cap + 1, 17)]).astype(np.int32)
    kind = ["fixed", "iid", "orderk"][seed % 3]
    sb = int(rng.choice([32, 32, 9, 17, 24, 31]))  # DATA_BLOCK_SIZE_BITS (cap = 400 < 2^9)
    if kind == "fixed":
        K = int(rng.integers(2, 257))
        T = int(rng.integers(K, 65537))
        f = np.maximum(1, np.floor(rng.dirichlet(np.full(K, float(rng.choice([0.1, 1.0, 10.0])))) * (T - K)).astype(np.int64) + 1)
        f[np.argmax(f)] += T - f.sum()
        f = f.astype(np.uint32)
        model = models.AecModel(0, f.tolist(), K, 0, 1 << 30, 32, sb)
        o_enc = lambda s: orc.aec_encode(s, orc.MODEL_FIXED, K, f_init=f, size_bits=sb)
        o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_FIXED, K, f_init=f, size_bits=sb)
        p = f / f.sum()
    elif kind == "iid":
        K = int(rng.integers(2, 257))
        f = rng.integers(1, 60, K).astype(np.uint32)
        model = models.AecModel(1, f.tolist(), K, 0, 1 << 30, 32, sb)
        o_enc = lambda s: orc.aec_encode(s, orc.MODEL_IID, K, f_init=f, size_bits=sb)
        o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_IID, K, f_init=f, size_bits=sb)
        p = rng.dirichlet(np.full(K, 0.3))
    else:
        combos = [(2, 1), (2, 3), (3, 2), (4, 2), (7, 1), (16, 1), (13, 1), (16, 0), (4, 1),
                  (7, 2), (5, 3), (20, 1), (40, 1), (16, 2), (200, 1)]  # the last six: one line per context, then dense rows
        K, k = combos[int(rng.integers(0, len(combos)))]
        model = models.AecModel(2, None, K, k, 1 << 30, 32, sb)
        o_enc = lambda s: orc.aec_encode(s, orc.MODEL_ORDERK, K, k=k, size_bits=sb)
        o_dec = lambda p, nb: orc.aec_decode(p, nb, orc.MODEL_ORDERK, K, k=k, size_bits=sb)
        p = rng.dirichlet(np.full(K, 0.5))
    assert model.fast_path(cap), kind
    sym = rng.choice(K, (lens.size, cap), p=p).astype(np.uint8)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0, kind
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    dec, used = dec.cpu().numpy(), used.cpu().numpy()
    assert np.array_equal(dlens.cpu().numpy(), lens)
    for c in range(lens.size):
        rb, rn = o_enc(sym[c, :lens[c]])
        assert int(nbits[c]) == rn, f"{kind} K={K} chunk {c}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"{kind} K={K} chunk {c}"
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"{kind} K={K} chunk {c}"
        if lens[c] > 0:
            assert used[c] == o_dec(rb, rn)[1], f"{kind} K={K} chunk {c}"


@pytest.mark.parametrize("precision", [33, 40, 48, 56, 62])
@pytest.mark.parametrize("kind", ["fixed", "iid", "orderk"])
def test_arithmetic_wide_precision_vs_oracle(precision, kind, dev):
    """PRECISION above 32 (round 3): the any-parameter kernels with low / high in 128 bits against the oracle (pinned on
    the reference's PRECISION 40 / 48 goldens, G7wide); ragged chunks, streams and consumed-bit counts; totals up to
    2^31 for the static model (the products then need all 128 bits)."""
    rng = np.random.default_rng(precision * 7 + len(kind))
    cap = 300
    lens = np.concatenate([[0, 1, 2, 299, 300], rng.integers(0, cap + 1, 11)]).astype(np.int32)
    max_total = 1 << (precision - 2)
    if kind == "fixed":
        K = 37
        f = rng.integers(1, 1 << 26, K).astype(np.uint32)  # total ~2^30
        model = models.AecModel(0, f.tolist(), K, 0, max_total, precision, 32)
        kw = dict(model_kind=orc.MODEL_FIXED, K=K, f_init=f)
        p = f / f.sum()
    elif kind == "iid":
        K = 20
        f = rng.integers(1, 60, K).astype(np.uint32)
        model = models.AecModel(1, f.tolist(), K, 0, max_total, precision, 32)
        kw = dict(model_kind=orc.MODEL_IID, K=K, f_init=f)
        p = rng.dirichlet(np.full(K, 0.3))
    else:
        K, k = 5, 2
        model = models.AecModel(2, None, K, k, max_total, precision, 32)
        kw = dict(model_kind=orc.MODEL_ORDERK, K=K, k=k)
        p = rng.dirichlet(np.full(K, 0.5))
    kw.update(max_total=max_total, precision=precision, size_bits=32)
    assert not model.fast_path(cap)
    sym = rng.choice(K, (lens.size, cap), p=p).astype(np.uint8)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    dec, used = dec.cpu().numpy(), used.cpu().numpy()
    assert np.array_equal(dlens.cpu().numpy(), lens)
    for c in range(lens.size):
        rb, rn = orc.aec_encode(sym[c, :lens[c]], **kw)
        assert int(nbits[c]) == rn, (kind, precision, c)
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), (kind, precision, c)
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), (kind, precision, c)
        if lens[c] > 0:
            assert used[c] == orc.aec_decode(rb, rn, **kw)[1], (kind, precision, c)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCL_RANDOM_SEEDS", 16))))
def test_random_totals_fast_paths_vs_oracle(seed, dev):
    """rANS with ANY total 2..4096 (the reference does not ask for a power of two, and its own tests use 5, 30, 92,
    874 ...): the tuned kernels divide by the total exactly in binary64 and pick the renormalised width with one
    comparison.  Random totals, alphabets and RANGE_FACTORs; 40 ragged chunks against the oracle."""
    rng = np.random.default_rng(70000 + seed)
    K = int(rng.choice([2, 3, 5, 6, 17, 100, 256]))
    M = int(rng.integers(max(K, 2), 4097))
    if seed % 5 == 0:
        M = int(rng.choice([5, 30, 92, 874, 4095, 3, 2049]))
        K = min(K, M)
    cuts = np.sort(rng.choice(np.arange(1, M), K - 1, replace=False)) if K > 1 else np.array([], dtype=np.int64)
    f = np.diff(np.concatenate([[0], cuts, [M]])).astype(np.uint32)
    assert f.sum() == M and f.min() >= 1
    rf = int(rng.choice([1 << 16, 1 << 16, 1 << 8, 1 << 12, 1, 2]))
    rans = models.RansModel(f.tolist(), rf, 1, 32)
    assert rans.info().fast_path == 1, (M, rf)
    cap = 640
    lens = np.concatenate([[0, 1, 127, 128, 129, 255, 256, 257, 640], rng.integers(0, cap + 1, 31)]).astype(np.int32)
    p = f / f.sum()
    sym = np.stack([rng.choice(K, cap, p=p) if c % 3 else rng.integers(0, K, cap) for c in range(lens.size)]).astype(np.uint8)
    d_sym, d_lens = torch.from_numpy(sym).to(dev), torch.from_numpy(lens).to(dev)
    # the range coder's tuned kernels take any total up to 4096 as well (range // M in binary64)
    for name, model, o_enc in [("rans", rans, lambda s: orc.rans_encode(s, f, RF=rf)),
                               ("range", models.RangeModel(f.tolist(), 32, 32), lambda s: orc.range_encode(s, f))]:
        enc = model.encode_batch(d_sym, lens=d_lens)
        dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0, name
        data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
        dec = dec.cpu().numpy()
        assert np.array_equal(dlens.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), nbits), name
        for c in range(lens.size):
            rb, rn = o_enc(sym[c, :lens[c]])
            assert int(nbits[c]) == rn, f"{name} M={M} RF={rf} chunk {c}"
            assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"{name} M={M} chunk {c}"
            assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"{name} M={M} chunk {c}"
        _also_on_striped_slots(model, d_sym, d_lens, enc, cap, f"{name} M={M} RF={rf}")


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCL_RANDOM_SEEDS", 10))))
def test_range_coder_large_totals_vs_oracle(seed, dev):
    """Range coder with totals above 4096 and up to BOTTOM = 2^16 (the reference's own extreme tables are {1, 65535}
    and {1, 1, 65534}, range_coder.py:336-374): the tuned decoder finds the symbol by binary search on the
    cumulative counts.  30 ragged chunks against the oracle."""
    rng = np.random.default_rng(81000 + seed)
    if seed == 0:
        f = np.array([1, 65535], dtype=np.uint32)
    elif seed == 1:
        f = np.array([1, 1, 65534], dtype=np.uint32)
    else:
        K = int(rng.choice([2, 5, 17, 100, 256]))
        M = int(rng.integers(4097, 65537))
        cuts = np.sort(rng.choice(np.arange(1, M), K - 1, replace=False))
        f = np.diff(np.concatenate([[0], cuts, [M]])).astype(np.uint32)
    K = f.size
    model = models.RangeModel(f.tolist(), 32, 32)
    assert model.fast_path()
    cap = 520
    lens = np.concatenate([[0, 1, 2, 127, 128, 129, 520], rng.integers(0, cap + 1, 23)]).astype(np.int32)
    p = f / f.sum()
    sym = np.stack([rng.choice(K, cap, p=p) if c % 3 else rng.integers(0, K, cap) for c in range(lens.size)]).astype(np.uint8)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    dec = dec.cpu().numpy()
    assert np.array_equal(dlens.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), nbits)
    for c in range(lens.size):
        rb, rn = orc.range_encode(sym[c, :lens[c]], f)
        assert int(nbits[c]) == rn, f"chunk {c}"
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"


def test_tans_reference_default_range_factor(dev):
    """tANSParams inherits RANGE_FACTOR = 2^16 from rANSParams (tANS.py:31-53): with a 4096-total table that asks for
    2^28-entry lookup tables.  tANS is rANS with its steps cached and writes the same stream (golden group G5), so such
    models run on the table-free rANS kernels: batch API and drop-in classes against the rANS oracle."""
    freq = bench_data.t256_table()
    model = models.TansModel(freq.tolist(), 1 << 16, 32)
    assert model.info().fast_path == 1
    lens = np.array([0, 1, 17, 127, 128, 129, 300, 512], dtype=np.int32)
    sym = bench_data.iid_chunks_host(freq, len(lens), 512, seed=77)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, 512)
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    assert np.array_equal(dlens.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), nbits)
    for c in range(len(lens)):
        rb, rn = orc.rans_encode(sym[c, :lens[c]], freq, RF=1 << 16)
        assert int(nbits[c]) == rn
        assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn])
        assert np.array_equal(dec[c, :lens[c]].cpu().numpy(), sym[c, :lens[c]])
    # drop-in classes with the reference's defaults, a block whose length is not a multiple of 16
    from stanford_compression_library_amd.compressors.tANS import tANSDecoder, tANSEncoder, tANSParams
    from stanford_compression_library_amd.core.data_block import DataBlock
    from stanford_compression_library_amd.core.prob_dist import Frequencies

    params = tANSParams(Frequencies({i: int(f) for i, f in enumerate(freq)}))
    block = DataBlock(sym[6, :301].tolist())
    bits = tANSEncoder(params).encode_block(block)
    rb, rn = orc.rans_encode(sym[6, :301], freq, RF=1 << 16)
    assert len(bits) == rn and np.array_equal(bits.packed(), rb)
    out, consumed = tANSDecoder(params).decode_block(bits)
    assert out.data_list == block.data_list and consumed == rn


@pytest.mark.parametrize("name", ["rans_default", "tans_rf1"])
@pytest.mark.parametrize("n", [128, 1000, 4096])
def test_cooperative_line_store_full_and_partial_waves(name, n, dev):
    """The rANS / tANS decoders store whole waves of equally long chunks cooperatively (CoopLineStore: the lanes
    l, l+16, l+32, l+48 share a half-line after a register transpose) and everything else lane by lane.  One launch
    holds both kinds of wave: 128 equal chunks (two cooperating waves), a wave where one chunk is shorter by a line,
    a wave with a truncated stream descriptor, and a partial wave; every row must equal its input, bytes of a row
    beyond the chunk must stay untouched, and a sample is compared with the oracle's decode."""
    make_model, o_enc, o_dec = CODERS[name]
    freq = bench_data.t256_table()
    model = make_model(freq)
    n_chunks = 64 * 4 + 19
    sym = bench_data.iid_chunks_host(freq, n_chunks, n, seed=77 + n)
    lens = np.full(n_chunks, n, dtype=np.int32)
    lens[128 + 5] = n - 128 if n > 128 else 1  # third wave: one lane a line behind the others
    d_sym, d_lens = torch.from_numpy(sym).to(dev), torch.from_numpy(lens).to(dev)
    enc = model.encode_batch(d_sym, lens=d_lens)
    avail = enc.nbits.clone()
    avail[192 + 7] = 10  # fourth wave: one stream too short for its header -> that lane leaves early
    out = model.alloc_decoded(n_chunks, n + 64, dev)
    out[0].fill_(0xA5)
    dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, avail, n + 64, out=out)
    torch.cuda.synchronize()
    status, dec = status.cpu().numpy(), dec.cpu().numpy()
    assert status[192 + 7] != 0 and int(np.abs(np.delete(status, 192 + 7)).sum()) == 0
    for c in range(n_chunks):
        if c == 192 + 7:
            continue
        assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        assert (dec[c, lens[c]:] == 0xA5).all(), f"chunk {c}: bytes beyond the chunk were written"
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in (0, 17, 63, 64, 127, 133, 191, 256, n_chunks - 1):
        bits = _stream_bits(data, offs[c], nbits[c])
        o_sym, o_used = o_dec(np.packbits(bits), int(nbits[c]), freq)
        assert o_used == nbits[c] == used[c].item()
        assert np.array_equal(np.asarray(o_sym), dec[c, :lens[c]])


_T86 = np.array([3, 1, 7, 2, 19, 40, 5, 9], dtype=np.int64)  # total 86 (tests/test_gpu_decoder_fuzz.py): the ML_T < 0 decoder
# decoder -> (model, table, slot layout, oracle arguments of orc.rans_encode, environment, the decode kernel that must serve it)
FRAME_DECODERS = {
    "rans_b1_linear": (lambda f: models.RansModel(f.tolist(), 1 << 16, 1, 32), None, "linear", dict(RF=1 << 16), {},
                       "rans_decode_fast_kernel<12, 3, 256, 1, false>"),
    "rans_b1_striped": (lambda f: models.RansModel(f.tolist(), 1 << 16, 1, 32), None, "striped", dict(RF=1 << 16), {},
                        "rans_decode_fast_kernel<12, 3, 256, 1, true>"),
    "rans_total86": (lambda f: models.RansModel(f.tolist(), 1 << 16, 1, 32), _T86, "linear", dict(RF=1 << 16), {},
                     "rans_decode_fast_kernel<-1, 0, 256, 1, false>"),
    "rans_b8": (lambda f: models.RansModel(f.tolist(), 1 << 8, 8, 32), None, "linear", dict(RF=1 << 8, b=8), {},
                "rans_decode_fast_kernel<0, 0, 256, 0, false>"),
    "rans_b2": (lambda f: models.RansModel(f.tolist(), 1 << 8, 2, 32), None, "linear", dict(RF=1 << 8, b=2), {},
                "rans_decode_fastb_kernel"),
    "tans_table": (lambda f: models.TansModel(f.tolist(), 1, 32), None, "linear", dict(RF=1), {"SCL_TANS_KERNELS": "table"},
                   "tans_decode_fast_kernel"),
}


@pytest.mark.parametrize("name", list(FRAME_DECODERS))
def test_ans_decode_frame(name, dev, monkeypatch):
    """What stands around the symbol step of every tuned ANS decoder (scl_ans_frame.h: header exit, ragged head, 16-byte
    blocks, cooperative line loop, status epilogue), on each decoder that uses it.  One launch of 64 x 3 + 19 chunks: a wave
    of 64 equal chunks of 256 symbols (cooperative store, two lines); a wave whose lengths sit on every loop boundary (not
    cooperating); a wave of 64 equal chunks of 128 where one lane's stream is too short for its header (the header exit
    inside a would-be cooperating wave); a partial wave of 19 equal chunks of 256."""
    make_model, table, layout, o_args, env, kernel = FRAME_DECODERS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    freq = bench_data.t256_table() if table is None else table
    model = make_model(freq)
    edges = [0, 1, 15, 16, 17, 112, 127, 128, 129, 143, 144, 255, 256, 257]
    lens = np.array([256] * 64 + [edges[i % len(edges)] for i in range(64)] + [128] * 64 + [256] * 19, dtype=np.int32)
    n_chunks, cap, cut = lens.size, 272, 128 + 37
    assert model.info().fast_path and model.kernel_names(n_chunks, layout)[1].startswith(kernel)
    sym = bench_data.iid_chunks_host(freq, n_chunks, cap, seed=4242)
    d_lens = torch.from_numpy(lens).to(dev)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=d_lens, layout=layout)
    avail = enc.nbits.clone()
    avail[cut] = 10
    got = []
    for generic in (False, True):
        out = model.alloc_decoded(n_chunks, cap, dev)
        out[0].fill_(0xA5)
        if generic:
            res = model.decode_batch(enc.linear_data(), enc.bit_offset, avail, cap, out=out, any_parameter_kernels=True)
        else:
            res = model.decode_batch(enc.data, enc.bit_offset, avail, cap, out=out,
                                     striped_stride=enc.stride if layout == "striped" else None)
        torch.cuda.synchronize()
        got.append([t.cpu().numpy() for t in res])
    dec, dlens, used, status = got[0]
    nbits = enc.nbits.cpu().numpy()
    want_lens = lens.copy()
    want_lens[cut] = 0
    assert np.array_equal(dlens, want_lens)
    assert status[cut] == backend_lib.ST_TRUNCATED and not np.delete(status, cut).any() and not enc.status.cpu().numpy().any()
    assert np.array_equal(np.delete(used, cut), np.delete(nbits, cut))
    for c in range(n_chunks):
        assert np.array_equal(dec[c, :want_lens[c]], sym[c, :want_lens[c]]), f"chunk {c}"
        assert (dec[c, want_lens[c]:] == 0xA5).all(), f"chunk {c}: bytes beyond the chunk were written"
    for what, a, b in zip(("symbols", "lengths", "consumed bits", "status"), got[0], got[1]):
        assert np.array_equal(a, b), f"tuned and any-parameter decoders differ in {what}"
    if layout == "linear":
        data, offs = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy()
        for c in (0, 63, 64, 65, 70, 77, 127, 128, cut, 191, 192, n_chunks - 1):
            rb, rn = orc.rans_encode(sym[c, :lens[c]], freq, **o_args)
            assert int(nbits[c]) == rn and np.array_equal(_stream_bits(data, offs[c], rn), np.unpackbits(rb)[:rn]), f"chunk {c}"


@pytest.mark.parametrize("seed", range(int(os.environ.get("SCL_RANDOM_SEEDS", 16))))
def test_random_models_num_bits_out_vs_oracle(seed, dev):
    """NUM_BITS_OUT in {2, 4, 8, 16} (the reference's own sweep uses 8, rANS.py:366-379) on the tuned kernels -- b = 2, and
    what scl_rans_fast.hip excludes, on scl_rans_fast_b.hip; b in {4, 8, 16} within their bounds on scl_rans_fast.hip:
    random power-of-two tables, RANGE_FACTOR as large as H < 2^31 and RF 2^b <= 2^24 allow (or
    small), ragged chunks, symbols from the table and from a uniform distribution; streams equal to the oracle's,
    decode equal to the input with the exact bit count -- and the same through the any-parameter kernels."""
    rng = np.random.default_rng(31000 + seed)
    b = int(rng.choice([2, 4, 8, 16]))
    K = int(rng.choice([2, 3, 5, 16, 17, 100, 255, 256]))
    m_log2 = int(rng.integers(max(1, int(np.ceil(np.log2(K)))), 13))
    r_max = min(24 - b, 31 - b - m_log2)
    if r_max < 0:
        m_log2 = 31 - b  # only for b = 16 with big tables: shrink the table instead
        K = min(K, 1 << m_log2)
        r_max = 0
    r = int(rng.integers(0, r_max + 1)) if seed % 3 else r_max
    RF = 1 << r
    f = _random_pow2_table(rng, K, m_log2)
    size_bits = int(rng.choice([32, 12, 20]))
    cap = 640
    lens = np.concatenate([[0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 640], rng.integers(0, cap + 1, 29)]).astype(np.int32)
    p = f / f.sum()
    sym = np.stack([rng.choice(K, cap, p=p) if c % 3 else rng.integers(0, K, cap) for c in range(lens.size)]).astype(np.uint8)
    d_sym, d_lens = torch.from_numpy(sym).to(dev), torch.from_numpy(lens).to(dev)
    model = models.RansModel(f.tolist(), RF, b, size_bits)
    assert model.info().fast_path, f"b={b} K={K} M=2^{m_log2} RF=2^{r}: expected the tuned kernels"
    for generic in (False, True):
        enc = model.encode_batch(d_sym, lens=d_lens, any_parameter_kernels=generic)
        dec, dlens, used, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, cap,
                                                      any_parameter_kernels=generic)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0 and int(status.abs().sum()) == 0
        data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
        dec = dec.cpu().numpy()
        assert np.array_equal(dlens.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), nbits)
        for c in range(lens.size):
            rb, rn = orc.rans_encode(sym[c, :lens[c]], f, RF=RF, b=b, size_bits=size_bits)
            assert int(nbits[c]) == rn, f"b={b} K={K} M=2^{m_log2} RF=2^{r} chunk {c} generic={generic}"
            assert np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn]), f"chunk {c}"
            assert np.array_equal(dec[c, :lens[c]], sym[c, :lens[c]]), f"chunk {c}"
        if not generic:  # (NUM_BITS_OUT in {4, 8, 16} within their bounds run on the headline kernels: striped too)
            _also_on_striped_slots(model, d_sym, d_lens, enc, cap, f"b={b} K={K} M=2^{m_log2} RF=2^{r}")


@pytest.mark.parametrize("framed", [False, True])
def test_compact_long_and_tiny_streams(framed, dev):
    """The copy kernel of scl_streams_compact walks a record in 16-byte blocks aligned in the destination, 256 per
    trip of the wave: records of several trips (11 KiB), records shorter than one block or than the 160 source bits
    an interior block needs, and every destination alignment (the records before them have random sizes)."""
    make_model, o_enc, _ = CODERS["rans_default"]
    freq = bench_data.t256_table()
    model = make_model(freq)
    rng = np.random.default_rng(5)
    cap = 12000
    lens = np.concatenate([[cap, 0, 1, 2, 3, cap - 1, 9000, 4500, 4600, 17, 18, 19, 20, 21, 22],
                           rng.integers(0, 64, 40), rng.integers(4000, cap + 1, 12)]).astype(np.int32)
    sym = bench_data.iid_chunks_host(freq, len(lens), cap, seed=22)
    enc = model.encode_batch(torch.from_numpy(sym).to(dev), lens=torch.from_numpy(lens).to(dev))
    dense, offsets = models.compact(enc, framed=framed)
    dense, offsets = dense.cpu().numpy(), offsets.cpu().numpy()
    expect = []
    for c in range(len(lens)):
        rb, rn = o_enc(sym[c, :lens[c]], freq)
        bits = np.unpackbits(rb)[:rn]
        expect.append(_frame_reference(bits) if framed else np.packbits(bits))
    sizes = np.array([e.size for e in expect])
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(sizes)]))
    for c, e in enumerate(expect):
        assert np.array_equal(dense[offsets[c]:offsets[c + 1]], e), f"record {c} (len {lens[c]})"


def test_compact_offsets_past_256_tiles_of_2048_records(dev):
    """The offsets of scl_streams_compact are a scan in three kernels: every tile of 2048 records scans its sizes, ONE
    workgroup scans the tile sums in trips of 256 with a carried prefix, every record adds its tile's base.  257 tiles
    and one record more: the second trip of the one workgroup, a last tile of one record, and entry n (the total).  The
    batch is made by hand -- 16-byte slots of random bytes, 0..128 of their bits a stream -- so the sizes come from the
    host alone.  A striped batch launches the same three kernels, and slots of 16 bytes lie where the linear ones do."""
    n, stride = 256 * 2048 + 2048 + 1, 16
    rng = np.random.default_rng(61)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    nbits = rng.integers(0, 8 * stride + 1, n).astype(np.int64)
    n_pad = (n + 63) // 64 * 64  # a striped batch holds whole waves of slots
    data = torch.zeros(n_pad * stride + 16, dtype=torch.uint8, device=dev)
    data[: n * stride] = torch.from_numpy(slots.reshape(-1)).to(dev)
    make = lambda d, layout: models.EncodedBatch(  # noqa: E731
        d, stride, torch.arange(n, dtype=torch.int64, device=dev) * (8 * stride),
        torch.from_numpy(nbits.astype(np.int32)).to(dev), torch.zeros(n, dtype=torch.int32, device=dev), n, layout)
    enc, striped = make(data[: n * stride + 16], "linear"), make(data, "striped")
    dense_bytes = (nbits + 7) // 8
    want_dense = np.concatenate([[0], np.cumsum(dense_bytes)])
    want_framed = np.concatenate([[0], np.cumsum(4 + (nbits + 3 + 7) // 8)])
    dense, offsets = models.compact(enc)
    _, framed_offsets = models.compact(enc, framed=True)
    assert np.array_equal(offsets.cpu().numpy(), want_dense), "dense offsets"
    assert np.array_equal(framed_offsets.cpu().numpy(), want_framed), "framed offsets"
    # every dense record: the slot's first ceil(nbits / 8) bytes, the bits behind the stream cleared
    expect = slots[np.arange(stride)[None, :] < dense_bytes[:, None]]
    cut = (nbits % 8 != 0)
    expect[want_dense[1:][cut] - 1] &= (0xFF00 >> (nbits[cut] % 8)).astype(np.uint8)
    assert np.array_equal(dense[: want_dense[-1]].cpu().numpy(), expect), "dense records"
    dense_s, offsets_s = models.compact(striped)
    assert torch.equal(offsets_s, offsets) and torch.equal(dense_s[: want_dense[-1]], dense[: want_dense[-1]]), "striped"


def test_status_reporting_num_bits_out_kernels(dev):
    """scl_rans_fast_b.hip: a symbol outside the alphabet is flagged (KeyError in the reference), the other chunks
    are untouched, and a corrupted stream ends in a status bit, never in a crash."""
    freq = bench_data.t256_table()[:64].copy()
    freq[0] += 4096 - freq.sum()
    model = models.RansModel(freq.tolist(), 1 << 8, 8, 32)
    assert model.info().fast_path
    rng = np.random.default_rng(3)
    sym = rng.integers(0, 64, (130, 300)).astype(np.uint8)
    sym[77, 123] = 64  # first symbol index outside the alphabet
    enc = model.encode_batch(torch.from_numpy(sym).to(dev))
    torch.cuda.synchronize()
    st = enc.status.cpu().numpy()
    assert st[77] & backend_lib.ST_SYMBOL and int(np.abs(np.delete(st, 77)).sum()) == 0
    data, offs, nbits = enc.data.cpu().numpy(), enc.bit_offset.cpu().numpy(), enc.nbits.cpu().numpy()
    for c in (0, 76, 78, 129):
        rb, rn = orc.rans_encode(sym[c], freq, RF=1 << 8, b=8)
        assert rn == nbits[c] and np.array_equal(_stream_bits(data, offs[c], nbits[c]), np.unpackbits(rb)[:rn])
    byte = int(enc.bit_offset[5].item()) // 8 + 11
    enc.data[byte] ^= 0xA5
    _, _, _, status = model.decode_batch(enc.data, enc.bit_offset, enc.nbits, 300)
    torch.cuda.synchronize()
    status = status.cpu().numpy()
    assert int(status[5]) & (backend_lib.ST_STATE | backend_lib.ST_TRUNCATED)
    assert int(np.abs(np.delete(status, [5, 77])).sum()) == 0
