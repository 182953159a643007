"""GPU: no kernel writes outside the buffers it was given (VERDICT r2 #7 -- the image has no compute-sanitizer, so the
write side of a memcheck is done by construction).  Every output buffer of a batched encode / decode is carved out of one
arena pre-filled with 0xA5, with 4 KiB guard bands in front of, between and behind the buffers; after the kernels ran --
ragged lengths, partial waves, both rANS ring writers, cooperative and per-lane stores, every tuned kernel family and the
any-parameter kernels -- every guard byte must still be 0xA5, and so must the bytes of every slot behind its stream."""
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 4096
FILL = 0xA5


class Arena:
    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)
        self.pos = GUARD
        self.used = []

    def take(self, nbytes, dtype=torch.uint8, shape=None):
        start = (self.pos + 255) // 256 * 256
        t = self.buf[start:start + nbytes]
        self.used.append((start, start + nbytes))
        self.pos = start + nbytes + GUARD
        assert self.pos + GUARD <= self.buf.numel()
        t = t.view(dtype)
        return t.view(shape) if shape is not None else t

    def check(self, what):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for a, b in self.used:
            mask[a:b] = False
        bad = ((self.buf != FILL) & mask).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} guard bytes overwritten, first at arena offset {int(bad[0])}"


def _models():
    from stanford_compression_library_amd import bench_data
    from stanford_compression_library_amd.backend import models

    t256 = bench_data.t256_table()
    small = [3, 1, 7, 2, 19]
    return {
        "rans_t256": (lambda: models.RansModel(t256.tolist(), 1 << 16, 1, 32), 256, t256),
        "rans_b8": (lambda: models.RansModel(t256.tolist(), 1 << 8, 8, 32), 256, t256),
        "rans_total32": (lambda: models.RansModel(small, 1 << 16, 1, 32), 5, np.array(small)),
        "tans": (lambda: models.TansModel(t256.tolist(), 1, 32), 256, t256),
        "range_t256": (lambda: models.RangeModel(t256.tolist(), 32, 32), 256, t256),
        "range_uniform1": (lambda: models.RangeModel([1] * 256, 32, 32), 256, np.ones(256, dtype=np.int64)),
        "aec_static": (lambda: models.AecModel(0, t256.tolist(), 256, 0, 1 << 30, 32, 32), 256, t256),
        "aec_iid256": (lambda: models.AecModel(1, [1] * 256, 256, 0, 1 << 30, 32, 32), 256, t256),
        "aec_order1_k16": (lambda: models.AecModel(2, None, 16, 1, 1 << 30, 32, 32), 16, np.ones(16, dtype=np.int64)),
        "aec_order1_k40": (lambda: models.AecModel(2, None, 40, 1, 1 << 30, 32, 32), 40, np.ones(40, dtype=np.int64)),
    }


@pytest.mark.parametrize("name", sorted(_models()))  # the same ids on every machine: conftest skips gpu tests without one
@pytest.mark.parametrize("shape", ["ragged", "full", "any_parameter"])
def test_outputs_stay_inside_their_buffers(name, shape, monkeypatch):
    from stanford_compression_library_amd.backend import lib
    from stanford_compression_library_amd.backend.models import EncodedBatch

    lib.require_device()
    dev = torch.device("cuda:0")
    make, K, freq = _models()[name]
    model = make()
    rng = np.random.default_rng(zlib.crc32(f"{name}/{shape}".encode()))  # NOT hash(): that is salted per process
    n_chunks, chunk_len = (333, 700) if shape != "full" else (512, 1024)
    p = freq / freq.sum()
    sym = torch.from_numpy(rng.choice(K, size=(n_chunks, (chunk_len + 15) // 16 * 16), p=p).astype(np.uint8)).to(dev)[:, :chunk_len]
    lens = None
    if shape != "full":
        ln = rng.integers(0, chunk_len + 1, n_chunks).astype(np.int32)
        ln[:4] = [0, 1, chunk_len, chunk_len - 1]
        if name.startswith("aec"):
            ln = np.maximum(ln, 1)  # the reference's arithmetic decoder never terminates on an empty block (quirk Q5)
        lens = torch.from_numpy(ln).to(dev)
    any_par = shape == "any_parameter"
    stride = model.slot_bytes(chunk_len)
    out_stride = (chunk_len + 15) // 16 * 16 + (8 if any_par else 0)
    arena = Arena(n_chunks * (stride + out_stride + 64) + 40 * GUARD + (1 << 20), dev)
    enc = EncodedBatch(arena.take(n_chunks * stride + 16), stride, arena.take(8 * n_chunks, torch.int64),
                       arena.take(4 * n_chunks, torch.int32), arena.take(4 * n_chunks, torch.int32), n_chunks)
    dec = (arena.take(n_chunks * out_stride, torch.uint8, (n_chunks, out_stride)), arena.take(4 * n_chunks, torch.int32),
           arena.take(4 * n_chunks, torch.int32), arena.take(4 * n_chunks, torch.int32))
    writers = ["L", "S"] if name.startswith("rans_t") or name == "rans_total32" else [""]
    for wsel in writers:
        if wsel:
            # the library reads the variable at every call (it used to cache it: ADVICE r3) -- and says which writer a
            # batch of this size would get, so the switch is known to have taken
            monkeypatch.setenv("SCL_RANS_ENC_WRITER", wsel)
            if not any_par:
                assert chr(lib.load().scl_rans_encoder_kind(model._h, n_chunks)) == wsel
        for t in (enc.data, enc.bit_offset, enc.nbits, enc.status, *dec):
            t.view(torch.uint8).fill_(FILL)
        if any_par:
            odd = torch.empty((n_chunks, out_stride), dtype=torch.uint8, device=dev)
            odd[:, :chunk_len] = sym
            L = lib.load()
            args = [model._h, odd.data_ptr(), out_stride, lens.data_ptr(), chunk_len, n_chunks, enc.data.data_ptr(), stride,
                    enc.bit_offset.data_ptr(), enc.nbits.data_ptr(), enc.status.data_ptr()]
            scratch = None
            if model._needs_scratch:
                scratch, nb = model._scratch(n_chunks, dev)
                args += [scratch.data_ptr() if scratch is not None else None, nb]
            lib.check(getattr(L, f"scl_{model._prefix}_encode_batch")(*args, torch.cuda.current_stream(dev).cuda_stream), "encode")
        else:
            model.encode_batch(sym, lens=lens, out=enc)
        torch.cuda.synchronize()
        arena.check(f"{name} encode {shape} {wsel}")
        assert int(enc.status.abs().sum()) == 0
        # inside a slot nothing but the stream (and, for the back-to-front coders, the zero padding in front of it) is written
        data = enc.data[:n_chunks * stride].view(n_chunks, stride).cpu().numpy()
        nbits, offs = enc.nbits.cpu().numpy(), enc.bit_offset.cpu().numpy()
        back = model._prefix in ("rans", "tans")
        for c in range(0, n_chunks, 37):
            nbytes = (int(nbits[c]) + 7) // 8
            if back:
                front = stride - nbytes
                assert int(offs[c]) == 8 * (c + 1) * stride - int(nbits[c])
                untouched = data[c, :max(front - 16, 0)]  # the line that holds the first stream byte may be zero-filled
            else:
                assert int(offs[c]) == 8 * c * stride
                untouched = data[c, min((nbytes + 127) // 128 * 128, stride):]  # whole lines are written
            assert (np.isin(untouched, (FILL, 0))).all(), f"{name} chunk {c}: bytes outside the stream were written"
        L = lib.load()
        sym_out, lens_out, used, status = dec
        dargs = [model._h, enc.data.data_ptr(), enc.data.numel(), enc.bit_offset.data_ptr(), enc.nbits.data_ptr(), n_chunks,
                 sym_out.data_ptr(), out_stride, chunk_len, lens_out.data_ptr(), used.data_ptr(), status.data_ptr()]
        if model._needs_scratch:
            scratch, nb = model._scratch(n_chunks, dev)
            dargs += [scratch.data_ptr() if scratch is not None else None, nb]
        lib.check(getattr(L, f"scl_{model._prefix}_decode_batch")(*dargs, torch.cuda.current_stream(dev).cuda_stream), "decode")
        torch.cuda.synchronize()
        arena.check(f"{name} decode {shape} {wsel}")
        assert int(status.abs().sum()) == 0
        ref_lens = lens if lens is not None else torch.full((n_chunks,), chunk_len, dtype=torch.int32, device=dev)
        assert torch.equal(lens_out, ref_lens)
        # num_bits_consumed equals the stream length -- except, for the arithmetic coder, on rare blocks of one or two
        # symbols, where the reference's own rule (arithmetic_coding.py:277-285) stops short (tests/test_gpu_stream_goldens.py)
        settled = torch.ones_like(ref_lens, dtype=torch.bool) if not name.startswith("aec") else ref_lens > 2
        assert torch.equal(used[settled], enc.nbits[settled])
        got, want = sym_out.cpu().numpy(), sym.cpu().numpy()
        ln_h = ref_lens.cpu().numpy()
        for c in range(n_chunks):
            assert np.array_equal(got[c, :ln_h[c]], want[c, :ln_h[c]]), (name, c)
