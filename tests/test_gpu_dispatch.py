"""GPU test of the kernel dispatch of the rANS, tANS, range and prefix coders (csrc/scl_entry.h: the walk over a coder's
table of tuned kernel families; the arithmetic coder's table has tests/test_gpu_aec_dispatch.py, whose shape and helpers
this file reuses).  One model per row of the family tables -- rANS on rans_fast, on rans_fastb and on neither, tANS on the
table-free rANS kernels and (SCL_TANS_KERNELS=table) on its table kernels, the range coder tuned and any-parameter, a
prefix code on its tuned kernels -- each on four layouts:
  (a) rows the tuned kernels take as they are,
  (b) symbol rows and output rows at an odd address with stride 211 (re-laid through the row relay),
  (c) an input moved by four bytes, which the tuned readers decline,
  (d) any_parameter_kernels=True.
Every layout gives the same streams, symbols, lengths and consumed counts and zero statuses; the first eight chunks equal
the CPU oracle; nothing is written outside the decoded symbols.

The second half pins what the reporting calls answer (kernel names, scl_rans_encoder_kind, fast_path) in a literal table
recorded from the library BEFORE the dispatch was table-driven: names and dispatch read the same family tables, and the
answers must not move."""
import numpy as np
import pytest

import scl_oracle as orc
import test_gpu_aec_dispatch as aec_dispatch
from prefix_helpers import code_bits, decode_reference, encode_numpy, table_case
from stanford_compression_library_amd import bench_data
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_CHUNKS, CHUNK_LEN, ODD_STRIDE, FILL, N_ORACLE = (aec_dispatch.N_CHUNKS, aec_dispatch.CHUNK_LEN, aec_dispatch.ODD_STRIDE,
                                                   aec_dispatch.FILL, aec_dispatch.N_ORACLE)
T256 = bench_data.t256_table()


class Case:
    """a model, the environment it runs under, the CPU oracle of its stream and what the library must report for it"""

    def __init__(self, make, oracle_encode, oracle_decode, env=None, kind=None, encoder=None, fast_path=None):
        self.make, self.oracle_encode, self.oracle_decode = make, oracle_encode, oracle_decode
        self.env = env or {}
        self.kind = kind            # scl_rans_encoder_kind for N_CHUNKS chunks (rANS models)
        self.encoder = encoder      # what the encode kernel's name starts with (coders that name their kernels)
        self.fast_path = fast_path  # RangeModel.fast_path()


def _rans(RF, b):
    kw = dict(RF=RF, b=b, size_bits=32)
    return dict(make=lambda: models.RansModel(T256.tolist(), RF, b, 32),
                oracle_encode=lambda s: orc.rans_encode(s, T256, **kw),
                oracle_decode=lambda p, n: orc.rans_decode(p, n, T256, cap=CHUNK_LEN, **kw))


def _tans():
    return dict(make=lambda: models.TansModel(T256.tolist(), 1, 32),
                oracle_encode=lambda s: orc.tans_encode(s, T256, RF=1, size_bits=32),
                oracle_decode=lambda p, n: orc.tans_decode(p, n, T256, RF=1, size_bits=32, cap=CHUNK_LEN))


def _range(precision):
    return dict(make=lambda: models.RangeModel(T256.tolist(), precision, 32),
                oracle_encode=lambda s: orc.range_encode(s, T256, precision=precision, size_bits=32),
                oracle_decode=lambda p, n: orc.range_decode(p, n, T256, precision=precision, size_bits=32, cap=CHUNK_LEN))


def _prefix():
    case = table_case("random256")
    code, length, bits_of = case.arr("code"), case.arr("len"), code_bits(case)

    def decode(packed, nbits):
        sym, used, status = decode_reference(code, length, packed, 0, nbits, CHUNK_LEN)
        assert status == 0
        return sym, used

    return dict(make=lambda: models.PrefixModel(code, length), oracle_encode=lambda s: encode_numpy(bits_of, s),
                oracle_decode=decode)


CASES = {
    "rans_fast": Case(**_rans(1 << 16, 1), kind="L", encoder="rans_encode_fast_kernel<"),
    "rans_fastb": Case(**_rans(1 << 8, 2), kind="B", encoder="rans_encode_fastb_kernel"),
    "rans_generic": Case(**_rans(3, 1), kind="G", encoder="rans_encode_generic"),
    "tans_on_rans": Case(**_tans(), encoder="rans_encode_fast_kernel<"),
    "tans_table": Case(**_tans(), env={"SCL_TANS_KERNELS": "table"}, encoder="tans_encode_fast_kernel"),
    "range_fast": Case(**_range(32), fast_path=True),
    "range_generic": Case(**_range(40), fast_path=False),
    "prefix_fast": Case(**_prefix(), encoder="prefix_encode_fast_kernel"),
}


@pytest.fixture(scope="module")
def dev():
    backend_lib.require_device()
    return torch.device("cuda:0")


def _encoded(model, d_sym, d_lens, **kw):
    """aec_dispatch._encoded, with the bit offsets as well: -> (batch, offsets, nbits, [bits of stream c])"""
    enc, nbits, bits = aec_dispatch._encoded(model, d_sym, d_lens, **kw)
    return enc, enc.bit_offset.cpu().numpy(), nbits, bits


@pytest.mark.parametrize("name", list(CASES))
def test_family_on_aligned_odd_declined_and_any_parameter_rows(name, dev, monkeypatch):
    case = CASES[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)  # the library reads its switches at every call
    model = case.make()
    L = backend_lib.load()
    if case.kind is not None:
        assert chr(L.scl_rans_encoder_kind(model._h, N_CHUNKS)) == case.kind
    if case.encoder is not None:
        assert model.kernel_names(N_CHUNKS)[0].startswith(case.encoder), model.kernel_names(N_CHUNKS)
    if case.fast_path is not None:
        assert model.fast_path() == case.fast_path
    lens = aec_dispatch._lens()
    sym = bench_data.iid_chunks_host(T256, N_CHUNKS, CHUNK_LEN, seed=41)
    d_lens = torch.from_numpy(lens).to(dev)

    # encode: (a) aligned rows, (b) the same symbols at base + 1 with stride 211, (d) the any-parameter kernels on (a)
    sym_a = torch.from_numpy(sym).to(dev)
    assert sym_a.data_ptr() % 16 == 0 and sym_a.stride(0) % 16 == 0
    _, rows_b = aec_dispatch._odd_rows(dev)
    rows_b[:, :CHUNK_LEN] = sym_a
    sym_b = rows_b[:, :CHUNK_LEN]
    assert sym_b.data_ptr() % 2 == 1 and sym_b.stride(0) == ODD_STRIDE
    enc_a, offs_a, nbits_a, bits_a = _encoded(model, sym_a, d_lens)
    for what, (_, offs, nbits, bits) in (("odd rows", _encoded(model, sym_b, d_lens)),
                                         ("any-parameter kernels", _encoded(model, sym_a, d_lens, any_parameter_kernels=True))):
        assert np.array_equal(nbits_a, nbits) and np.array_equal(offs_a, offs), what
        for c in range(N_CHUNKS):
            assert np.array_equal(bits_a[c], bits[c]), f"chunk {c}: {what} give another stream"

    # the oracle on the first eight chunks (lengths 0, 1, 207, 208 among them)
    ref_used = {}
    for c in range(N_ORACLE):
        rb, rn = case.oracle_encode(sym[c, :lens[c]])
        assert int(nbits_a[c]) == rn, f"chunk {c}: {nbits_a[c]} bits vs oracle {rn}"
        assert np.array_equal(bits_a[c], np.unpackbits(np.asarray(rb, np.uint8))[:rn]), f"chunk {c}: stream differs from the oracle's"
        o_sym, ref_used[c] = case.oracle_decode(rb, rn)
        assert np.array_equal(np.asarray(o_sym)[:lens[c]], sym[c, :lens[c]]) and len(o_sym) == lens[c]

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

    # decode the (a) streams into (a) aligned rows
    check(*model.decode_batch(enc_a.data, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN), "aligned rows")
    # (b) rows at an odd base and an odd stride inside a buffer of sentinels
    buf, rows = aec_dispatch._odd_rows(dev)
    outs = tuple(torch.zeros(N_CHUNKS, dtype=torch.int32, device=dev) for _ in range(3))
    check(*model.decode_batch(enc_a.data, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN, out=(rows,) + outs), "odd rows")
    got = rows.cpu().numpy()
    for c in range(N_CHUNKS):
        assert (got[c, lens[c]:] == FILL).all(), f"chunk {c}: bytes behind the decoded symbols were written"
    assert (buf[:1].cpu().numpy() == FILL).all() and (buf[1 + N_CHUNKS * ODD_STRIDE:].cpu().numpy() == FILL).all()
    # (c) aligned rows from an input that is 4-byte but not 16-byte aligned: the tuned readers decline it (the streams
    # are copied to base + 4 and keep their bit offsets, as in the arithmetic coder's test)
    moved = torch.zeros(enc_a.data.numel() + 16, dtype=torch.uint8, device=dev)[4:4 + enc_a.data.numel()]
    moved.copy_(enc_a.data)
    assert moved.data_ptr() % 16 == 4
    check(*model.decode_batch(moved, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN), "input at base + 4")
    # (d) the any-parameter kernels, into rows pre-filled with sentinels
    rows_d = torch.full((N_CHUNKS, CHUNK_LEN), FILL, dtype=torch.uint8, device=dev)
    outs = tuple(torch.zeros(N_CHUNKS, dtype=torch.int32, device=dev) for _ in range(3))
    check(*model.decode_batch(enc_a.data, enc_a.bit_offset, enc_a.nbits, CHUNK_LEN, out=(rows_d,) + outs,
                              any_parameter_kernels=True), "any-parameter kernels")
    got = rows_d.cpu().numpy()
    for c in range(N_CHUNKS):
        assert (got[c, lens[c]:] == FILL).all(), f"chunk {c}: the any-parameter kernels wrote behind the decoded symbols"


# ---- what the reporting calls answer ------------------------------------------------------------------------------------
REPORT_CHUNKS = (1000, 65536, 131072, 196608, 262144)
REPORT_ENVS = {"default": {}, "tans_table": {"SCL_TANS_KERNELS": "table"}, "writer_L": {"SCL_RANS_ENC_WRITER": "L"},
               "writer_S": {"SCL_RANS_ENC_WRITER": "S"}}
REPORT_MODELS = dict({n: c.make for n, c in CASES.items() if n != "tans_table"},
                     aec_static=aec_dispatch.CASES["static_fixed_t256"][0])


def report(model_name, model, any_parameter):
    """what the library reports for one model under the current environment and thread switch: the fast_path answer and,
    per batch size of REPORT_CHUNKS, (encode kernel, decode kernel) and (rANS) the encoder kind.  No launches."""
    L = backend_lib.load()
    coder = model._prefix
    with models._any_parameter(any_parameter):
        if coder == "range":
            return {"fast_path": int(model.fast_path())}
        if coder == "aec":
            return {"fast_path": int(model.fast_path(CHUNK_LEN))}
        out = {"fast_path": int(model.info().fast_path), "kernels": [model.kernel_names(n) for n in REPORT_CHUNKS]}
        if coder == "rans":
            out["kind"] = "".join(chr(L.scl_rans_encoder_kind(model._h, n)) for n in REPORT_CHUNKS)
        return out


# Recorded from a run of the library as it was before the dispatch became table-driven (every coder's walk written out by
# hand), on an MI355X (256 CUs: the writer choice of scl_rans_encoder_kind counts workgroups per CU).
# model -> {environment of REPORT_ENVS ("default" where it is not listed: the switch does not reach that model) ->
# (report() while the thread lets the tuned kernels run, report() while it keeps them out)}
def _rans_fast_names(writers, enc_consts, dec_consts):
    """the tuned rANS kernels' names per batch size of REPORT_CHUNKS: the encoder's writer is one letter of `writers`, the
    decoder runs 256 lanes per workgroup up to 131 072 chunks and 1024 beyond"""
    return [(f"rans_encode_fast_kernel<AnsBackWriter{w}<256>, {enc_consts}>", f"rans_decode_fast_kernel<{dec_consts}, {t}, 1, false>")
            for w, t in zip(writers, (256, 256, 256, 1024, 1024))]


_RANS_ANY = dict(kernels=("rans_encode_generic", "rans_decode_generic"), kind="GGGGG")
_TANS_ANY = dict(fast_path=1, kernels=("tans_encode_kernel", "tans_decode_kernel"))
_PREFIX = (dict(fast_path=1, kernels=("prefix_encode_fast_kernel", "prefix_decode_fast_kernel")),
           dict(fast_path=1, kernels=("prefix_encode_kernel", "prefix_decode_kernel")))


def _rans_fast(writers):
    return (dict(fast_path=1, kernels=_rans_fast_names(writers, "0, 10, 16, 1", "12, 3"), kind=writers), dict(fast_path=1, **_RANS_ANY))


def _tans_on_rans(writers):
    return (dict(fast_path=1, kernels=_rans_fast_names(writers, "0, -1, 0, 1", "0, 3")), _TANS_ANY)


EXPECTED_REPORT = {
    "rans_fast": {"default": _rans_fast("LLLSL"), "writer_L": _rans_fast("LLLLL"), "writer_S": _rans_fast("SSSSS")},
    "rans_fastb": {"default": (dict(fast_path=1, kernels=("rans_encode_fastb_kernel", "rans_decode_fastb_kernel"), kind="BBBBB"),
                               dict(fast_path=1, **_RANS_ANY))},
    "rans_generic": {"default": (dict(fast_path=0, **_RANS_ANY), dict(fast_path=0, **_RANS_ANY))},
    "tans_on_rans": {"default": _tans_on_rans("LLLSL"), "writer_L": _tans_on_rans("LLLLL"), "writer_S": _tans_on_rans("SSSSS"),
                     "tans_table": (dict(fast_path=1, kernels=("tans_encode_fast_kernel", "tans_decode_fast_kernel")), _TANS_ANY)},
    "range_fast": {"default": (dict(fast_path=1), dict(fast_path=1))},
    "range_generic": {"default": (dict(fast_path=0), dict(fast_path=0))},
    "prefix_fast": {"default": _PREFIX},
    "aec_static": {"default": (dict(fast_path=1), dict(fast_path=1))},
}


def _expected(name, env_name, any_parameter):
    by_env = EXPECTED_REPORT[name]
    entry = dict(by_env.get(env_name, by_env["default"])[int(any_parameter)])
    if "kernels" in entry and isinstance(entry["kernels"], tuple):  # one pair: the same at every batch size
        entry["kernels"] = [entry["kernels"]] * len(REPORT_CHUNKS)
    return entry


def test_reporting_calls_answer_as_before(dev, monkeypatch):
    made = {name: make() for name, make in REPORT_MODELS.items()}
    assert set(made) == set(EXPECTED_REPORT)
    for env_name, env in REPORT_ENVS.items():
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for name, model in made.items():
                for any_parameter in (False, True):
                    assert report(name, model, any_parameter) == _expected(name, env_name, any_parameter), \
                        (name, env_name, any_parameter)
