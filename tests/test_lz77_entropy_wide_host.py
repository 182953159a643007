"""The wide entropy stage of LZ77 without a GPU: the entry points check their arguments before any device call, the scratch
size is monotone, and the hand-made fixtures of tests/lz77_entropy_wide_helpers.py are what the GPU tests take them for."""
import ctypes as C

import numpy as np
import pytest

from lz77_entropy_helpers import header_positions
from lz77_entropy_wide_helpers import (GROUP_BITS, NEVER_SYMBOLS, damaged_inputs, elias_delta_bits, grid_cases, never_counts,
                                       never_in_step_stream)
from lz77_helpers import use_host_prefix_coder
from stanford_compression_library_amd.backend import lib as backend_lib
from stanford_compression_library_amd.backend import lz77 as dev_lz77
from stanford_compression_library_amd.compressors.lz77 import LZ77StreamsDecoder
from stanford_compression_library_amd.utils.bitarray_utils import BitArray

FAKE = 0x10000  # an aligned address that is never dereferenced: every check below fails before a device call


def enc_args(**kw):
    a = dict(d_lit_count=FAKE, d_match_len=FAKE, d_match_off=FAKE, n_seq=10, d_literals=FAKE, n_lit=10, binned_offset=16,
             reserved=0, d_out=FAKE, out_cap_bytes=4096, d_nbits=FAKE, d_status=FAKE, d_scratch=FAKE, scratch_bytes=1 << 20)
    a.update(kw)
    return backend_lib.Lz77EntropyWideEncodeArgs(**a)


def dec_args(**kw):
    a = dict(d_in=FAKE, in_size_bytes=4096, in_bit_offset=3, in_nbits=1000, binned_offset=16, reserved=0, seq_cap=10, lit_cap=10,
             d_lit_count=FAKE, d_match_len=FAKE, d_match_off=FAKE, d_literals=FAKE, d_result=FAKE, d_scratch=FAKE,
             scratch_bytes=1 << 20)
    a.update(kw)
    return backend_lib.Lz77EntropyWideDecodeArgs(**a)


def refused(name, args):
    L = backend_lib.load()
    rc = getattr(L, name)(None if args is None else C.byref(args), None)
    assert rc == backend_lib.E_PARAM, name
    message = backend_lib.last_error()
    assert message.startswith(name[len("scl_"):] + ":"), message
    return message


def test_null_arguments_are_refused_before_any_device_call():
    for name, make in (("scl_lz77_entropy_encode_wide", enc_args), ("scl_lz77_entropy_decode_wide", dec_args)):
        assert "null pointer" in refused(name, None)
        fields = [f for f, t in make()._fields_ if t is C.c_void_p]
        assert len(fields) >= 7
        for field in fields:
            assert "null pointer" in refused(name, make(**{field: None})), field


def test_the_other_parameter_checks():
    enc, dec = "scl_lz77_entropy_encode_wide", "scl_lz77_entropy_decode_wide"
    assert "binned_offset" in refused(enc, enc_args(binned_offset=33))
    assert "binned_offset" in refused(dec, dec_args(binned_offset=33))
    assert "2^32" in refused(enc, enc_args(n_seq=1 << 32)) and "2^32" in refused(enc, enc_args(n_lit=1 << 32))
    assert "2^32" in refused(dec, dec_args(seq_cap=1 << 32)) and "2^32" in refused(dec, dec_args(lit_cap=1 << 32))
    assert "aligned" in refused(enc, enc_args(d_out=FAKE + 2)) and "aligned" in refused(enc, enc_args(d_scratch=FAKE + 4))
    assert "aligned" in refused(enc, enc_args(d_match_len=FAKE + 1)) and "aligned" in refused(enc, enc_args(d_nbits=FAKE + 4))
    assert "aligned" in refused(dec, dec_args(d_in=FAKE + 1)) and "aligned" in refused(dec, dec_args(d_result=FAKE + 4))
    assert "scratch" in refused(enc, enc_args(scratch_bytes=dev_lz77.entropy_wide_scratch_bytes(10, 10) - 1))
    assert "scratch" in refused(dec, dec_args(scratch_bytes=dev_lz77.entropy_wide_scratch_bytes(10, 10, 1000) - 1))
    assert "in_size_bytes" in refused(dec, dec_args(in_size_bytes=125))  # 3 + 1000 bits end in byte 126
    assert "2^46" in refused(dec, dec_args(in_nbits=1 << 46, in_size_bytes=1 << 60))
    assert backend_lib.load().scl_lz77_entropy_wide_kernel_names(None, None, None, 8) == backend_lib.E_PARAM


def test_scratch_bytes_is_monotone_and_the_names_are_kernels():
    sizes = (0, 1, 4095, 4096, 4097, 1 << 20, 1 << 24, (1 << 32) - 1)
    f = dev_lz77.entropy_wide_scratch_bytes
    for fixed in ((0, 0), (4097, 1 << 20)):
        for axis in range(3):
            at = lambda v: f(*[v if i == axis else fixed[i - (i > axis)] for i in range(3)])  # noqa: E731
            values = [at(v) for v in sizes]
            assert values == sorted(values) and values[0] > 0 and values[-1] > values[0], (fixed, axis)
    assert f(10, 10, 0) % 256 == 0
    assert dev_lz77.entropy_wide_kernel_names() == ("lzw_emit_kernel", "lzw_sync_kernel", "lzw_resid_kernel")
    assert dev_lz77.entropy_wide_threshold() >= 1


def test_the_never_in_step_fixture_is_that_tree_and_a_block_the_classes_decode(monkeypatch):
    codes, lengths = dev_lz77.huffman_from_counts(never_counts())
    words = sorted(format(int(codes[s]), f"0{int(lengths[s])}b") for s in NEVER_SYMBOLS)
    assert words == sorted(["0", "11", "101", "100"])
    assert int(lengths.astype(np.int64).sum()) == 9  # no other symbol has a codeword
    bits, literals = never_in_step_stream(codes, lengths, pairs=40)
    assert "".join(map(str, bits[-120:].tolist())) == "011" * 40
    use_host_prefix_coder(monkeypatch)
    (seqs, lits), used = LZ77StreamsDecoder(16).decode_block(BitArray._wrap(bits.copy()))
    assert used == len(bits) and seqs == [] and list(lits) == literals.tolist()
    # the full fixture: five decoder workgroups, and the second one starts at a bit = 2 mod 3, inside "101" for ever
    full, _ = never_in_step_stream(codes, lengths)
    values_at = len(full) - 150000
    assert -(-150000 // GROUP_BITS) == 5 and GROUP_BITS % 3 == 2
    assert "".join(map(str, full[values_at + GROUP_BITS: values_at + GROUP_BITS + 3].tolist())) == "101"
    assert elias_delta_bits(0) == [1] and elias_delta_bits(1) == [0, 1, 0, 0] and elias_delta_bits(3) == [0, 1, 1, 0, 0]


def test_the_grid_covers_what_it_claims():
    cases = grid_cases()
    assert len({name for name, _, _ in cases}) == len(cases)
    assert {len(s[0]) for _, s, _ in cases} >= {0, 1, 2, 4095, 4096, 4097, 8193}
    assert {len(s[1]) for _, s, _ in cases} >= {0, 1, 4095, 4096, 4097, 40000, 5000, 4000}
    assert {o for _, _, o in cases} == {0, 16, 32}
    by_name = {name: s for name, s, _ in cases}
    assert (by_name["widths-0"][0] < 16).all() and (by_name["widths-31"][0] >= 16 + (1 << 31) - 1).all()
    assert by_name["widths-31"][0].max() < 1 << 32
    assert all(len(np.unique(by_name["one-symbol-4097"][0][:, f])) == 1 for f in range(3))


def test_damaged_inputs_cut_every_header_and_section(monkeypatch):
    from lz77_entropy_helpers import host_encode
    from lz77_entropy_wide_helpers import edge_stream

    use_host_prefix_coder(monkeypatch)
    stream = edge_stream(40, 90, 16, 5, lit_hi=256)
    bits = host_encode(stream)
    heads = header_positions(stream, bits)
    cases = damaged_inputs(stream, bits)
    cuts = {fed for name, _, fed in cases if name.startswith("cut")}
    assert all({h, h + 31, h + 32} <= cuts for h in heads) and len(bits) - 1 in cuts
    assert sum(name.startswith("head") for name, _, _ in cases) == 40
    assert sum(name.startswith("flip") for name, _, _ in cases) == 48
