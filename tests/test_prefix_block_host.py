"""One large prefix-code block coded by the whole grid (csrc/scl_prefix_block.hip), host side (no GPU): the entry points
exist with the signatures include/scl_hip.h declares, and each refuses a null model by name before it touches a device."""
import ctypes
import os
import re

import pytest

from stanford_compression_library_amd.backend import lib as backend_lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scl_hip.h")
BLOCK_ENTRY_POINTS = [f"scl_prefix_{op}_block{host}{form}" for host in ("", "_host") for form in ("", "_u16")
                      for op in ("encode", "decode")]
# parameters of the declarations, pointers as "p" and integers by their width
DECLARED = {
    "scl_prefix_block_info_get": "pp",
    "scl_prefix_block_scratch_bytes": "p88",
    "scl_prefix_encode_block": "pp8p8ppp8p",
    "scl_prefix_decode_block": "pp888p8pp8p",
    "scl_prefix_encode_block_host": "pp8p8p",
    "scl_prefix_decode_block_host": "pp8p8pp",
}


def kinds_of(argtypes):
    out = ""
    for t in argtypes:
        out += "8" if t is ctypes.c_uint64 else "4" if t is ctypes.c_uint32 else "p"
    return out


def declared_in_header(name):
    text = open(HEADER).read()
    m = re.search(r"\b(?:int|uint64_t)\s+" + name + r"\(([^;]*)\);", text)
    assert m, f"{name} is not declared in include/scl_hip.h"
    out = ""
    for param in m.group(1).split(","):
        out += "p" if "*" in param else "8" if "uint64_t" in param else "4"
    return out


@pytest.mark.parametrize("name", sorted(DECLARED) + [n + "_u16" for n in DECLARED if n.endswith(("_block", "_host"))])
def test_block_entry_points_exist_with_the_declared_signatures(name):
    L = backend_lib.load()
    fn = getattr(L, name)
    want = DECLARED[name[:-4] if name.endswith("_u16") else name]
    assert kinds_of(fn.argtypes) == want
    assert declared_in_header(name) == want
    assert fn.restype is (ctypes.c_uint64 if name.endswith("scratch_bytes") else ctypes.c_int)


def test_block_structs_have_the_declared_layout():
    assert [f[0] for f in backend_lib.PrefixBlockInfo._fields_] == ["sub_bits", "tile_symbols", "code_len_gcd"]
    assert ctypes.sizeof(backend_lib.PrefixBlockInfo) == 12
    assert [f[0] for f in backend_lib.PrefixBlockResult._fields_] == ["n_out", "consumed", "status", "sync_passes"]
    assert ctypes.sizeof(backend_lib.PrefixBlockResult) == 24
    assert backend_lib.load().scl_abi_version() == 8  # the block calls joined ABI 8 without a new number


@pytest.mark.parametrize("name", BLOCK_ENTRY_POINTS + ["scl_prefix_block_info_get"])
def test_block_entry_points_refuse_a_null_model(name):
    L = backend_lib.load()
    fn = getattr(L, name)
    assert fn(*[None if t is ctypes.c_void_p or hasattr(t, "contents") else 0 for t in fn.argtypes]) == backend_lib.E_PARAM
    assert backend_lib.last_error().startswith(name[len("scl_"):] + ":"), backend_lib.last_error()


def test_block_scratch_bytes_without_a_model():
    assert backend_lib.load().scl_prefix_block_scratch_bytes(None, 1 << 20, 1 << 23) == 0


def test_the_threshold_is_a_class_attribute():
    from stanford_compression_library_amd.backend.models import PrefixModel

    v = PrefixModel.BLOCK_PARALLEL_MIN
    assert isinstance(v, int) and v >= 1 << 12 and v & (v - 1) == 0  # a power of two; 4 Ki is where the sweep starts
