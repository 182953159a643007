"""ctypes binding of ``libscl_hip.so`` (the C ABI declared in include/scl_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing, cannot be loaded or reports
no device, the product path raises.  (The CPU oracle lives in oracle/ and is test infrastructure.)
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_DIR, "libscl_hip.so")

OK = 0
E_PARAM, E_ALLOC, E_HIP, E_NODEVICE, E_CHUNK = -2, -7, -8, -9, -10
ST_CAPACITY, ST_SYMBOL, ST_TRUNCATED, ST_STATE, ST_TOTAL, ST_SIZE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
MODEL_FIXED, MODEL_IID, MODEL_ORDERK = 0, 1, 2
COMPACT_DENSE, COMPACT_FRAMED = 0, 1
UINT_GOLOMB, UINT_UNIVERSAL, UINT_ELIAS_DELTA = 0, 1, 2
FIXED_TILE = 8192  # SCL_FIXED_TILE: symbols a workgroup of the fixed-width kernels codes


class SclHipError(RuntimeError):
    """A call into libscl_hip.so failed (carries the status code and the library's message)."""

    def __init__(self, code: int, what: str, message: str):
        super().__init__(f"{what}: status {code}: {message}")
        self.code = code
        self.message = message


class RansInfo(C.Structure):
    _fields_ = [("M", C.c_uint64), ("L", C.c_uint64), ("H", C.c_uint64), ("K", C.c_uint32),
                ("num_state_bits", C.c_uint32), ("size_bits", C.c_uint32), ("num_bits_out", C.c_uint32),
                ("max_bits_per_symbol", C.c_uint32), ("fast_path", C.c_uint32), ("device", C.c_int32)]


class PrefixInfo(C.Structure):
    _fields_ = [("K", C.c_uint32), ("min_len", C.c_uint32), ("max_len", C.c_uint32), ("lut_bits", C.c_uint32),
                ("fast_path", C.c_uint32), ("device", C.c_int32)]


class PrefixBlockInfo(C.Structure):
    _fields_ = [("sub_bits", C.c_uint32), ("tile_symbols", C.c_uint32), ("code_len_gcd", C.c_uint32)]


class PrefixBlockResult(C.Structure):
    _fields_ = [("n_out", C.c_uint64), ("consumed", C.c_uint64), ("status", C.c_uint32), ("sync_passes", C.c_uint32)]


class UintCodeStruct(C.Structure):
    """scl_uint_code"""
    _fields_ = [("kind", C.c_uint32), ("M", C.c_uint32)]


class TypicalInfo(C.Structure):
    """scl_typical_info"""
    _fields_ = [("N", C.c_uint32), ("count", C.c_uint32), ("bt", C.c_uint32), ("bo", C.c_uint32), ("K", C.c_uint32),
                ("n", C.c_uint32), ("device", C.c_int32), ("reserved", C.c_uint32)]


TYPICAL_NONE = 0xFFFFFFFF        # SCL_TYPICAL_NONE: no rank (an atypical tuple), no width (an empty typical set)
TYPICAL_MAX_TUPLES = 1 << 24     # SCL_TYPICAL_MAX_TUPLES


class Lz77ParseArgs(C.Structure):
    """scl_lz77_parse_args: device pointers travel as integers"""
    _fields_ = [("d_win", C.c_void_p), ("d_win_off", C.c_void_p), ("d_start", C.c_void_p), ("n_streams", C.c_uint64),
                ("total_bytes", C.c_uint64), ("min_match_length", C.c_uint32), ("max_matches", C.c_uint32),
                ("seq_cap", C.c_uint32), ("phases", C.c_uint32), ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p),
                ("d_match_off", C.c_void_p), ("d_literals", C.c_void_p), ("d_n_seq", C.c_void_p), ("d_n_lit", C.c_void_p),
                ("d_status", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77ReplayArgs(C.Structure):
    """scl_lz77_replay_args"""
    _fields_ = [("d_win", C.c_void_p), ("d_win_off", C.c_void_p), ("d_have", C.c_void_p), ("n_streams", C.c_uint64),
                ("total_bytes", C.c_uint64), ("seq_cap", C.c_uint32), ("reserved", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_n_seq", C.c_void_p), ("d_literals", C.c_void_p), ("lit_bytes", C.c_uint64), ("d_lit_off", C.c_void_p),
                ("d_n_lit", C.c_void_p), ("d_out_len", C.c_void_p), ("d_status", C.c_void_p)]


class Lz77SlidingParseArgs(C.Structure):
    """scl_lz77_sliding_parse_args"""
    _fields_ = [("d_win", C.c_void_p), ("d_win_off", C.c_void_p), ("d_start", C.c_void_p), ("n_streams", C.c_uint64),
                ("total_bytes", C.c_uint64), ("hash_table_size", C.c_uint64), ("hash_length", C.c_uint32),
                ("max_chain_length", C.c_uint32), ("lazy", C.c_uint32), ("min_match_length", C.c_uint32),
                ("window_size", C.c_uint32), ("seq_cap", C.c_uint32), ("phases", C.c_uint32), ("reserved", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_literals", C.c_void_p), ("d_n_seq", C.c_void_p), ("d_n_lit", C.c_void_p), ("d_status", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77SlidingReplayArgs(C.Structure):
    """scl_lz77_sliding_replay_args"""
    _fields_ = [("d_win", C.c_void_p), ("d_win_off", C.c_void_p), ("d_have", C.c_void_p), ("n_streams", C.c_uint64),
                ("total_bytes", C.c_uint64), ("seq_cap", C.c_uint32), ("window_size", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_n_seq", C.c_void_p), ("d_literals", C.c_void_p), ("lit_bytes", C.c_uint64), ("d_lit_off", C.c_void_p),
                ("d_n_lit", C.c_void_p), ("d_out_len", C.c_void_p), ("d_status", C.c_void_p)]


class Lz77WideParseArgs(C.Structure):
    """scl_lz77_wide_parse_args"""
    _fields_ = [("d_win", C.c_void_p), ("n", C.c_uint64), ("start", C.c_uint64), ("min_match_length", C.c_uint32),
                ("max_matches", C.c_uint32), ("seq_cap", C.c_uint32), ("phases", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_literals", C.c_void_p), ("d_n_seq", C.c_void_p), ("d_n_lit", C.c_void_p), ("d_status", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77WideReplayArgs(C.Structure):
    """scl_lz77_wide_replay_args"""
    _fields_ = [("d_win", C.c_void_p), ("have", C.c_uint64), ("cap", C.c_uint64), ("d_lit_count", C.c_void_p),
                ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p), ("n_seq", C.c_uint64),
                ("d_literals", C.c_void_p), ("n_lit", C.c_uint64), ("d_out_len", C.c_void_p), ("d_status", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77SlidingWideParseArgs(C.Structure):
    """scl_lz77_sliding_wide_parse_args"""
    _fields_ = [("d_win", C.c_void_p), ("n", C.c_uint64), ("start", C.c_uint64), ("hash_table_size", C.c_uint64),
                ("hash_length", C.c_uint32), ("max_chain_length", C.c_uint32), ("lazy", C.c_uint32),
                ("min_match_length", C.c_uint32), ("window_size", C.c_uint32), ("seq_cap", C.c_uint32),
                ("phases", C.c_uint32), ("reserved", C.c_uint32), ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p),
                ("d_match_off", C.c_void_p), ("d_literals", C.c_void_p), ("d_n_seq", C.c_void_p), ("d_n_lit", C.c_void_p),
                ("d_status", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77SlidingWideReplayArgs(C.Structure):
    """scl_lz77_sliding_wide_replay_args"""
    _fields_ = Lz77WideReplayArgs._fields_ + [("window_size", C.c_uint32), ("reserved", C.c_uint32)]


class Lz77EntropyEncodeArgs(C.Structure):
    """scl_lz77_entropy_encode_args"""
    _fields_ = [("n_streams", C.c_uint64), ("seq_cap", C.c_uint32), ("binned_offset", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_n_seq", C.c_void_p), ("d_literals", C.c_void_p), ("lit_bytes", C.c_uint64), ("d_lit_off", C.c_void_p),
                ("d_n_lit", C.c_void_p), ("d_out", C.c_void_p), ("out_stride", C.c_uint64), ("d_bit_off", C.c_void_p),
                ("d_nbits", C.c_void_p), ("d_status", C.c_void_p)]


class Lz77EntropyDecodeArgs(C.Structure):
    """scl_lz77_entropy_decode_args"""
    _fields_ = [("d_in", C.c_void_p), ("in_size_bytes", C.c_uint64), ("d_bit_off", C.c_void_p), ("d_in_nbits", C.c_void_p),
                ("n_streams", C.c_uint64), ("seq_cap", C.c_uint32), ("binned_offset", C.c_uint32),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_n_seq", C.c_void_p), ("d_literals", C.c_void_p), ("lit_bytes", C.c_uint64), ("d_lit_off", C.c_void_p),
                ("d_lit_cap", C.c_void_p), ("d_n_lit", C.c_void_p), ("d_consumed", C.c_void_p), ("d_status", C.c_void_p)]


class Lz77EntropyWideEncodeArgs(C.Structure):
    """scl_lz77_entropy_wide_encode_args"""
    _fields_ = [("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p), ("n_seq", C.c_uint64),
                ("d_literals", C.c_void_p), ("n_lit", C.c_uint64), ("binned_offset", C.c_uint32), ("reserved", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap_bytes", C.c_uint64), ("d_nbits", C.c_void_p), ("d_status", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


class Lz77EntropyWideResult(C.Structure):
    """scl_lz77_entropy_wide_result"""
    _fields_ = [("consumed", C.c_uint64), ("n_seq", C.c_uint32), ("n_lit", C.c_uint32), ("status", C.c_uint32),
                ("sync_passes", C.c_uint32)]


class Lz77EntropyWideDecodeArgs(C.Structure):
    """scl_lz77_entropy_wide_decode_args"""
    _fields_ = [("d_in", C.c_void_p), ("in_size_bytes", C.c_uint64), ("in_bit_offset", C.c_uint64), ("in_nbits", C.c_uint64),
                ("binned_offset", C.c_uint32), ("reserved", C.c_uint32), ("seq_cap", C.c_uint64), ("lit_cap", C.c_uint64),
                ("d_lit_count", C.c_void_p), ("d_match_len", C.c_void_p), ("d_match_off", C.c_void_p),
                ("d_literals", C.c_void_p), ("d_result", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64)]


LZ77_INDEX, LZ77_PARSE = 1, 2
LZ77_WIDE_INDEX, LZ77_WIDE_SCORE, LZ77_WIDE_WALK, LZ77_WIDE_EMIT = 1, 2, 4, 8
LZ77_SLIDING_WIDE_INDEX, LZ77_SLIDING_WIDE_SPECULATE, LZ77_SLIDING_WIDE_WALK, LZ77_SLIDING_WIDE_EMIT = 1, 2, 4, 8

_u8p, _u32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)
_vp, _u32, _u64, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int

# name -> (restype, argtypes); device pointers travel as void* (integers from tensor.data_ptr())
_ENC_BATCH = [_vp, _vp, _u64, _vp, _u32, _u64, _vp, _u64, _vp, _vp, _vp, _vp]
_DEC_BATCH = [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _vp, _vp]
_ENC_HOST = [_vp, _u8p, _u64, _u8p, _u64, _u64p]
_DEC_HOST = [_vp, _u8p, _u64, _u8p, _u64, _u64p, _u64p]
_SIGNATURES = {
    "scl_last_error": (C.c_char_p, []),
    "scl_device_count": (_int, [C.POINTER(_int)]),
    "scl_abi_version": (_int, []),
    "scl_rans_encoder_kind": (_int, [_vp, _u64]),
    "scl_rans_kernel_names": (_int, [_vp, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_tans_kernel_names": (_int, [_vp, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_set_any_parameter_kernels": (_int, [_int]),
    "scl_rans_model_create": (_int, [_u32p, _u32, _u64, _u32, _u32, C.POINTER(_vp)]),
    "scl_rans_model_destroy": (None, [_vp]),
    "scl_rans_model_info": (_int, [_vp, C.POINTER(RansInfo)]),
    "scl_rans_slot_bytes": (_u64, [_vp, _u64]),
    "scl_rans_encode_batch": (_int, _ENC_BATCH),
    "scl_rans_decode_batch": (_int, _DEC_BATCH),
    "scl_rans_encode_host": (_int, _ENC_HOST),
    "scl_rans_decode_host": (_int, _DEC_HOST),
    "scl_tans_model_create": (_int, [_u32p, _u32, _u64, _u32, C.POINTER(_vp)]),
    "scl_tans_model_destroy": (None, [_vp]),
    "scl_tans_model_info": (_int, [_vp, C.POINTER(RansInfo)]),
    "scl_tans_slot_bytes": (_u64, [_vp, _u64]),
    "scl_tans_model_tables": (_int, [_vp, _u32p, _u32p, _u32p, _u32p, _u32p]),
    "scl_tans_encode_batch": (_int, _ENC_BATCH),
    "scl_tans_decode_batch": (_int, _DEC_BATCH),
    "scl_tans_encode_host": (_int, _ENC_HOST),
    "scl_tans_decode_host": (_int, _DEC_HOST),
    "scl_range_model_create": (_int, [_u32p, _u32, _u32, _u32, C.POINTER(_vp)]),
    "scl_range_model_destroy": (None, [_vp]),
    "scl_range_slot_bytes": (_u64, [_vp, _u64]),
    "scl_range_fast_path": (_int, [_vp]),
    "scl_range_encode_batch": (_int, _ENC_BATCH),
    "scl_range_decode_batch": (_int, _DEC_BATCH),
    "scl_range_encode_host": (_int, _ENC_HOST),
    "scl_range_decode_host": (_int, _DEC_HOST),
    # prefix-free codes (any code table; Huffman): added to ABI 8
    "scl_prefix_model_create": (_int, [_u32p, _u8p, _u32, C.POINTER(_vp)]),
    "scl_prefix_model_destroy": (None, [_vp]),
    "scl_prefix_model_info": (_int, [_vp, C.POINTER(PrefixInfo)]),
    "scl_prefix_kernel_names": (_int, [_vp, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_prefix_slot_bytes": (_u64, [_vp, _u64]),
    "scl_prefix_encode_batch": (_int, _ENC_BATCH),
    "scl_prefix_decode_batch": (_int, _DEC_BATCH),
    "scl_prefix_encode_host": (_int, _ENC_HOST),
    "scl_prefix_decode_host": (_int, _DEC_HOST),
    # one large block coded by the whole grid (scl_prefix_block.hip)
    "scl_prefix_block_info_get": (_int, [_vp, C.POINTER(PrefixBlockInfo)]),
    "scl_prefix_block_scratch_bytes": (_u64, [_vp, _u64, _u64]),
    "scl_prefix_encode_block": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    "scl_prefix_decode_block": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "scl_prefix_encode_block_host": (_int, _ENC_HOST),
    "scl_prefix_decode_block_host": (_int, _DEC_HOST),
    # integer codes (Golomb, universal, Elias-delta): one block coded by the whole grid (scl_uint_block.hip)
    "scl_uint_block_scratch_bytes": (_u64, [_u64, _u64]),
    "scl_uint_encode_block": (_int, [C.POINTER(UintCodeStruct), _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    "scl_uint_decode_block": (_int, [C.POINTER(UintCodeStruct), _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "scl_uint_encode_block_host": (_int, [C.POINTER(UintCodeStruct), _u32p, _u64, _u8p, _u64, _u64p, _u32p]),
    "scl_uint_decode_block_host": (_int, [C.POINTER(UintCodeStruct), _u8p, _u64, _u32p, _u64, _u64p, _u64p, _u32p]),
    "scl_uint_codeword_host": (_int, [C.POINTER(UintCodeStruct), _u32, _u32p, _u32p]),
    "scl_uint_decode_one_host": (_int, [C.POINTER(UintCodeStruct), _u32, _u32, _u32p, _u32p]),
    # ... and batched, one lane per chunk (scl_uint.hip): the prefix batch's call shape over uint32 rows
    "scl_uint_slot_bytes": (_u64, [C.POINTER(UintCodeStruct), _u64, _u32]),
    "scl_uint_encode_batch": (_int, [C.POINTER(UintCodeStruct), _vp, _u64, _vp, _u32, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "scl_uint_decode_batch": (_int, [C.POINTER(UintCodeStruct), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _vp,
                                     _vp]),
    "scl_uint_kernel_names": (_int, [C.POINTER(UintCodeStruct), _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_uint_fields_host": (_int, [C.POINTER(UintCodeStruct), _u32, _u32p, _u32p, _u32p]),
    "scl_uint_decode_wide_one_host": (_int, [C.POINTER(UintCodeStruct), _u8p, _u64, _u64, _u32, _u32p, _u32p]),
    # fixed-width codes, batched (scl_fixed.hip): widths and alphabet sizes are host arrays
    "scl_fixed_slot_bytes": (_u64, [_u64, _u32]),
    **{f"scl_fixed_encode_batch{s}": (_int, [_vp, _u64, _vp, _u32, _u32p, _u64p, _u64, _vp, _u64, _vp, _vp, _vp, _vp])
       for s in ("", "_u16", "_u32")},
    **{f"scl_fixed_decode_batch{s}": (_int, [_vp, _u64, _vp, _vp, _vp, _u32p, _u64p, _u64, _vp, _u64, _u32, _vp, _vp, _vp,
                                             _vp])
       for s in ("", "_u16", "_u32")},
    "scl_fixed_kernel_names": (_int, [_u32, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_fixed_encode_host": (_int, [_u32p, _u64, _u32, _u64, _u8p, _u64, _u64p, _u32p]),
    "scl_fixed_decode_host": (_int, [_u8p, _u64, _u64, _u64, _u32, _u64, _u32p, _u64, _u64p, _u64p, _u32p]),
    # typical-set code: tables built on the device, one block coded by the whole grid (scl_typical.hip)
    "scl_typical_model_create": (_int, [_f64p, _u32, _u32, C.c_double, C.c_double, C.POINTER(_vp)]),
    "scl_typical_model_destroy": (None, [_vp]),
    "scl_typical_model_info": (_int, [_vp, C.POINTER(TypicalInfo)]),
    "scl_typical_model_tables": (_int, [_vp, _u32p, _u32p]),
    "scl_typical_table_host": (_int, [_f64p, _u32, _u32, C.c_double, C.c_double, _u32p, _u32p]),
    "scl_typical_index_bits_host": (_u32, [_u64]),
    "scl_typical_block_scratch_bytes": (_u64, [_vp, _u64, _u64]),
    "scl_typical_encode_block": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp]),
    "scl_typical_decode_block": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "scl_typical_encode_block_host": (_int, [_vp, _vp, _u64, _u8p, _u64, _u64p, _u32p]),
    "scl_typical_decode_block_host": (_int, [_vp, _u8p, _u64, _vp, _u64, _u64p, _u64p, _u32p]),
    # LZ77: match index, greedy parse, sequence replay (scl_lz77.hip)
    "scl_lz77_scratch_bytes": (_u64, [_u64, _u64]),
    "scl_lz77_parse_batch": (_int, [C.POINTER(Lz77ParseArgs), _vp]),
    "scl_lz77_replay_batch": (_int, [C.POINTER(Lz77ReplayArgs), _vp]),
    "scl_lz77_kernel_names": (_int, [C.c_char_p, C.c_char_p, C.c_char_p, _u64]),
    "scl_lz77_parse_host": (_int, [_u8p, _u64, _u64, _u32, _u32, _u32p, _u32p, _u32p, _u64, _u64p, _u8p, _u64, _u64p]),
    "scl_lz77_replay_host": (_int, [_u8p, _u64, _u64, _u32p, _u32p, _u32p, _u64, _u8p, _u64, _u64p]),
    # LZ77 with a sliding window: hash-bucket index, lazy parse, windowed replay (scl_lz77_sliding.hip)
    "scl_lz77_sliding_scratch_bytes": (_u64, [_u64, _u64]),
    "scl_lz77_sliding_parse_batch": (_int, [C.POINTER(Lz77SlidingParseArgs), _vp]),
    "scl_lz77_sliding_replay_batch": (_int, [C.POINTER(Lz77SlidingReplayArgs), _vp]),
    "scl_lz77_sliding_kernel_names": (_int, [C.c_char_p, C.c_char_p, C.c_char_p, _u64]),
    "scl_lz77_sliding_bucket_host": (_u32, [_u8p, _u32, _u32]),
    "scl_lz77_sliding_parse_host": (_int, [_u8p, _u64, _u64, _u32, _u64, _u32, _u32, _u32, _u32, _u32p, _u32p, _u32p, _u64,
                                           _u64p, _u8p, _u64, _u64p]),
    "scl_lz77_sliding_replay_host": (_int, [_u8p, _u64, _u64, _u32, _u32p, _u32p, _u32p, _u64, _u8p, _u64, _u64p]),
    # LZ77: one large stream across the whole GPU (scl_lz77_wide.hip)
    "scl_lz77_wide_scratch_bytes": (_u64, [_u64]),
    "scl_lz77_wide_replay_scratch_bytes": (_u64, [_u64, _u64]),
    "scl_lz77_parse_wide": (_int, [C.POINTER(Lz77WideParseArgs), _vp]),
    "scl_lz77_replay_wide": (_int, [C.POINTER(Lz77WideReplayArgs), _vp]),
    "scl_lz77_wide_shape": (None, [_u32p, _u32p]),
    "scl_lz77_wide_threshold": (_u64, []),
    "scl_lz77_wide_kernel_names": (_int, [C.c_char_p, C.c_char_p, C.c_char_p, _u64]),
    # LZ77 with a sliding window: one large stream across the whole GPU (scl_lz77_sliding_wide.hip)
    "scl_lz77_sliding_wide_scratch_bytes": (_u64, [_u64]),
    "scl_lz77_sliding_parse_wide": (_int, [C.POINTER(Lz77SlidingWideParseArgs), _vp]),
    "scl_lz77_sliding_replay_wide": (_int, [C.POINTER(Lz77SlidingWideReplayArgs), _vp]),
    "scl_lz77_sliding_wide_shape": (None, [_u32p, _u32p]),
    "scl_lz77_sliding_wide_threshold": (_u64, []),
    "scl_lz77_sliding_wide_kernel_names": (_int, [C.c_char_p, C.c_char_p, C.c_char_p, _u64]),
    # LZ77: the entropy stage (scl_lz77_entropy.hip)
    "scl_lz77_entropy_encode_batch": (_int, [C.POINTER(Lz77EntropyEncodeArgs), _vp]),
    "scl_lz77_entropy_decode_batch": (_int, [C.POINTER(Lz77EntropyDecodeArgs), _vp]),
    "scl_lz77_entropy_slot_bytes": (_u64, [_u64, _u64, _u32]),
    "scl_lz77_entropy_kernel_names": (_int, [C.c_char_p, C.c_char_p, _u64]),
    "scl_lz77_huffman_from_counts_host": (_int, [_u64p, _u32, _u32p, _u8p]),
    # LZ77: the entropy stage of one large stream across the whole GPU (scl_lz77_entropy_wide.hip)
    "scl_lz77_entropy_encode_wide": (_int, [C.POINTER(Lz77EntropyWideEncodeArgs), _vp]),
    "scl_lz77_entropy_decode_wide": (_int, [C.POINTER(Lz77EntropyWideDecodeArgs), _vp]),
    "scl_lz77_entropy_wide_scratch_bytes": (_u64, [_u64, _u64, _u64]),
    "scl_lz77_entropy_wide_threshold": (_u64, []),
    "scl_lz77_entropy_wide_kernel_names": (_int, [C.c_char_p, C.c_char_p, C.c_char_p, _u64]),
    "scl_aec_model_create": (_int, [_int, _u32p, _u32, _u32, _u64, _u32, _u32, C.POINTER(_vp)]),
    "scl_aec_model_destroy": (None, [_vp]),
    "scl_aec_slot_bytes": (_u64, [_vp, _u64]),
    "scl_aec_scratch_bytes": (_u64, [_vp, _u64]),
    "scl_aec_fast_path": (_int, [_vp, _u64]),
    "scl_aec_encode_batch": (_int, _ENC_BATCH[:-1] + [_vp, _u64, _vp]),
    "scl_aec_decode_batch": (_int, _DEC_BATCH[:-1] + [_vp, _u64, _vp]),
    "scl_aec_encode_host": (_int, _ENC_HOST),
    "scl_aec_decode_host": (_int, _DEC_HOST),
    "scl_aec_state_bytes": (_u64, [_vp, _u64]),
    "scl_aec_state_counts": (_u64, [_vp]),
    "scl_aec_state_reset": (_int, [_vp, _vp, _u64, _u64, _vp]),
    "scl_aec_state_upload": (_int, [_vp, _vp, _u64, _u64, _u32p, _u32p, _vp]),
    "scl_aec_state_download": (_int, [_vp, _vp, _u64, _u64, _u32p, _u32p, _vp]),
    "scl_aec_encode_batch_resume": (_int, _ENC_BATCH[:-1] + [_vp, _u64, _u64, _vp]),
    "scl_aec_decode_batch_resume": (_int, _DEC_BATCH[:-1] + [_vp, _u64, _u64, _vp]),
    "scl_aec_encode_host_resume": (_int, _ENC_HOST + [_u32p, _u32p]),
    "scl_aec_decode_host_resume": (_int, _DEC_HOST + [_u32p, _u32p]),
    "scl_streams_compact_scratch_bytes": (_u64, [_u64]),
    "scl_streams_compact": (_int, [_vp, _vp, _vp, _u64, _int, _vp, _u64, _vp, _vp, _vp]),
    "scl_streams_compact_at": (_int, [_vp, _vp, _vp, _u64, _int, _vp, _u64, _vp, _vp, _vp, _vp]),
    # wave-striped slots (ABI 8): the tuned rANS kernels (and the tANS models they serve) on the interleaved layout
    "scl_rans_striped_ok": (_int, [_vp]),
    "scl_tans_striped_ok": (_int, [_vp]),
    "scl_range_striped_ok": (_int, [_vp]),
    "scl_range_encode_batch_striped": (_int, _ENC_BATCH),
    "scl_range_decode_batch_striped": (_int, _DEC_BATCH),
    "scl_rans_kernel_names_striped": (_int, [_vp, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_tans_kernel_names_striped": (_int, [_vp, _u64, C.c_char_p, C.c_char_p, _u64]),
    "scl_rans_encode_batch_striped": (_int, _ENC_BATCH),
    "scl_rans_decode_batch_striped": (_int, _DEC_BATCH),
    "scl_tans_encode_batch_striped": (_int, _ENC_BATCH),
    "scl_tans_decode_batch_striped": (_int, _DEC_BATCH),
    "scl_streams_compact_striped": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp, _u64, _vp, _vp, _vp, _vp]),
    "scl_stream_block_size_host": (_int, [_u8p, _u64, _u32, _u64p]),
    "scl_framed_index_host": (_int, [_vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64p, _u64p]),
    "scl_histogram_u8": (_int, [_vp, _u64, _vp, _vp]),
    "scl_histogram_u16": (_int, [_vp, _u64, _u32, _vp, _vp, _vp]),
    "scl_rccl_inject_api": (_int, [_vp]),
    "scl_rccl_comm_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "scl_rccl_unique_id": (_int, [_u8p]),
    "scl_rccl_comm_create": (_int, [_u8p, _int, _int, C.POINTER(_vp)]),
    "scl_rccl_comm_destroy": (None, [_vp]),
    "scl_rccl_allgather_u64": (_int, [_vp, _u64, _u64p, _vp]),
    "scl_rccl_allgather_async": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "scl_streams_gather_rccl": (_int, [_vp, _int, _vp, _u64, _vp, _u64p, _vp]),
    "scl_streams_gather_blocks_rccl": (_int, [_vp, _int, _vp, _u64, _vp, _u64, _vp, _vp, _u64p, _u64p, _vp]),
    "scl_streams_gatherv_rccl": (_int, [_vp, _int, _u32, C.POINTER(_vp), _u64p, C.POINTER(_vp), _u64p, _vp]),
}

# the *_u16 twins (alphabets up to 65536 symbols): same arguments, symbol arrays are uint16; host arrays travel as void*
_ENC_HOST16 = [_vp, _vp, _u64, _u8p, _u64, _u64p]
_DEC_HOST16 = [_vp, _u8p, _u64, _vp, _u64, _u64p, _u64p]
for _coder in ("rans", "tans", "range", "aec", "prefix"):
    for _op, _host in (("encode", _ENC_HOST16), ("decode", _DEC_HOST16)):
        _SIGNATURES[f"scl_{_coder}_{_op}_batch_u16"] = _SIGNATURES[f"scl_{_coder}_{_op}_batch"]
        _SIGNATURES[f"scl_{_coder}_{_op}_host_u16"] = (_int, _host)
for _op, _host in (("encode", _ENC_HOST16), ("decode", _DEC_HOST16)):
    _SIGNATURES[f"scl_aec_{_op}_batch_resume_u16"] = _SIGNATURES[f"scl_aec_{_op}_batch_resume"]
    _SIGNATURES[f"scl_aec_{_op}_host_resume_u16"] = (_int, _host + [_u32p, _u32p])

for _op, _host in (("encode", _ENC_HOST16), ("decode", _DEC_HOST16)):
    _SIGNATURES[f"scl_prefix_{_op}_block_u16"] = _SIGNATURES[f"scl_prefix_{_op}_block"]
    _SIGNATURES[f"scl_prefix_{_op}_block_host_u16"] = (_int, _host)
    _SIGNATURES[f"scl_typical_{_op}_block_u16"] = _SIGNATURES[f"scl_typical_{_op}_block"]
    _SIGNATURES[f"scl_typical_{_op}_block_host_u16"] = _SIGNATURES[f"scl_typical_{_op}_block_host"]


def any_parameter_forced() -> bool:
    """are the tuned kernels kept out of the calling thread's batch calls right now?  (``scl_set_any_parameter_kernels``
    has no getter: set-and-restore, which is thread-local and therefore race-free)"""
    L = load()
    prev = L.scl_set_any_parameter_kernels(-1)
    L.scl_set_any_parameter_kernels(prev)
    if prev >= 0:
        return prev == 1
    return os.environ.get("SCL_ANY_PARAMETER_KERNELS", "")[:1] == "1"


_lib = None
_lock = threading.Lock()


def load(path: str = None) -> C.CDLL:
    """Load libscl_hip.so and declare every entry point of include/scl_hip.h.  Raises
    ``SclHipError`` when the library was not built -- there is no fallback."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise SclHipError(E_NODEVICE, "load", f"{p} not found: build it with __graft_entry__.build() "
                              "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
        if "torch" not in sys.modules:
            # One HIP runtime per process: torch bundles its own libamdhip64, libscl_hip.so resolves to the system's.  Whichever
            # is loaded first serves both -- but if the system's comes first, torch later initialises ITS copy beside it and
            # finds no devices ("No HIP GPUs are available": __graft_entry__.build() followed by smoke() in one process,
            # round 6).  The batch entry points are fed by torch tensors anyway: let torch's runtime be the first.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(p)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI and the binding disagree
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


def last_error() -> str:
    msg = load().scl_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str) -> None:
    if rc != OK:
        raise SclHipError(rc, what, last_error())


def device_count() -> int:
    n = _int(0)
    rc = load().scl_device_count(C.byref(n))
    return n.value if rc == OK else 0


def require_device() -> None:
    if device_count() < 1:
        raise SclHipError(E_NODEVICE, "require_device", "no HIP device visible; the entropy-coding "
                          "path runs on MI355X only (no CPU fallback): " + last_error())


def u8_ptr(a: np.ndarray):
    return a.ctypes.data_as(_u8p)


def u32_ptr(a: np.ndarray):
    return a.ctypes.data_as(_u32p)


def u64_ptr(a: np.ndarray):
    return a.ctypes.data_as(_u64p)
