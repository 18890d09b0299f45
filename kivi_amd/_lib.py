"""ctypes binding of libkivi_hip.so (C ABI: include/kivi_hip.h).

Fails loudly: if the shared library has not been built (python -m kivi_amd.build
or __graft_entry__.build()) importing any op raises; nothing here falls back to
PyTorch or to the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkivi_hip.so")
# tuning sessions (KIVI_TUNING=1; A/B of two builds inside one GPU session): KIVI_HIP_LIB=/path/to/other/libkivi_hip.so
from . import _tuning  # noqa: E402

LIB_PATH = _tuning.knob("KIVI_HIP_LIB", LIB_PATH)

_i64, _i32, _vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p

_GEMV_ARGS = [_vp, _i64, _i64,            # q / a + strides
              _vp, _i64, _i64, _i64,      # code + strides
              _vp, _vp, _i64, _i64, _i64,  # scale, mn + strides
              _vp, _i64, _i64]            # out + strides

class DecodeAttendArgs(ctypes.Structure):
    """kivi_decode_attend_args (include/kivi_hip.h), field for field."""
    _fields_ = [
        ("q", _vp), ("q_sb", _i64), ("q_sh", _i64),
        ("kres", _vp), ("kres_sb", _i64), ("kres_sh", _i64), ("kres_st", _i64),
        ("knew", _vp), ("knew_sb", _i64), ("knew_sh", _i64), ("k_res_len", _i32),
        ("scores", _vp), ("s_sb", _i64), ("s_sh", _i64),
        ("inv_scale", ctypes.c_float), ("mask", _vp), ("mask_sb", _i64),
        ("v_code", _vp), ("vc_sb", _i64), ("vc_sh", _i64), ("vc_sr", _i64),
        ("v_scale", _vp), ("v_mn", _vp), ("vs_sb", _i64), ("vs_sh", _i64), ("vs_sr", _i64),
        ("vres", _vp), ("vres_sb", _i64), ("vres_sh", _i64), ("vres_st", _i64), ("v_win_start", _i32), ("v_res_len", _i32),
        ("vnew", _vp), ("vnew_sb", _i64), ("vnew_sh", _i64), ("v_flush", _i32),
        ("out", _vp), ("out_sb", _i64), ("out_sh", _i64),
        ("B", _i32), ("nh", _i32), ("nh_kv", _i32), ("D", _i32), ("group_size", _i32), ("v_bits", _i32),
        ("Tq", _i64), ("Tv", _i64),
        ("workspace", _vp), ("workspace_bytes", _i64),
        ("k_code", _vp), ("kc_sb", _i64), ("kc_sh", _i64), ("kc_sp", _i64), ("kc_sr", _i64),
        ("k_scale", _vp), ("k_mn", _vp), ("ks_sb", _i64), ("ks_sh", _i64), ("ks_sp", _i64), ("ks_sr", _i64),
        ("k_page_tokens", _i64), ("k_bits", _i32),
    ]


class LayerDesc(ctypes.Structure):
    """kivi_layer_desc (include/kivi_hip.h), field for field."""
    _fields_ = [
        ("B", _i32), ("nh_kv", _i32), ("D", _i32), ("k_bits", _i32), ("v_bits", _i32), ("group_size", _i32),
        ("residual_length", _i32), ("inv_scale", ctypes.c_float),
        ("cap", _i64), ("page_tokens", _i64), ("v_window_rows", _i64), ("s_pitch", _i64),
        ("k_code", _vp), ("kc_sb", _i64), ("kc_sh", _i64), ("kc_sp", _i64), ("kc_sr", _i64),
        ("k_scale", _vp), ("k_mn", _vp), ("ks_sb", _i64), ("ks_sh", _i64), ("ks_sp", _i64), ("ks_sr", _i64),
        ("k_res", _vp), ("kr_sb", _i64), ("kr_sh", _i64), ("kr_st", _i64),
        ("v_code", _vp), ("vc_sb", _i64), ("vc_sh", _i64), ("vc_sr", _i64),
        ("v_scale", _vp), ("v_mn", _vp), ("vs_sb", _i64), ("vs_sh", _i64), ("vs_sr", _i64),
        ("v_res", _vp), ("vr_sb", _i64), ("vr_sh", _i64), ("vr_st", _i64),
        ("scores", _vp), ("s_sb", _i64), ("s_sh", _i64),
        ("workspace", _vp), ("workspace_bytes", _i64),
    ]


class GqaDecodeArgs(ctypes.Structure):
    """kivi_gqa_decode_args of include/kivi_hip.h (field order must match)."""
    _fields_ = [
        ("B", _i32), ("nh", _i32), ("nh_kv", _i32), ("D", _i32), ("group_size", _i32), ("bits", _i32),
        ("inv_scale", ctypes.c_float),
        ("q", _vp), ("q_sb", _i64), ("q_sh", _i64),
        ("mask", _vp), ("mask_sb", _i64),
        ("kt", _vp), ("kt_sb", _i64), ("kt_sh", _i64), ("kt_ss", _i64), ("Tq", _i64),
        ("kres", _vp), ("kres_sb", _i64), ("kres_sh", _i64), ("kres_st", _i64),
        ("knew", _vp), ("knew_sb", _i64), ("knew_sh", _i64), ("k_res_len", _i32),
        ("vt", _vp), ("vt_sb", _i64), ("vt_sh", _i64), ("vt_ss", _i64), ("Tv", _i64),
        ("vres", _vp), ("vres_sb", _i64), ("vres_sh", _i64), ("vres_st", _i64), ("v_win_start", _i32), ("v_res_len", _i32),
        ("vnew", _vp), ("vnew_sb", _i64), ("vnew_sh", _i64), ("v_flush", _i32),
        ("scores", _vp), ("s_sb", _i64), ("s_sh", _i64),
        ("stats", _vp), ("stats_bytes", _i64),
        ("workspace", _vp), ("workspace_bytes", _i64),
        ("out", _vp), ("out_sb", _i64), ("out_sh", _i64),
        ("residual_length", _i32), ("v_window_rows", _i64), ("kt_superblocks", _i64), ("vt_superblocks", _i64),
        ("flags", _i32),
        ("kt_range", _vp), ("vt_range", _vp),
        ("dyn_step", _vp),
    ]


class MfStep(ctypes.Structure):
    """kivi_mf_step (include/kivi_hip.h): the six lengths of a decode step, host copy of the device-resident struct."""
    _fields_ = [("Tq", _i64), ("Tv", _i64), ("k_res_len", _i32), ("v_res_len", _i32), ("v_win_start", _i32), ("v_flush", _i32)]


GQA_FORCE_SPLIT, GQA_FORCE_ROW, GQA_WINDOW_RING, GQA_DUMP_SCORES = 1, 2, 4, 8


def gqa_slices(n: int) -> int:
    """KIVI_GQA_SLICES(n): force the one-launch form with n slices per row (nh / nh_kv in {4, 8}; tests, tuning)."""
    return (n & 0xFF) << 8


class MfLayerDesc(ctypes.Structure):
    """kivi_mf_layer_desc (include/kivi_hip.h), field for field."""
    _fields_ = [
        ("B", _i32), ("nh_kv", _i32), ("D", _i32), ("bits", _i32), ("group_size", _i32), ("residual_length", _i32),
        ("inv_scale", ctypes.c_float),
        ("cap", _i64), ("v_window_rows", _i64), ("s_pitch", _i64),
        ("kt", _vp), ("kt_sb", _i64), ("kt_sh", _i64), ("kt_ss", _i64),
        ("vt", _vp), ("vt_sb", _i64), ("vt_sh", _i64), ("vt_ss", _i64),
        ("k_res", _vp), ("kr_sb", _i64), ("kr_sh", _i64), ("kr_st", _i64),
        ("v_res", _vp), ("vr_sb", _i64), ("vr_sh", _i64), ("vr_st", _i64),
        ("scores", _vp), ("s_sb", _i64), ("s_sh", _i64),
        ("stats", _vp), ("stats_bytes", _i64),
        ("workspace", _vp), ("workspace_bytes", _i64),
        ("flags", _i32),
        ("kt_range", _vp), ("vt_range", _vp),
    ]


REORDER_MAX_SLABS = 32    # include/kivi_hip.h: KIVI_REORDER_MAX_SLABS
REORDER_MAX_GROUP = 1024
SAMPLE_MAX_B = 65535      # include/kivi_hip.h: KIVI_SAMPLE_MAX_B, KIVI_SAMPLE_MAX_V
SAMPLE_MAX_V = 1 << 20
SAMPLE_MAX_LIST = 1024      # include/kivi_hip.h: KIVI_SAMPLE_MAX_LIST
STOP_MAX_IDS, STOP_MAX_SEQS, STOP_MAX_LEN = 16, 8, 16    # include/kivi_hip.h: KIVI_STOP_MAX_*
MOE_TOKEN_TILE, MOE_NORM_TOPK, MOE_ROUND_WEIGHTS = 16, 1, 2    # include/kivi_hip.h: KIVI_MOE_*
MOE_MAX_E, MOE_MAX_K = 256, 16


class ReorderSlab(ctypes.Structure):
    """kivi_reorder_slab (include/kivi_hip.h): byte (i0, i1, i2, j) of row b at base + b*row_stride + sum(i_k*stride[k]) + j."""
    _fields_ = [("base", _vp), ("row_stride", _i64), ("n", _i64 * 3), ("stride", _i64 * 3), ("run", _i64)]


class AdmitSlab(ctypes.Structure):
    """kivi_admit_slab (include/kivi_hip.h): a slab with base, row stride and level strides per side (destination, source); the level
    counts and the run are shared."""
    _fields_ = [("dst_base", _vp), ("dst_row_stride", _i64), ("dst_stride", _i64 * 3),
                ("src_base", _vp), ("src_row_stride", _i64), ("src_stride", _i64 * 3), ("n", _i64 * 3), ("run", _i64)]


# name -> (restype, argtypes); must list every symbol include/kivi_hip.h declares
SIGNATURES = {
    "kivi_abi_version": (_i32, []),
    "kivi_last_error": (ctypes.c_char_p, []),
    "kivi_device_error": (_i32, []),
    "kivi_quant_pack_lastdim": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "kivi_quant_pack_k_tmajor": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64,
                                        _i64, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_unpack_dequant_lastdim": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "kivi_pack_codes_lastdim": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp]),
    "kivi_unpack_codes_lastdim": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp]),
    "kivi_gemv_k": (_i32, _GEMV_ARGS + [_i32, _i32, _i32, _i32, _i64, _i32, _i32, _vp]),
    "kivi_gemv_v": (_i32, _GEMV_ARGS + [_i32, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_gemv_outer_dim": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "kivi_gemv_k_paged": (_i32, [_i32, _i64, _i64, _i64] + _GEMV_ARGS + [_i32, _i32, _i32, _i32, _i64, _i32, _i32, _vp]),
    "kivi_decode_scores": (_i32, [_i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64,
                                  _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                  _i32, _i32, _i32, _i32, _i64, _i32, _i32, _vp]),
    "kivi_softmax_scaled": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, ctypes.c_float, _vp, _i64, _i32, _vp]),
    "kivi_decode_output": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64,
                                  _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                  _i32, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_decode_softmax_output": (_i32, [_vp, _i64, _i64, ctypes.c_float, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64,
                                          _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _i32, _vp, _i64,
                                          _i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_decode_attend": (_i32, [ctypes.POINTER(DecodeAttendArgs), _vp]),
    "kivi_decode_layer": (_i32, [ctypes.POINTER(LayerDesc), ctypes.POINTER(_i64), _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                 _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp]),
    # (a KT / VT store = pointer + 3 word strides + the pointer to its range flags)
    "kivi_kt_pack": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_vt_pack": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_kt_relayout": (_i32, [_i32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                _i64, _i32, _i32, _i32, _vp]),
    "kivi_vt_relayout": (_i32, [_i32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                _i64, _i32, _i32, _i32, _vp]),
    "kivi_gqa_scores": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _i32,
                               _i32, _vp]),
    "kivi_gqa_output": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _i32,
                               _i32, _vp, _i64, _vp]),
    "kivi_gqa_decode": (_i32, [ctypes.POINTER(GqaDecodeArgs), _vp]),
    "kivi_gqa_decode_lead": (_i32, [ctypes.POINTER(GqaDecodeArgs), _vp, _vp]),
    "kivi_mf_launch_plan": (_i32, [_i32, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32]),
    "kivi_mf_decode_layer": (_i32, [ctypes.POINTER(MfLayerDesc), ctypes.POINTER(_i64), _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                    _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp]),
    "kivi_mf_decode_layer_dyn": (_i32, [ctypes.POINTER(MfLayerDesc), ctypes.POINTER(MfStep), _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                        _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp]),
    # (the same two with a per-row lead -- B int32 of device memory or null -- before the stream)
    "kivi_mf_decode_layer_lead": (_i32, [ctypes.POINTER(MfLayerDesc), ctypes.POINTER(_i64), _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                         _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "kivi_mf_decode_layer_dyn_lead": (_i32, [ctypes.POINTER(MfLayerDesc), ctypes.POINTER(MfStep), _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64,
                                             _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "kivi_mf_extend_layer": (_i32, [ctypes.POINTER(MfLayerDesc), ctypes.POINTER(_i64), _i32, _vp, _i64, _i64, _i64, _i32, _vp, _i64,
                                    _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp]),
    "kivi_vt_pack_at": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_cache_reorder": (_i32, [ctypes.POINTER(ReorderSlab), _i32, _i32, _i32, _vp, _i32, _vp]),
    "kivi_cache_snapshot": (_i32, [ctypes.POINTER(ReorderSlab), _i32, _i32, _vp, ctypes.c_size_t, _i32, _vp]),
    "kivi_cache_admit": (_i32, [ctypes.POINTER(AdmitSlab), _i32, _i32, _vp, _i32, _i32, _vp]),
    "kivi_mf_store_shift": (_i32, [_vp, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _vp]),
    "kivi_mf_store_admit": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i64,
                                   _i64, _vp]),
    "kivi_sample": (_i32, [_vp, _i32, _i64, _i32, _i32, ctypes.c_float, _i32, ctypes.c_float, ctypes.c_float, _vp, _vp, _i64, _vp]),
    "kivi_sample_rows": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "kivi_sample_rows_pen": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "kivi_seen_mark": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp]),
    "kivi_sample_rows_con": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "kivi_allow_mark": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp]),
    "kivi_stop_rows": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp]),
    "kivi_token_logprob": (_i32, [_vp, _i32, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "kivi_token_top_logprobs": (_i32, [_vp, _i32, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "kivi_prefill_attention": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp,
                                      _i32, _i32, _i32, _i32, _i32, ctypes.c_float, _vp]),
    "kivi_qk_rope": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, ctypes.c_float, _vp, _vp,
                            _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "kivi_qkv_rope_bf16": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp,
                                  ctypes.c_float, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "kivi_moe_max_tiles": (_i32, [_i32, _i32, _i32]),
    "kivi_moe_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "kivi_moe_route": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kivi_moe_experts": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64,
                                _vp]),
    "kivi_moe_experts_w8": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                   _vp, _i64, _vp]),
    "kivi_w4_bytes": (_i64, [_i32, _i32, _i32]),
    "kivi_w4_pack": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "kivi_w4_dequant": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "kivi_w4_linear": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kivi_w4_gate_up": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kivi_w8_bytes": (_i64, [_i32, _i32]),
    "kivi_w8_dequant": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    "kivi_w8_linear": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kivi_w8_gate_up": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kivi_lora_shrink": (_i32, [_vp, _i64, _i32, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "kivi_lora_expand": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _i64, _i64, _i32, _vp]),
    "kivi_mf_step_key": (_i64, [ctypes.POINTER(MfStep), _i32, _i32, _i32, _i32, _i32]),
    "kivi_mf_step_advance": (_i32, [ctypes.POINTER(MfStep), _i32, _i64]),
    "kivi_mf_step_upload": (_i32, [ctypes.POINTER(MfStep), _vp, _vp]),
    "kivi_gemv_awq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp]),
    "kivi_gemv_k_num_variants": (_i32, []),
    "kivi_gemv_k_variant_name": (ctypes.c_char_p, [_i32]),
    "kivi_gemv_k_variant": (_i32, [_i32] + _GEMV_ARGS + [_i32, _i32, _i32, _i32, _i64, _i32, _i32, _vp]),
    "kivi_gemv_v_num_variants": (_i32, []),
    "kivi_gemv_v_variant_name": (ctypes.c_char_p, [_i32]),
    "kivi_gemv_v_variant": (_i32, [_i32] + _GEMV_ARGS + [_i32, _i32, _i32, _i64, _i32, _i32, _i32, _vp]),
    "kivi_event_create": (_vp, []),
    "kivi_event_destroy": (None, [_vp]),
    "kivi_set_launch_events": (None, [_vp, _vp]),
    "kivi_event_elapsed_us": (ctypes.c_float, [_vp, _vp]),
    "kivi_last_timed_kernel": (ctypes.c_char_p, []),
    "kivi_debug_set_stamps": (None, [_vp]),
}

_lib = None


class KiviHipError(RuntimeError):
    rc = None


ABI_VERSION = 3      # include/kivi_hip.h: KIVI_ABI_VERSION (3: range words with an explicit byte 2, ticket ids always, device error word)


class KiviTimeout(KiviHipError):
    """KIVI_ETIMEOUT: a block of an EARLIER sliced launch gave up waiting for a partner (that step's output holds NaN for the unit);
    the error is cleared by being reported, the next call runs normally."""


class KiviUnsupported(KiviHipError):
    """KIVI_EUNSUPPORTED: valid request, no tuned kernel for this shape (callers may compose the unfused ops)."""


def load() -> ctypes.CDLL:
    """Load the library once; raise (never fall back) if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KiviHipError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -m kivi_amd.build). "
            "kivi_amd has no CPU / PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.kivi_abi_version() != ABI_VERSION:
        raise KiviHipError(f"ABI version mismatch: library reports {lib.kivi_abi_version()}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().kivi_last_error().decode(errors="replace")
        err = {-3: KiviUnsupported, -4: KiviTimeout}.get(rc, KiviHipError)(f"{what} failed (rc={rc}): {msg}")
        err.rc = rc
        raise err


def stream_ptr(t: torch.Tensor) -> ctypes.c_void_p:
    """hipStream_t of torch's current stream on the tensor's device."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise KiviHipError(f"{name} must live on the GPU (got device={t.device}); kivi_amd has no CPU path")


def ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


LOGITS_BF16 = 0x110   # include/kivi_hip.h: KIVI_LOGITS_BF16
LOGITS_BITS = {torch.float16: 16, torch.float32: 32, torch.bfloat16: LOGITS_BF16}   # dtype -> `logits_bits` of the fused logits entries


# --------------------------------------------------------------------------- tensors -> arguments of a layer step
def unit_rows(x: torch.Tensor) -> torch.Tensor:
    """`x` if its inner stride is 1 (what every kernel that reads rows needs), a contiguous copy otherwise."""
    return x if x.stride(3) == 1 else x.contiguous()


def rows16(x: torch.Tensor) -> torch.Tensor:
    """16-byte loads of whole rows: unit inner stride, 16-byte aligned rows (a copy otherwise)."""
    ok = x.stride(3) == 1 and x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0
    return x if ok else x.contiguous()


def check_mask_size(attention_mask: torch.Tensor, size: tuple) -> None:
    """The reference's complaint about an additive mask of the wrong shape (llama_kivi.py:364-368)."""
    if attention_mask.size() != size:
        raise ValueError(f"Attention mask should be of size {size}, but is {attention_mask.size()}")


def mask_arg(attention_mask, B: int, kv_len: int, wider: bool = False):
    """(pointer, batch stride) of a decode step's additive (B, 1, 1, kv_len) fp16 mask; (None, 0) without one.  `wider`: a static
    buffer whose rows are longer than the step's row (graph replays) passes."""
    if attention_mask is None:
        return None, 0
    if wider:
        assert attention_mask.shape[3] >= kv_len
    else:
        check_mask_size(attention_mask, (B, 1, 1, kv_len))
    assert attention_mask.dtype == torch.float16 and attention_mask.stride(3) == 1
    return attention_mask.data_ptr(), attention_mask.stride(0)


def lead_arg(lead, B: int):
    """Pointer of a decode step's per-row lead: (B,) int32 on the device, contiguous; None without one."""
    if lead is None:
        return None
    assert lead.dtype == torch.int32 and tuple(lead.shape) == (B,) and lead.is_contiguous() and lead.is_cuda
    return lead.data_ptr()


def out_arg(out, shape: tuple, device) -> torch.Tensor:
    """The fp16 result buffer of a layer step: the caller's (checked) or a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float16, device=device)
    assert out.shape == shape and out.dtype == torch.float16 and out.stride(3) == 1
    return out
