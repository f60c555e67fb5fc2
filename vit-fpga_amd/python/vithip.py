"""ctypes binding of libvithip.so — the thin host-side mirror used by tests/, bench.py and
__graft_entry__.py.  Everything goes through the C ABI declared in include/vithip.h; there is
no Python compute path and no fallback: if the library is missing, import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("VITHIP_LIB") or os.path.join(PKG_ROOT, "libvithip.so")   # VITHIP_LIB: A/B builds (tools/)

DTYPE_BF16, DTYPE_FP16, DTYPE_FP8 = 0, 1, 2
FLAG_LN_FOLD_OFF, FLAG_LN_FOLD_ON, FLAG_W8_E4M3, FLAG_CLS_TAIL = 1, 2, 4, 8   # vh_config.flags
FLAG_PRE_LN, FLAG_QUICK_GELU = 16, 32   # CLIP's vision towers: LayerNorm in front of layer 0, x * sigmoid(1.702 x) in the MLP
FLAG_REGISTERS_MASK, MAX_REGISTERS = 31 << 9, 16


def FLAG_REGISTERS(n):
    """VH_FLAG_REGISTERS(n): n register tokens (0 .. 16) between the class token and the patch rows, in bits 9 .. 13 of flags."""
    return (int(n) & 31) << 9


def registers_of(flags):
    """VH_FLAG_REGISTERS_OF(flags)."""
    return (int(flags) & FLAG_REGISTERS_MASK) >> 9


# Pooled heads and models without a class token (VH_FLAG_NO_CLS, VH_FLAG_POOL; vithip.h): model bits, in the blob header too
FLAG_NO_CLS, FLAG_POOL_MASK = 1 << 15, 3 << 16
POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM, POOL_CLS_AVG = range(4)


def FLAG_POOL(m):
    """VH_FLAG_POOL(m): the head's input, POOL_CLS (LN(row 0)), POOL_AVG_NORM (mean LN(patch rows)), POOL_AVG_FCNORM (LN(mean patch
    rows)) or POOL_CLS_AVG (concat of the first two, head [C, 2 D]), in bits 16 .. 17 of flags."""
    return (int(m) & 3) << 16


def pool_of(flags):
    """VH_FLAG_POOL_OF(flags)."""
    return (int(flags) & FLAG_POOL_MASK) >> 16


# SigLIP's vision towers (VH_FLAG_MAP_HEAD, VH_FLAG_TANH_GELU; vithip.h): model bits, in the blob header too.  MAP_HEAD: the head's
# input is the attention-pooling block (needs FLAG_NO_CLS, at most MAP_MAX_HEADS heads); TANH_GELU: gelu_pytorch_tanh in the MLP
FLAG_MAP_HEAD, FLAG_TANH_GELU, MAP_MAX_HEADS = 1 << 19, 1 << 21, 16

# Rotary position embedding (VH_FLAG_ROPE; vithip.h): a model bit, in the blob header too.  q and k of the patch rows are rotated in
# every layer by the blob's last two tensors rope.cos / rope.sin [NP][head_dim / 2]; excludes FLAG_CLS_TAIL
FLAG_ROPE = 1 << 23

# SwiGLU MLP (VH_FLAG_SWIGLU; vithip.h): a model bit, in the blob header too.  mlp_dim = M is the gated width; fc1 of every layer is
# [2 M, dim] + [2 M] (gate rows, then value rows) and h = silu(g) * u is made by a pass of its own behind fc1.  Excludes FLAG_QUICK_GELU,
# FLAG_TANH_GELU, FLAG_MAP_HEAD, FLAG_CLS_TAIL, FLAG_W8_E4M3 and DTYPE_FP8
FLAG_SWIGLU = 1 << 25


EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_F32, EPI_PATCH, EPI_LNFOLD, EPI_LNFOLD_GELU, EPI_RESID_LN, EPI_RESID_SPLIT, EPI_PATCH_SPLIT = range(10)
EPI_BIAS_QGELU, EPI_LNFOLD_QGELU = 10, 11
# tanh GELU (12 is no code).  tests/gemm_exact.py enumerates every EPI_* name of this module, so these two run through the exact GEMM
# suite like every other code (its emulator knows the erf, QuickGELU and tanh activations); tests/test_gpu_siglip.py sweeps the
# activation itself.  EPILOGUE_*: the names the codes had while that suite skipped them, kept for their users
EPI_BIAS_TGELU, EPI_LNFOLD_TGELU = 13, 14
EPILOGUE_BIAS_TGELU, EPILOGUE_LNFOLD_TGELU = EPI_BIAS_TGELU, EPI_LNFOLD_TGELU
ELEM_F32, ELEM_F16, ELEM_BF16, ELEM_U8 = range(4)   # element type of an image tensor (VH_ELEM_*)
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1                      # its layout (VH_LAYOUT_*): [B][S][S][C] / [B][C][S][S]
ELEM_BYTES = {ELEM_F32: 4, ELEM_F16: 2, ELEM_BF16: 2, ELEM_U8: 1}
ACT_IDENTITY, ACT_RELU2, ACT_RELU, ACT_HARDTANH, ACT_GELU = range(5)

STAGES = ["im2col", "patch_gemm", "cls_rows", "layernorm", "qkv_gemm", "attention", "proj_gemm",
          "fc1_gemm", "fc2_gemm", "final_layernorm", "head_gemm", "ln_stats", "pre_layernorm"]
# the stages of a forward (what profile_forward reports), and behind them the one launch that is no part of it: the resize of the
# frames entry points (vh_stage_name(len(STAGES)); set_stage_timing takes it like any other)
STAGE_RESIZE = "resize"
TIMED_STAGES = STAGES + [STAGE_RESIZE]


class VhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libvithip error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("channels", C.c_int32),
                ("dim", C.c_int32), ("heads", C.c_int32), ("mlp_dim", C.c_int32),
                ("layers", C.c_int32), ("classes", C.c_int32), ("dtype", C.c_int32),
                ("max_batch", C.c_int32), ("ln_eps", C.c_float), ("flags", C.c_int32)]


class Frame(C.Structure):
    """vh_frame: one 8-bit interleaved frame inside the buffer of a call, and the box to resample to image_size^2."""
    _fields_ = [("offset", C.c_uint64), ("height", C.c_int32), ("width", C.c_int32), ("row_stride", C.c_int32),
                ("box", C.c_float * 4)]


class FrameNV12(C.Structure):
    """vh_frame_nv12: one NV12 frame (a Y plane and a plane of interleaved U,V pairs) inside the buffer of a call, and the box (in
    luma pixels) to resample to image_size^2."""
    _fields_ = [("y_offset", C.c_uint64), ("uv_offset", C.c_uint64), ("height", C.c_int32), ("width", C.c_int32),
                ("y_stride", C.c_int32), ("uv_stride", C.c_int32), ("box", C.c_float * 4)]


class FrameYUV(C.Structure):
    """vh_frame_yuv: one planar YUV frame (three byte planes; chroma sub-sampled by sub_x, sub_y = 1 or 2) inside the buffer of a
    call, and the box (in luma pixels) to resample to image_size^2.  72 bytes."""
    _fields_ = [("y_offset", C.c_uint64), ("u_offset", C.c_uint64), ("v_offset", C.c_uint64), ("height", C.c_int32),
                ("width", C.c_int32), ("y_stride", C.c_int32), ("u_stride", C.c_int32), ("v_stride", C.c_int32),
                ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("box", C.c_float * 4), ("reserved", C.c_int32)]


class FrameYUY2(C.Structure):
    """vh_frame_yuy2: one packed 4:2:2 frame (one plane of macropixels in the order of `layout`, L422_*) inside the buffer of a call,
    and the box (in luma pixels) to resample to image_size^2.  40 bytes."""
    _fields_ = [("offset", C.c_uint64), ("height", C.c_int32), ("width", C.c_int32), ("row_stride", C.c_int32),
                ("layout", C.c_int32), ("box", C.c_float * 4)]


FEAT_NORM, FEAT_RAW = 0, 1   # vh_features.norm (VH_FEAT_*): through the model's final LayerNorm / the residual stream as it is
FEAT_FORM_F32 = -1           # op_token_features: fp32 rows instead of split planes (DTYPE_* = the planes of that path)


class Features(C.Structure):
    """vh_features: where the token features of the last forward go (host or device pointers, None = not wanted), their element
    type (ELEM_F32 / ELEM_F16 / ELEM_BF16) and FEAT_NORM / FEAT_RAW.  32 bytes."""
    _fields_ = [("cls", C.c_void_p), ("patch", C.c_void_p), ("mean", C.c_void_p), ("elem", C.c_int32), ("norm", C.c_int32)]


FEAT_ROWS, FEAT_NCHW = 0, 1   # vh_layer_features.patch_layout (VH_FEAT_*): patch [B, NP, D] / [B, D, gh, gw]
MAX_FEATURE_LAYERS = 8


class LayerFeatures(C.Structure):
    """vh_layer_features: Features + reg (the register rows), layer (-1 / cfg.layers = the final state, else a listed layer of the
    last forward) and patch_layout (FEAT_ROWS / FEAT_NCHW).  48 bytes."""
    _fields_ = [("cls", C.c_void_p), ("patch", C.c_void_p), ("mean", C.c_void_p), ("reg", C.c_void_p), ("elem", C.c_int32),
                ("norm", C.c_int32), ("layer", C.c_int32), ("patch_layout", C.c_int32)]


MAX_ATTENTION_LAYERS = 64
ATTN_Q_CLS, ATTN_Q_LEAD = 0, 1        # vh_set_attention_layers queries (VH_ATTN_Q_*): the class token's row / every leading row
ATTN_KEYS_ALL, ATTN_KEYS_PATCH = 0, 1  # vh_attention_maps.keys (VH_ATTN_KEYS_*): all key columns / the patch columns


class AttentionMaps(C.Structure):
    """vh_attention_maps: where the attention maps of the last forward go (host or device pointers, None = not wanted): probs
    [B, H, Q, K], head_mean [B, Q, K]; element type, layer (-1 = the last layer, else a listed layer), keys (ATTN_KEYS_*) and a
    reserved 0.  32 bytes."""
    _fields_ = [("probs", C.c_void_p), ("head_mean", C.c_void_p), ("elem", C.c_int32), ("layer", C.c_int32), ("keys", C.c_int32),
                ("reserved", C.c_int32)]


L422_YUYV, L422_UYVY, L422_YVYU, L422_VYUY, L422_V210 = range(5)   # vh_frame_yuy2.layout (VH_422_*); V210: the 16-bit entry points only
class FrameBGRA(C.Structure):
    """vh_frame_bgra: one packed 4:4:4 frame (one plane of pixels whose samples lie as `layout`, L444_*, says) inside the buffer of a
    call, and the box (in pixels) to resample to image_size^2.  40 bytes."""
    _fields_ = [("offset", C.c_uint64), ("height", C.c_int32), ("width", C.c_int32), ("row_stride", C.c_int32),
                ("layout", C.c_int32), ("box", C.c_float * 4)]


def layout_444(p0, p1, p2, four, yuv):
    """VH_444: p_k = the index within the pixel of the sample that becomes output component k; four: 4 samples per pixel, else 3;
    yuv: the samples pass the colour matrix."""
    return p0 | p1 << 2 | p2 << 4 | (64 if four else 0) | (128 if yuv else 0)


# vh_frame_bgra.layout (VH_444_*), memory order in the name
L444_RGB, L444_BGR = layout_444(0, 1, 2, 0, 0), layout_444(2, 1, 0, 0, 0)
L444_RGBA, L444_BGRA, L444_ARGB, L444_ABGR = (layout_444(0, 1, 2, 1, 0), layout_444(2, 1, 0, 1, 0), layout_444(1, 2, 3, 1, 0),
                                              layout_444(3, 2, 1, 1, 0))
L444_YUV24, L444_VUYA, L444_AYUV = layout_444(0, 1, 2, 0, 1), layout_444(2, 1, 0, 1, 1), layout_444(1, 2, 3, 1, 1)
L444_Y416, L444_AYUV64 = layout_444(1, 0, 2, 1, 1), layout_444(1, 2, 3, 1, 1)     # 16-bit words: the _y410 entry points
L444_Y410, L444_V410 = layout_444(1, 0, 2, 1, 1) | 256, layout_444(1, 0, 2, 1, 1) | 768   # one 32-bit word of three 10-bit codes
CHROMA_CENTER, CHROMA_LEFT = 0, 1          # vh_set_frame_colour / vh_op_resize_nv12: JPEG / MPEG-1 siting, MPEG-2 / H.264 / HEVC siting
YUV_BT601, YUV_BT709, YUV_BT2020 = 0, 1, 2  # vh_yuv_matrix

# every exported symbol of include/vithip.h: name -> (restype, argtypes)
_vp, _i, _i64, _u64, _sz, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float
_pi = C.POINTER(C.c_int)
SYMBOLS = {
    "vh_abi_version": (_i, []),
    "vh_device_count": (_i, [_pi]),
    "vh_last_error": (C.c_char_p, [_vp]),
    "vh_malloc": (_i, [_i, _sz, C.POINTER(_vp)]),
    "vh_free": (_i, [_i, _vp]),
    "vh_memcpy_h2d": (_i, [_i, _vp, _vp, _sz]),
    "vh_memcpy_d2h": (_i, [_i, _vp, _vp, _sz]),
    "vh_device_synchronize": (_i, [_i]),
    "vh_create": (_i, [C.POINTER(Config), _i, C.POINTER(_vp)]),
    "vh_destroy": (_i, [_vp]),
    "vh_get_config": (_i, [_vp, C.POINTER(Config)]),
    "vh_get_register_tokens": (_i, [_vp]),
    "vh_get_ln_fold": (_i, [_vp, _pi]),
    "vh_get_ln_guard": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), _pi]),
    "vh_get_fp8_guard": (_i, [_vp, C.POINTER(_f), C.POINTER(_f)]),
    "vh_weight_blob_bytes": (_sz, [C.POINTER(Config)]),
    "vh_load_weights": (_i, [_vp, _vp, _sz]),
    "vh_load_weights_device": (_i, [_vp, _vp, _sz]),
    "vh_init_weights_seeded": (_i, [_vp, _u64]),
    "vh_export_weights": (_i, [_vp, _vp, _sz]),
    "vh_export_weights_device": (_i, [_vp, _vp, _sz]),
    "vh_forward": (_i, [_vp, _vp, _i, _vp]),
    "vh_forward_device": (_i, [_vp, _vp, _i, _vp]),
    "vh_forward_device_async": (_i, [_vp, _vp, _i, _vp, _i]),
    "vh_synchronize": (_i, [_vp]),
    "vh_set_input_norm": (_i, [_vp, _vp, _vp]),
    "vh_get_input_norm": (_i, [_vp, _vp, _vp]),
    "vh_forward_u8": (_i, [_vp, _vp, _i, _vp]),
    "vh_forward_device_u8": (_i, [_vp, _vp, _i, _vp]),
    "vh_forward_device_u8_async": (_i, [_vp, _vp, _i, _vp, _i]),
    "vh_forward_tensor": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vh_forward_device_tensor": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vh_forward_device_tensor_async": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "vh_resize_table": (_i, [_i, C.c_double, C.c_double, _i, _vp, _vp, _vp, _i]),
    "vh_forward_frames_u8": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_u8": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_yuv_matrix": (_i, [_i, _i, _vp]),
    "vh_set_frame_colour": (_i, [_vp, _vp, _i]),
    "vh_get_frame_colour": (_i, [_vp, _vp, _pi]),
    "vh_forward_frames_nv12": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_nv12": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_yuv": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_yuv": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_yuv_matrix16": (_i, [_i, _i, _i, _i, _vp]),
    "vh_set_frame_colour16": (_i, [_vp, _vp, _i]),
    "vh_get_frame_colour16": (_i, [_vp, _vp, _pi]),
    "vh_forward_frames_p016": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_p016": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_yuv16": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_yuv16": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_yuy2": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_yuy2": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_y210": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_y210": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_bgra": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_bgra": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_frames_y410": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_forward_device_frames_y410": (_i, [_vp, _vp, _sz, _vp, _i, _vp]),
    "vh_fill_input_seeded": (_i, [_vp, _u64, _i, _vp]),
    "vh_last_forward_us": (_i, [_vp, C.POINTER(_i64)]),
    "vh_last_kernel_ms": (_i, [_vp, C.POINTER(C.c_double)]),
    "vh_profile_forward": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_double), _i, _pi]),
    "vh_stage_name": (C.c_char_p, [_i]),
    "vh_filter_create": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_void_p)]),
    "vh_filter_destroy": (_i, [_vp]),
    "vh_filter_free_slots": (_i, [_vp, _pi]),
    "vh_filter_submit": (_i, [_vp, _vp]),
    "vh_filter_collect": (_i, [_vp, _vp]),
    "vh_filter_last_error": (C.c_char_p, [_vp]),
    "vh_device_mem_info": (_i, [_i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vh_blob_file_config": (_i, [C.c_char_p, C.POINTER(Config)]),
    "vh_blob_file_read": (_i, [C.c_char_p, _vp, _sz]),
    "vh_save_weights_file": (_i, [_vp, C.c_char_p]),
    "vh_load_weights_file": (_i, [_vp, C.c_char_p]),
    "vh_ring_create": (_i, [_vp, _i, _i]),
    "vh_ring_destroy": (_i, [_vp]),
    "vh_ring_free_slots": (_i, [_vp, _pi]),
    "vh_ring_input": (_i, [_vp, C.POINTER(C.POINTER(C.c_float))]),
    "vh_ring_submit": (_i, [_vp, _vp, _i]),
    "vh_ring_collect": (_i, [_vp, _vp, _pi]),
    "vh_ring_create_u8": (_i, [_vp, _i, _i]),
    "vh_ring_input_u8": (_i, [_vp, C.POINTER(C.POINTER(C.c_uint8))]),
    "vh_ring_submit_u8": (_i, [_vp, _vp, _i]),
    "vh_ring_create_tensor": (_i, [_vp, _i, _i, _i, _i]),
    "vh_ring_input_tensor": (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "vh_ring_submit_tensor": (_i, [_vp, _vp, _i]),
    "vh_ring_create_frames": (_i, [_vp, _i, _i, _sz]),
    "vh_ring_input_frames": (_i, [_vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(_sz)]),
    "vh_ring_submit_frames": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_nv12": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_yuv": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_p016": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_yuv16": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_yuy2": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_y210": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_bgra": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_ring_submit_frames_y410": (_i, [_vp, _vp, _sz, _vp, _i]),
    "vh_set_graph": (_i, [_vp, _i]),
    "vh_get_graph": (_i, [_vp, _pi, _pi]),
    "vh_set_streams": (_i, [_vp, _i]),
    "vh_get_streams": (_i, [_vp, _pi]),
    "vh_get_inflight": (_i, [_vp, _pi]),
    "vh_set_stage_timing": (_i, [_vp, _i]),
    "vh_get_stage_timing": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), _pi]),
    "vh_set_step_timing": (_i, [_vp, _i]),
    "vh_get_step_timing": (_i, [_vp, C.POINTER(C.c_double), _i, _pi]),
    "vh_debug_read": (_i, [_vp, _i, _vp, _sz]),
    "vh_debug_set_layers": (_i, [_vp, _i]),
    "vh_features_dims": (_i, [_vp, _pi, _pi, _pi, _pi]),
    "vh_read_features": (_i, [_vp, _vp]),
    "vh_read_features_device": (_i, [_vp, _vp]),
    "vh_read_features_device_async": (_i, [_vp, _vp]),
    "vh_set_feature_layers": (_i, [_vp, _pi, _i]),
    "vh_get_feature_layers": (_i, [_vp, _pi, _pi]),
    "vh_read_layer_features": (_i, [_vp, _vp]),
    "vh_read_layer_features_device": (_i, [_vp, _vp]),
    "vh_read_layer_features_device_async": (_i, [_vp, _vp]),
    "vh_set_attention_layers": (_i, [_vp, _pi, _i, _i]),
    "vh_get_attention_layers": (_i, [_vp, _pi, _pi, _pi]),
    "vh_attention_dims": (_i, [_vp, _pi, _pi, _pi, _pi, _pi]),
    "vh_read_attention": (_i, [_vp, _vp]),
    "vh_read_attention_device": (_i, [_vp, _vp]),
    "vh_read_attention_device_async": (_i, [_vp, _vp]),
    "vh_op_gemm": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "vh_op_gemm_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "vh_op_gemm_fp8_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "vh_op_quantize_rows": (_i, [_vp, _i, _i, C.c_float, _vp, _vp, _vp]),
    "vh_op_gemm_ex": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "vh_op_gemm_layout": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "vh_op_gemm_lead": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i64, _i, _i, _vp]),
    "vh_op_lead_rows": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vh_op_gemm_fp8_layout": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vh_op_tile_rows": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "vh_op_rowstats_cast": (_i, [_vp, _i64, _i, _f, _vp, _vp, _i, _vp]),
    "vh_op_finalize_stats": (_i, [_vp, _i, _i64, _i, _f, _vp, _vp]),
    "vh_op_pre_layernorm": (_i, [_vp, _i64, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _vp]),
    "vh_op_rowstats_split": (_i, [_vp, _i64, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "vh_op_fold_ln": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "vh_op_layernorm": (_i, [_vp, _i64, _i, _i64, _vp, _vp, _f, _vp, _i, _vp]),
    "vh_op_rowstats_guard": (_i, [_vp, _i64, _i, _f, _vp, _vp, _vp, _i, _i64, _vp, _vp]),
    "vh_op_pre_layernorm_guard": (_i, [_vp, _i64, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp]),
    "vh_op_finalize_stats_guard": (_i, [_vp, _i, _i64, _i, _f, _vp, _i64, _vp, _vp, _vp]),
    "vh_op_ln_guard": (_i, [_vp, _i64, _vp, _vp]),
    "vh_op_layernorm_f32": (_i, [_vp, _i64, _i, _i64, _vp, _vp, _f, _vp, _vp]),
    "vh_op_layernorm_split": (_i, [_vp, _vp, _i64, _i, _i64, _vp, _vp, _f, _vp, _i, _vp]),
    "vh_op_head_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "vh_op_fold_ln_f8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "vh_op_fake_quant_rows": (_i, [_vp, _i, _i, _vp, _vp]),
    "vh_op_attention": (_i, [_vp, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_attention_stream": (_i, [_vp, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_attention_hd": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_attention_cls": (_i, [_vp, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_attention_layout": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i64, _vp]),
    "vh_op_attention_probs": (_i, [_vp, _i, _i, _i, _i, _i, _i64, _i, _vp, _vp]),
    "vh_op_attention_readout": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "vh_op_im2col": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_im2col_padded": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "vh_op_im2col_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "vh_op_im2col_tensor": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "vh_op_resize_u8": (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _vp]),
    "vh_op_resize_nv12": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_yuv": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_p016": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_yuv16": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_yuy2": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_y210": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_bgra": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_resize_y410": (_i, [_vp, _sz, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "vh_op_cast": (_i, [_vp, _vp, _i64, _i, _vp]),
    "vh_op_token_features": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _i, _vp, _vp, _vp]),
    "vh_op_token_features2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "vh_op_pool_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp]),
    "vh_op_map_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _vp, _i, _vp, _vp]),
    "vh_op_rope": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i64, _vp, _vp, _vp]),
    "vh_op_swiglu": (_i, [_vp, _i, _i64, _i, _vp, _i, _vp]),
    "vh_op_fill": (_i, [_vp, _i64, _u64, C.c_uint32, _i, _f, _vp]),
    "vh_bench_gemm": (_i, [_i, _i64, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_double)]),
    "vh_group_create": (_i, [C.POINTER(Config), _pi, _i, C.POINTER(_vp)]),
    "vh_group_destroy": (_i, [_vp]),
    "vh_group_size": (_i, [_vp, _pi]),
    "vh_group_member": (_i, [_vp, _i, C.POINTER(_vp), _pi]),
    "vh_group_last_error": (C.c_char_p, [_vp]),
    "vh_group_shard_bounds": (None, [_i, _i, _i, _pi, _pi]),
    "vh_group_load_weights": (_i, [_vp, _vp, _sz]),
    "vh_group_init_weights_seeded": (_i, [_vp, _u64]),
    "vh_group_broadcast_weights": (_i, [_vp]),
    "vh_group_forward": (_i, [_vp, _vp, _i, _vp]),
    "vh_group_fill_inputs_seeded": (_i, [_vp, _u64, _i]),
    "vh_group_forward_resident": (_i, [_vp, _i, _i]),
    "vh_group_read_logits": (_i, [_vp, _i, _vp]),
    "vh_mlp_create": (_i, [_i, _i, _i, _pi, _i, C.POINTER(_vp)]),
    "vh_mlp_load_params": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vh_mlp_forward": (_i, [_vp, _vp, _i, _vp]),
    "vh_mlp_last_forward_us": (_i, [_vp, C.POINTER(_i64)]),
    "vh_mlp_init_gradient": (_i, [_vp, _vp, _vp, _i]),
    "vh_mlp_launch_gradient": (_i, [_vp, _i, _f, _f, _vp]),
    "vh_mlp_read_params": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "vh_mlp_last_gradient_us": (_i, [_vp, C.POINTER(_i64)]),
    "vh_mlp_last_error": (C.c_char_p, [_vp]),
    "vh_mlp_destroy": (_i, [_vp]),
}

_lib = None


def lib():
    """Load libvithip.so (in-tree build).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: run `make -C vit-fpga_amd` (or "
                              "__graft_entry__.build()); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib().vh_last_error(ctx)
        raise VhError(rc, msg.decode() if msg else "?")


def device_count():
    n = C.c_int(0)
    rc = lib().vh_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def blob_file_config(path):
    """Model shape stored in a VHBLOB1 file (host only) -> dict usable as `cfg`."""
    c = Config()
    _check(lib().vh_blob_file_config(os.fsencode(path), C.byref(c)))
    return {k: getattr(c, k) for k in ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")}, c.ln_eps


def blob_file_flags(path):
    """The model bits of a VHBLOB1 file's header as vh_config flags (FLAG_PRE_LN, FLAG_QUICK_GELU, FLAG_REGISTERS(n), FLAG_NO_CLS,
    FLAG_POOL(m), FLAG_MAP_HEAD, FLAG_TANH_GELU, FLAG_ROPE, FLAG_SWIGLU); host only."""
    c = Config()
    _check(lib().vh_blob_file_config(os.fsencode(path), C.byref(c)))
    return c.flags


# The header's flags word (byte 52) carries the model bits of vh_config flags: these two at header positions of their own, the rest at
# their flag positions (bit 0 of the word belongs to the file form's checksum).
_HEADER_BITS = ((FLAG_PRE_LN, 2), (FLAG_QUICK_GELU, 4))
_SAME_BITS = FLAG_REGISTERS_MASK | FLAG_NO_CLS | FLAG_POOL_MASK | FLAG_MAP_HEAD | FLAG_TANH_GELU | FLAG_ROPE | FLAG_SWIGLU


def _blob_bits(flags):
    """vh_config flags -> the model bits of a blob header's flags word."""
    return sum(h for f, h in _HEADER_BITS if flags & f) | (flags & _SAME_BITS)


def blob_flags_of(blob):
    """The model bits of a memory blob's header as vh_config flags (what blob_file_flags returns for a file)."""
    bits = int(np.ascontiguousarray(blob[52:56]).view(np.uint32)[0])
    return sum(f for f, h in _HEADER_BITS if bits & h) | (bits & _SAME_BITS)


def _blob_header(cfg, ln_eps, flags):
    """The 64-byte header of a memory blob: magic, the model shape, ln_eps and the model bits of the flags word (byte 52)."""
    h = np.zeros(64, dtype=np.uint8)
    h[:7] = np.frombuffer(b"VHBLOB1", dtype=np.uint8)
    h[8:40] = np.array([cfg[k] for k in ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")],
                       dtype=np.int32).view(np.uint8)
    h[40:44] = np.array([ln_eps], dtype=np.float32).view(np.uint8)
    h[52:56] = np.array([_blob_bits(flags)], dtype=np.uint32).view(np.uint8)
    return h


def blob_tensor_table(cfg, flags=0):
    """[(name, shape)] of the canonical blob's fp32 tensors behind the header, in blob order, for a context of these model flags: the
    names of include/vithip.h's blob section.  The one statement of the order on the Python side; every converter packs through it."""
    D, M, E, P, CH, H = cfg["dim"], cfg["mlp_dim"], cfg["classes"], cfg["patch_size"], cfg["channels"], cfg["heads"]
    NP = (cfg["image_size"] // P) ** 2
    R, cls = registers_of(flags), 0 if flags & FLAG_NO_CLS else 1
    t = [("patch.weight", (D, CH, P, P)), ("patch.bias", (D,))] + [("cls", (D,))] * cls + [("pos", (NP + cls, D))]
    if R:
        t.append(("reg", (R, D)))
    if flags & FLAG_PRE_LN:
        t += [("pre_ln.weight", (D,)), ("pre_ln.bias", (D,))]
    rows = {"ln1": (D,), "q": (D, D), "k": (D, D), "v": (D, D), "o": (D, D), "ln2": (D,),
            "fc1": (2 * M if flags & FLAG_SWIGLU else M, D), "fc2": (D, M)}   # FLAG_SWIGLU: gate rows, then value rows
    for l in range(cfg["layers"]):
        for n, shape in rows.items():
            t += [(f"l{l}.{n}.weight", shape), (f"l{l}.{n}.bias", shape[:1])]
    t += [("lnf.weight", (D,)), ("lnf.bias", (D,)), ("head.weight", (E, 2 * D if pool_of(flags) == POOL_CLS_AVG else D)), ("head.bias", (E,))]
    if flags & FLAG_MAP_HEAD:
        t += [("map.qk", (H, D)), ("map.v.weight", (D, D)), ("map.v.bias", (D,)), ("map.o.weight", (D, D)), ("map.o.bias", (D,)),
              ("map.ln.weight", (D,)), ("map.ln.bias", (D,)), ("map.fc1.weight", (M, D)), ("map.fc1.bias", (M,)),
              ("map.fc2.weight", (D, M)), ("map.fc2.bias", (D,))]
    if flags & FLAG_ROPE:
        t += [("rope.cos", (NP, D // H // 2)), ("rope.sin", (NP, D // H // 2))]
    return t


def _pack_blob(me, cfg, ln_eps, flags, tensors):
    """The blob of a converter's `tensors` {blob_tensor_table name: array}: every name of the table, with exactly its element count."""
    parts = [_blob_header(cfg, ln_eps, flags)]
    for name, shape in blob_tensor_table(cfg, flags):
        if name not in tensors:
            raise KeyError(f"{me}: no tensor for {name}")
        a = np.ascontiguousarray(tensors[name], dtype=np.float32).reshape(-1)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{me}: {name} has {a.size} elements, the blob holds {tuple(shape)}")
        parts.append(a.view(np.uint8))
    return np.concatenate(parts)


def _taker(sd, me):
    """take(name, shape, f) of a converter: tensor `name` of the state dict, checked for presence and shape, flattened as type f."""
    def take(name, shape, f=np.float32):
        if name not in sd:
            raise KeyError(f"{me}: missing tensor {name}")
        a = np.asarray(sd[name])
        if a.shape != tuple(shape):
            raise ValueError(f"{me}: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}")
        return np.ascontiguousarray(a, dtype=f).reshape(-1)
    return take


def _take_named(take, cfg, flags, top, layer_prefix, layer):
    """{our name: tensor} for the rows of blob_tensor_table that a converter's name table covers.  top: {our name: their name, or
    (their name, their shape) where it is not ours, or None for a row the converter fills itself}; layer: {ln1, q, ..: their
    module} under layer_prefix.format(l)."""
    names = {f"l{l}.{ours}.{wb}": f"{layer_prefix.format(l)}{theirs}.{wb}"
             for l in range(cfg["layers"]) for ours, theirs in layer.items() for wb in ("weight", "bias")}
    names.update(top)
    out = {}
    for name, shape in blob_tensor_table(cfg, flags):
        theirs = names.get(name)
        if theirs is not None:
            out[name] = take(theirs, shape) if isinstance(theirs, str) else take(*theirs)
    return out


def _scaled(take, sd, D, n_in, module, lname, optional=False):
    """LayerScale folded into the layer it scales: diag(lambda) W and lambda b in float64, one rounding to fp32 (exact for
    lambda == 1).  optional: a checkpoint without `lname` has no LayerScale."""
    w, b = take(module + ".weight", (D, n_in), np.float64).reshape(D, n_in), take(module + ".bias", (D,), np.float64)
    if not optional or lname in sd:
        lam = take(lname, (D,), np.float64)
        w, b = w * lam[:, None], b * lam
    return w.astype(np.float32).reshape(-1), b.astype(np.float32)


def _head(me, head, E, W):
    """(weight, bias) of a converter's `head` argument: zeros when there is none."""
    if head is None:
        return np.zeros(E * W, np.float32), np.zeros(E, np.float32)
    hw, hb = (np.asarray(a) for a in head)
    if hw.shape != (E, W) or hb.shape != (E,):
        raise ValueError(f"{me}: head has shapes {hw.shape}, {hb.shape}, expected {(E, W)}, {(E,)}")
    return hw, hb


def _register_count(me, cfg, sd, key):
    """cfg['registers'], which must be the row count of the checkpoint's register tensor `key` (absent: 0)."""
    R = int(cfg.get("registers", 0))
    have = int(np.asarray(sd[key]).shape[-2]) if key in sd else 0
    if have != R:
        raise ValueError(f"{me}: the checkpoint has {have} register tokens, cfg['registers'] is {R}")
    return R


def _gated_mlp(me, take, sd, cfg, l, gate, up, down, lname):
    """The four MLP tensors of layer l of a FLAG_SWIGLU blob from a gated checkpoint.  gate / up: (tensor name stem, first row, rows) of
    the two halves of fc1 (one tensor `weights_in`, or `gate_proj` and `up_proj`); down: fc2's stem; LayerScale `lname` is folded into
    fc2 in float64, one rounding.  A hidden width M' that is no multiple of 64 is zero-padded to cfg['mlp_dim'], a larger multiple of 64:
    gate rows, value rows, both bias halves and fc2's columns -- exact, silu(0) * 0 = 0 meets zero columns.  Any other width is refused."""
    D, M = cfg["dim"], cfg["mlp_dim"]
    if down + ".weight" not in sd:
        raise KeyError(f"{me}: missing tensor {down}.weight")
    Mc = int(np.asarray(sd[down + ".weight"]).shape[-1])
    if Mc != M and not (Mc % 64 and M > Mc and M % 64 == 0):
        raise ValueError(f"{me}: {down}.weight has a hidden width of {Mc}, cfg['mlp_dim'] is {M}"
                         " (only a width that is no multiple of 64 is zero-padded, to a larger multiple of 64)")
    w1, b1 = np.zeros((2 * M, D), np.float32), np.zeros(2 * M, np.float32)
    for half, (stem, r0, total) in enumerate((gate, up)):
        w1[half * M:half * M + Mc] = take(stem + ".weight", (total, D)).reshape(total, D)[r0:r0 + Mc]
        b1[half * M:half * M + Mc] = take(stem + ".bias", (total,))[r0:r0 + Mc]
    w2c, b2 = _scaled(take, sd, D, Mc, down, lname)
    w2 = np.zeros((D, M), np.float32)
    w2[:, :Mc] = w2c.reshape(D, Mc)
    return {f"l{l}.fc1.weight": w1, f"l{l}.fc1.bias": b1, f"l{l}.fc2.weight": w2, f"l{l}.fc2.bias": b2}


def _gated_names(me, sd, swiglu, plain, gated):
    """The refusals both DINO converters share, once swiglu=True is given: the checkpoint must have every name stem of `gated` in some
    layer and none of `plain`."""
    has = lambda stem: any(k.endswith(stem + ".weight") for k in sd)
    if not swiglu:
        return
    if has(plain) and any(has(g) for g in gated):
        raise ValueError(f"{me}: the checkpoint has both {plain} and a gated MLP ({gated[0]}): one of them is not this model's")
    missing = [g for g in gated if not has(g)]
    if missing:
        raise ValueError(f"{me}: swiglu=True, but the checkpoint has no {missing[0]}")


def _check_dino_args(me, cfg, pool):
    if pool not in (POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM, POOL_CLS_AVG):
        raise ValueError(f"{me}: pool = {pool} is not POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM or POOL_CLS_AVG")
    R = int(cfg.get("registers", 0))
    if not 0 <= R <= MAX_REGISTERS:
        raise ValueError(f"{me}: cfg['registers'] = {R} is outside 0 .. {MAX_REGISTERS}")


# their module of each of our layer tensors; o and fc2 are missing where LayerScale is folded into them
_CLIP_LAYER = {"ln1": "layer_norm1", "q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.out_proj",
               "ln2": "layer_norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
_DINOV2_LAYER = {"ln1": "norm1", "q": "attention.attention.query", "k": "attention.attention.key", "v": "attention.attention.value",
                 "ln2": "norm2", "fc1": "mlp.fc1"}
_DINOV3_LAYER = {"ln1": "norm1", "q": "attention.q_proj", "k": "attention.k_proj", "v": "attention.v_proj", "ln2": "norm2", "fc1": "mlp.up_proj"}
_IJEPA_LAYER = {"ln1": "layernorm_before", "q": "attention.q_proj", "k": "attention.k_proj", "v": "attention.v_proj", "o": "attention.o_proj",
                "ln2": "layernorm_after", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
_TIMM_LAYER = {"ln1": "norm1", "ln2": "norm2", "fc1": "mlp.fc1"}


def blob_from_clip_state_dict(sd, cfg, ln_eps=1e-5):
    """Canonical blob of a CLIP vision tower from a dict of arrays under the Hugging Face `CLIPVisionModelWithProjection`
    parameter names (numpy only; torch tensors: pass `{k: v.numpy() for k, v in model.state_dict().items()}`).
    `cfg`: the model shape with classes = the projection width, plus `flags` (FLAG_PRE_LN always; FLAG_QUICK_GELU for
    hidden_act == "quick_gelu").  CLIP's patch convolution and projection have no bias: both are written as zeros; the
    header carries the model bits.  A missing or wrongly shaped tensor is refused by name."""
    me = "blob_from_clip_state_dict"
    flags = cfg.get("flags", FLAG_PRE_LN)
    if not flags & FLAG_PRE_LN:
        raise ValueError(f"{me}: every CLIP vision tower has ln_pre: cfg['flags'] needs FLAG_PRE_LN")
    if flags & ~(FLAG_PRE_LN | FLAG_QUICK_GELU):
        raise ValueError(f"{me}: cfg['flags'] takes the model bits FLAG_PRE_LN | FLAG_QUICK_GELU only")
    v, emb = "vision_model.", "vision_model.embeddings."
    top = {"patch.weight": emb + "patch_embedding.weight", "cls": emb + "class_embedding", "pos": emb + "position_embedding.weight",
           "pre_ln.weight": v + "pre_layrnorm.weight", "pre_ln.bias": v + "pre_layrnorm.bias",
           "lnf.weight": v + "post_layernorm.weight", "lnf.bias": v + "post_layernorm.bias", "head.weight": "visual_projection.weight"}
    t = _take_named(_taker(sd, me), cfg, flags, top, v + "encoder.layers.{}.", _CLIP_LAYER)
    t["patch.bias"], t["head.bias"] = np.zeros(cfg["dim"], np.float32), np.zeros(cfg["classes"], np.float32)
    return _pack_blob(me, cfg, ln_eps, flags, t)


def blob_from_dinov2_state_dict(sd, cfg, ln_eps=1e-6, head=None, pool=POOL_CLS, swiglu=False):
    """Canonical blob of a DINOv2 backbone from a dict of arrays under the Hugging Face `Dinov2Model` /
    `Dinov2WithRegistersModel` parameter names (numpy only; torch tensors: `{k: v.numpy() for k, v in model.state_dict().items()}`).
    `cfg`: the model shape, `registers` = the number of register tokens (0 for the models without), classes = the head's width.
    LayerScale is folded into the layer it scales, exactly: W_o' = diag(lambda1) W_o, b_o' = lambda1 b_o, and fc2 with lambda2
    likewise, computed in float64 and rounded once to fp32.  The backbone has no head: it is zero unless head = (weight
    [classes, dim], bias [classes]) is given.  `embeddings.mask_token` is ignored.  Refused: a SwiGLU MLP (mlp.weights_in), a
    position table whose row count is not NP + 1 of cfg (nothing is interpolated here), a register count other than
    cfg['registers'], a missing or wrongly shaped tensor (by name).
    pool = POOL_CLS_AVG: the published ImageNet linear classifiers (`Dinov2ForImageClassification`,
    `Dinov2WithRegistersForImageClassification`: head(concat(cls, mean of the patch tokens)), head weight [classes, 2 dim], the
    class-token half first).  A state dict of those models is taken as it is: the `dinov2.` / `dinov2_with_registers.` prefix is
    dropped and `classifier.*` is the head unless `head` is given.  The head's shape is checked against the mode ([classes, dim]
    for POOL_CLS / POOL_AVG_NORM / POOL_AVG_FCNORM); the header carries FLAG_POOL(pool).
    swiglu=True (DINOv2-g/14, `use_swiglu_ffn`): a FLAG_SWIGLU blob from `mlp.weights_in.{weight, bias}` [2 M', dim] (gate half first)
    and `mlp.weights_out.{weight, bias}`; cfg['mlp_dim'] is the gated width M', or a larger multiple of 64 where M' is none (688 -> 704, or 768
    to reach the folded loop; the padding is zeros, and exact: _gated_mlp).  Refused by name: a checkpoint with `mlp.fc1` beside the gated names, or without one of
    them.  Without swiglu=True a gated checkpoint is refused as before."""
    me = "blob_from_dinov2_state_dict"
    _check_dino_args(me, cfg, pool)
    for prefix in ("dinov2.", "dinov2_with_registers."):
        if any(k.startswith(prefix) for k in sd):
            if head is None and "classifier.weight" in sd and "classifier.bias" in sd:
                head = (sd["classifier.weight"], sd["classifier.bias"])
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    D, M, E = cfg["dim"], cfg["mlp_dim"], cfg["classes"]
    NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
    if not swiglu and any(k.endswith("mlp.weights_in.weight") for k in sd):
        raise ValueError(f"{me}: the checkpoint has a SwiGLU MLP (mlp.weights_in), which this library does not run")
    _gated_names(me, sd, swiglu, "mlp.fc1", ("mlp.weights_in", "mlp.weights_out"))
    emb = "embeddings."
    R = _register_count(me, cfg, sd, emb + "register_tokens")
    if emb + "position_embeddings" in sd:
        rows = int(np.asarray(sd[emb + "position_embeddings"]).shape[-2])
        if rows != NP + 1:
            raise ValueError(f"{me}: {emb}position_embeddings has {rows} rows, cfg needs NP + 1 = {NP + 1} "
                             "(interpolate the table to the image size first)")
    flags = FLAG_REGISTERS(R) | FLAG_POOL(pool) | (FLAG_SWIGLU if swiglu else 0)
    take = _taker(sd, me)
    top = {"patch.weight": emb + "patch_embeddings.projection.weight", "patch.bias": emb + "patch_embeddings.projection.bias",
           "cls": (emb + "cls_token", (1, 1, D)), "pos": (emb + "position_embeddings", (1, NP + 1, D)),
           "reg": (emb + "register_tokens", (1, R, D)), "lnf.weight": "layernorm.weight", "lnf.bias": "layernorm.bias"}
    t = _take_named(take, cfg, flags, top, "encoder.layer.{}.", {k: v for k, v in _DINOV2_LAYER.items() if not (swiglu and k == "fc1")})
    for l in range(cfg["layers"]):
        b = f"encoder.layer.{l}."
        t[f"l{l}.o.weight"], t[f"l{l}.o.bias"] = _scaled(take, sd, D, D, b + "attention.output.dense", b + "layer_scale1.lambda1")
        if swiglu:
            Mc = int(np.asarray(sd[b + "mlp.weights_out.weight"]).shape[-1]) if b + "mlp.weights_out.weight" in sd else M
            t.update(_gated_mlp(me, take, sd, cfg, l, (b + "mlp.weights_in", 0, 2 * Mc), (b + "mlp.weights_in", Mc, 2 * Mc), b + "mlp.weights_out",
                                b + "layer_scale2.lambda1"))
        else:
            t[f"l{l}.fc2.weight"], t[f"l{l}.fc2.bias"] = _scaled(take, sd, D, M, b + "mlp.fc2", b + "layer_scale2.lambda1")
    t["head.weight"], t["head.bias"] = _head(me, head, E, 2 * D if pool == POOL_CLS_AVG else D)
    return _pack_blob(me, cfg, ln_eps, flags, t)


def blob_from_siglip_state_dict(sd, cfg, ln_eps=1e-6, hidden_act="gelu_pytorch_tanh"):
    """Canonical blob of a SigLIP vision tower from a dict of arrays under the Hugging Face parameter names (numpy only), with or
    without the `vision_model.` prefix.  Two models:
      `SiglipVisionModel` (no `classifier.*`): a FLAG_NO_CLS | FLAG_MAP_HEAD context whose head is the identity -- cfg['classes'] must
      equal cfg['dim'] -- so that the logits ARE `pooler_output`.  The attention-pooling head's query is one learned vector, so it is
      folded through the key projection here, in float64, one rounding to fp32:  map.qk[h] = W_k,h^T (W_q,h probe + b_q,h) / sqrt(hd)
      (the key bias shifts every score of a head alike and drops out of the softmax; the library has no fold code).  map.v.* = the
      value third of `head.attention.in_proj_*`, map.o.* = `head.attention.out_proj.*`, map.ln.* = `head.layernorm.*`, map.fc1 / fc2 =
      `head.mlp.*`.
      `SiglipForImageClassification` (`classifier.*` present): head(mean of the post-LayerNormed patch tokens), a FLAG_NO_CLS |
      FLAG_POOL(POOL_AVG_NORM) context with the classifier as its head; the tower's `head.*` is not used by that model and is ignored.
    hidden_act: "gelu_pytorch_tanh" (every published SigLIP) -> FLAG_TANH_GELU, "gelu" -> erf GELU, "quick_gelu" -> FLAG_QUICK_GELU.  The
    header carries the flags; blob_flags_of(blob) returns them.  Refused: a position table whose row count is not NP of cfg (interpolate
    first), more than MAP_MAX_HEADS heads with the MAP head, classes != dim without a classifier, a missing or wrongly shaped tensor."""
    me = "blob_from_siglip_state_dict"
    acts = {"gelu_pytorch_tanh": FLAG_TANH_GELU, "gelu": 0, "quick_gelu": FLAG_QUICK_GELU}
    if hidden_act not in acts:
        raise ValueError(f"{me}: hidden_act = {hidden_act!r} is not one of {sorted(acts)}")
    D, E, H = cfg["dim"], cfg["classes"], cfg["heads"]
    NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
    if any(k.startswith("vision_model.") for k in sd):
        sd = dict({k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")},
                  **{k: v for k, v in sd.items() if k.startswith("classifier.")})
    classifier = "classifier.weight" in sd and "classifier.bias" in sd
    flags = FLAG_NO_CLS | acts[hidden_act] | (FLAG_POOL(POOL_AVG_NORM) if classifier else FLAG_MAP_HEAD)
    if not classifier and E != D:
        raise ValueError(f"{me}: without a classifier the head is the identity: cfg['classes'] = {E} must equal cfg['dim'] = {D}")
    if not classifier and H > MAP_MAX_HEADS:
        raise ValueError(f"{me}: the attention-pooling head takes at most {MAP_MAX_HEADS} heads, cfg['heads'] is {H}")
    emb, h = "embeddings.", "head."
    if emb + "position_embedding.weight" in sd:
        rows = int(np.asarray(sd[emb + "position_embedding.weight"]).shape[0])
        if rows != NP:
            raise ValueError(f"{me}: {emb}position_embedding.weight has {rows} rows, cfg needs NP = {NP} (interpolate the table first)")
    take = _taker(sd, me)
    top = {"patch.weight": emb + "patch_embedding.weight", "patch.bias": emb + "patch_embedding.bias", "pos": emb + "position_embedding.weight",
           "lnf.weight": "post_layernorm.weight", "lnf.bias": "post_layernorm.bias",
           "map.o.weight": h + "attention.out_proj.weight", "map.o.bias": h + "attention.out_proj.bias",
           "map.ln.weight": h + "layernorm.weight", "map.ln.bias": h + "layernorm.bias", "map.fc1.weight": h + "mlp.fc1.weight",
           "map.fc1.bias": h + "mlp.fc1.bias", "map.fc2.weight": h + "mlp.fc2.weight", "map.fc2.bias": h + "mlp.fc2.bias"}
    if classifier:
        top.update({"head.weight": "classifier.weight", "head.bias": "classifier.bias"})
    t = _take_named(take, cfg, flags, top, "encoder.layers.{}.", _CLIP_LAYER)
    if not classifier:
        t["head.weight"], t["head.bias"] = np.eye(D, dtype=np.float32), np.zeros(D, np.float32)
        hd = D // H
        probe = take(h + "probe", (1, 1, D), np.float64)
        w = take(h + "attention.in_proj_weight", (3 * D, D), np.float64).reshape(3, D, D)
        bias = take(h + "attention.in_proj_bias", (3 * D,), np.float64).reshape(3, D)
        q = ((w[0] @ probe + bias[0]) / np.sqrt(float(hd))).reshape(H, hd)               # the query of every image, scaled
        t["map.qk"] = np.einsum("hj,hjk->hk", q, w[1].reshape(H, hd, D))                  # through the key projection, per head
        t["map.v.weight"], t["map.v.bias"] = w[2], bias[2]
    return _pack_blob(me, cfg, ln_eps, flags, t)


def rope_tables_dinov3(grid, head_dim, theta=100.0):
    """(cos, sin) [grid * grid, head_dim / 2] fp32: the rope.cos / rope.sin tensors of a DINOv3 ViT (Hugging Face
    `DINOv3ViTRopePositionEmbedding` without augmentation).  Patch p = (y, x) of the grid has coordinates cy = 2 (y + 0.5) / grid - 1 and
    cx likewise; column a < head_dim / 2, with i = a mod head_dim / 4, holds the angle 2 pi (cy if a < head_dim / 4 else cx)
    theta^(-4 i / head_dim).  Computed in float64, rounded once."""
    if head_dim % 4:
        raise ValueError(f"rope_tables_dinov3: head_dim = {head_dim} is not a multiple of 4")
    q = head_dim // 4
    c = 2.0 * (np.arange(grid, dtype=np.float64) + 0.5) / grid - 1.0
    cy, cx = (a.reshape(-1) for a in np.meshgrid(c, c, indexing="ij"))
    inv = float(theta) ** (-4.0 * np.arange(q, dtype=np.float64) / head_dim)
    ang = 2.0 * np.pi * np.concatenate([cy[:, None] * inv[None, :], cx[:, None] * inv[None, :]], axis=1)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def blob_from_dinov3_state_dict(sd, cfg, ln_eps=1e-5, head=None, pool=POOL_CLS, theta=100.0, swiglu=False):
    """Canonical blob of a DINOv3 ViT-S/B/L backbone from a dict of arrays under the Hugging Face `DINOv3ViTModel` parameter names
    (numpy only): `embeddings.{cls_token, register_tokens, patch_embeddings.{weight, bias}}`, `model.layer.N.` or `layer.N.` +
    `{norm1, attention.{q,k,v,o}_proj, layer_scale1.lambda1, norm2, mlp.{up,down}_proj, layer_scale2.lambda1}`, `norm`.
    `cfg`: the model shape, `registers` = the number of register tokens, classes = the head's width.  `embeddings.mask_token` is
    ignored; a missing `k_proj.bias` is zeros (key_bias=False).  LayerScale is folded into o_proj and down_proj in float64, one
    rounding, as blob_from_dinov2_state_dict does.  The model has no position table: pos is zeros; the last two tensors are
    rope_tables_dinov3(grid, head dim, theta).  The head is zero unless head = (weight [classes, dim], bias [classes]) is given; with
    an identity head `vh_read_features(VH_FEAT_NORM)` / debug tap 1 is the model's `pooler_output` (the normalised class token).
    Header flags: FLAG_ROPE | FLAG_REGISTERS(R) | FLAG_POOL(pool).  Refused by name: a gated MLP (mlp.gate_proj: the H+ and 7B
    checkpoints), a register count other than cfg['registers'], a missing or wrongly shaped tensor.
    swiglu=True (ViT-H+/16 and 7B, `use_gated_mlp` with hidden_act = "silu"): a FLAG_ROPE | FLAG_SWIGLU blob; fc1 = `mlp.gate_proj` rows, then
    `mlp.up_proj` rows, fc2 = `mlp.down_proj`; cfg['mlp_dim'] is `intermediate_size` (or a larger multiple of 64 where it is none: zero
    padding, exact).  Refused by name: `mlp.fc1` beside the gated names, a missing gate_proj / up_proj / down_proj.  Without swiglu=True a
    gated checkpoint is refused as before."""
    me = "blob_from_dinov3_state_dict"
    _check_dino_args(me, cfg, pool)
    D, M, E, H = cfg["dim"], cfg["mlp_dim"], cfg["classes"], cfg["heads"]
    g = cfg["image_size"] // cfg["patch_size"]
    if not swiglu and any(k.endswith("mlp.gate_proj.weight") for k in sd):
        raise ValueError(f"{me}: the checkpoint has a gated MLP (mlp.gate_proj), which this library does not run")
    _gated_names(me, sd, swiglu, "mlp.fc1", ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"))
    emb = "embeddings."
    R = _register_count(me, cfg, sd, emb + "register_tokens")
    pre = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."
    flags = FLAG_ROPE | FLAG_REGISTERS(R) | FLAG_POOL(pool) | (FLAG_SWIGLU if swiglu else 0)
    take = _taker(sd, me)
    top = {"patch.weight": emb + "patch_embeddings.weight", "patch.bias": emb + "patch_embeddings.bias", "cls": (emb + "cls_token", (1, 1, D)),
           "reg": (emb + "register_tokens", (1, R, D)), "lnf.weight": "norm.weight", "lnf.bias": "norm.bias"}
    no_key_bias = [f"l{l}.k.bias" for l in range(cfg["layers"]) if f"{pre}{l}.attention.k_proj.bias" not in sd]      # key_bias=False: zeros
    top.update(dict.fromkeys(no_key_bias))
    t = _take_named(take, cfg, flags, top, pre + "{}.", {k: v for k, v in _DINOV3_LAYER.items() if not (swiglu and k == "fc1")})
    t.update({n: np.zeros(D, np.float32) for n in no_key_bias})
    t["pos"] = np.zeros((g * g + 1) * D, np.float32)                                      # the model has no position table
    for l in range(cfg["layers"]):
        b = f"{pre}{l}."
        t[f"l{l}.o.weight"], t[f"l{l}.o.bias"] = _scaled(take, sd, D, D, b + "attention.o_proj", b + "layer_scale1.lambda1")
        if swiglu:
            Mc = int(np.asarray(sd[b + "mlp.down_proj.weight"]).shape[-1]) if b + "mlp.down_proj.weight" in sd else M
            t.update(_gated_mlp(me, take, sd, cfg, l, (b + "mlp.gate_proj", 0, Mc), (b + "mlp.up_proj", 0, Mc), b + "mlp.down_proj", b + "layer_scale2.lambda1"))
        else:
            t[f"l{l}.fc2.weight"], t[f"l{l}.fc2.bias"] = _scaled(take, sd, D, M, b + "mlp.down_proj", b + "layer_scale2.lambda1")
    t["head.weight"], t["head.bias"] = _head(me, head, E, 2 * D if pool == POOL_CLS_AVG else D)
    t["rope.cos"], t["rope.sin"] = rope_tables_dinov3(g, D // H, theta)
    return _pack_blob(me, cfg, ln_eps, flags, t)


def blob_from_ijepa_state_dict(sd, cfg, ln_eps=1e-6, head=None):
    """Canonical blob of an I-JEPA encoder from a dict of arrays under the Hugging Face `IJepaModel` / `IJepaForImageClassification`
    parameter names (`ijepa.embeddings.*`, `ijepa.layers.N.attention.{q,k,v,o}_proj`, `layernorm_before` / `layernorm_after`,
    `mlp.fc1` / `mlp.fc2`, `ijepa.layernorm`, `classifier`; an `IJepaModel` dict without the `ijepa.` prefix is taken too; numpy
    only).  The model has no class token and its classifier is head(mean(LN(x))): the blob is one of a FLAG_NO_CLS |
    FLAG_POOL(POOL_AVG_NORM) context -- no `cls` tensor, pos [NP, dim] -- and its header says so.  The head is `classifier.*`, else
    head = (weight [classes, dim], bias [classes]), else zero.  `embeddings.mask_token` is ignored.  Refused: a `cls_token` in the
    state dict, a position table whose row count is not NP of cfg, a wrongly shaped head, a missing or wrongly shaped tensor (by name)."""
    me = "blob_from_ijepa_state_dict"
    D, E = cfg["dim"], cfg["classes"]
    NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
    if not any(k.startswith("ijepa.") for k in sd):
        sd = dict({"ijepa." + k: v for k, v in sd.items() if not k.startswith("classifier.")},
                  **{k: v for k, v in sd.items() if k.startswith("classifier.")})
    emb = "ijepa.embeddings."
    if emb + "cls_token" in sd:
        raise ValueError(f"{me}: the checkpoint has a class token ({emb}cls_token); the blob of a FLAG_NO_CLS context has none")
    if emb + "position_embeddings" in sd:
        rows = int(np.asarray(sd[emb + "position_embeddings"]).shape[-2])
        if rows != NP:
            raise ValueError(f"{me}: {emb}position_embeddings has {rows} rows, cfg needs NP = {NP} (no class-token row; "
                             "interpolate the table to the image size first)")
    flags = FLAG_NO_CLS | FLAG_POOL(POOL_AVG_NORM)
    top = {"patch.weight": emb + "patch_embeddings.projection.weight", "patch.bias": emb + "patch_embeddings.projection.bias",
           "pos": (emb + "position_embeddings", (1, NP, D)), "lnf.weight": "ijepa.layernorm.weight", "lnf.bias": "ijepa.layernorm.bias"}
    t = _take_named(_taker(sd, me), cfg, flags, top, "ijepa.layers.{}.", _IJEPA_LAYER)
    if head is None and "classifier.weight" in sd and "classifier.bias" in sd:
        head = (sd["classifier.weight"], sd["classifier.bias"])
    t["head.weight"], t["head.bias"] = _head(me, head, E, D)
    return _pack_blob(me, cfg, ln_eps, flags, t)


def blob_from_timm_vit_state_dict(sd, cfg, ln_eps=1e-6, global_pool="token", fc_norm=None):
    """Canonical blob of a timm `VisionTransformer` classifier from a dict of arrays under timm's parameter names: `cls_token`,
    `reg_token`, `pos_embed`, `patch_embed.proj.*`, `blocks.N.{norm1, attn.qkv, attn.proj, ls1.gamma, norm2, mlp.fc1, mlp.fc2,
    ls2.gamma}`, `norm` / `fc_norm`, `head` (numpy only).  NOT run against a timm install (none was at hand): the names and
    the pooling rules are timm's as documented, the test builds the state dict under those names from seeded tensors.
      global_pool 'token' -> POOL_CLS; 'avg' with fc_norm (timm's default for 'avg') -> POOL_AVG_FCNORM, lnf = `fc_norm.*`; 'avg'
      with fc_norm=False -> POOL_AVG_NORM, lnf = `norm.*`.  fc_norm = None means timm's default: global_pool == 'avg'.
      No `cls_token` (class_token=False) -> FLAG_NO_CLS, which needs global_pool 'avg'.  cfg['registers'] = the rows of `reg_token`.
      The fused qkv is split, LayerScale (`ls1.gamma`, `ls2.gamma`; optional) is folded as the DINOv2 converter folds it.
      `pos_embed` has NP or NP + 1 rows, nothing else: with a class token, NP rows mean no_embed_class (the class token's position
      row is zero); without one, NP rows are required.  (Register tokens carry no position row here, as in the library.)
    Refused: a pooling other than 'token' / 'avg', 'token' without a class token, pos_embed rows other than those, a register
    count other than cfg['registers'], a missing or wrongly shaped tensor (by name)."""
    me = "blob_from_timm_vit_state_dict"
    D, M = cfg["dim"], cfg["mlp_dim"]
    NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
    if global_pool not in ("token", "avg"):
        raise ValueError(f"{me}: global_pool = {global_pool!r} is not 'token' or 'avg'")
    if fc_norm is None:
        fc_norm = global_pool == "avg"
    has_cls = "cls_token" in sd
    if not has_cls and global_pool == "token":
        raise ValueError(f"{me}: global_pool='token' needs a cls_token")
    if fc_norm and global_pool != "avg":
        raise ValueError(f"{me}: fc_norm goes with global_pool='avg'")
    pool = POOL_CLS if global_pool == "token" else POOL_AVG_FCNORM if fc_norm else POOL_AVG_NORM
    R = _register_count(me, cfg, sd, "reg_token")
    flags = FLAG_REGISTERS(R) | (0 if has_cls else FLAG_NO_CLS) | FLAG_POOL(pool)
    take = _taker(sd, me)
    if "pos_embed" not in sd:
        raise KeyError(f"{me}: missing tensor pos_embed")
    rows = int(np.asarray(sd["pos_embed"]).shape[-2])
    if rows not in ((NP, NP + 1) if has_cls else (NP,)):
        raise ValueError(f"{me}: pos_embed has {rows} rows, cfg needs " + (f"NP = {NP} or NP + 1 = {NP + 1}" if has_cls else f"NP = {NP}"))
    ln = "fc_norm" if fc_norm else "norm"
    top = {"patch.weight": "patch_embed.proj.weight", "patch.bias": "patch_embed.proj.bias", "cls": ("cls_token", (1, 1, D)),
           "reg": ("reg_token", (1, R, D)), "lnf.weight": ln + ".weight", "lnf.bias": ln + ".bias", "head.weight": "head.weight", "head.bias": "head.bias"}
    t = _take_named(take, cfg, flags, top, "blocks.{}.", _TIMM_LAYER)
    pos = take("pos_embed", (1, rows, D))
    t["pos"] = np.concatenate([np.zeros(D, np.float32), pos]) if has_cls and rows == NP else pos   # no_embed_class: the class token carries no position
    for l in range(cfg["layers"]):
        b = f"blocks.{l}."
        qkv_w, qkv_b = take(b + "attn.qkv.weight", (3 * D, D)).reshape(3, D * D), take(b + "attn.qkv.bias", (3 * D,)).reshape(3, D)
        for i, n in enumerate("qkv"):
            t[f"l{l}.{n}.weight"], t[f"l{l}.{n}.bias"] = qkv_w[i], qkv_b[i]
        t[f"l{l}.o.weight"], t[f"l{l}.o.bias"] = _scaled(take, sd, D, D, b + "attn.proj", b + "ls1.gamma", optional=True)
        t[f"l{l}.fc2.weight"], t[f"l{l}.fc2.bias"] = _scaled(take, sd, D, M, b + "mlp.fc2", b + "ls2.gamma", optional=True)
    return _pack_blob(me, cfg, ln_eps, flags, t)


def device_free_bytes(device=0):
    free, total = C.c_size_t(0), C.c_size_t(0)
    _check(lib().vh_device_mem_info(device, C.byref(free), C.byref(total)))
    return free.value


def input_norm_from_mean_std(mean, std):
    """(scale, shift) for set_input_norm such that a pixel p enters as (p / 255 - mean) / std: scale = 1 / (255 std),
    shift = -mean / std per channel, computed in float64 and rounded once to float32."""
    mean, std = np.atleast_1d(np.asarray(mean, dtype=np.float64)), np.atleast_1d(np.asarray(std, dtype=np.float64))
    if mean.shape != std.shape or mean.ndim != 1 or not (std != 0).all():
        raise ValueError("input_norm_from_mean_std: mean and std are per-channel vectors of one length, std non-zero")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def center_crop_box(h, w, fraction=0.875):
    """The centred square of side fraction * min(h, w) as a box (x0, y0, x1, y1): with the default fraction, what torchvision's
    Resize(256) + CenterCrop(224) keeps of a frame."""
    if h < 1 or w < 1 or not 0.0 < fraction <= 1.0:
        raise ValueError("center_crop_box: h, w >= 1 and 0 < fraction <= 1")
    side = fraction * min(h, w)
    x0, y0 = (w - side) / 2.0, (h - side) / 2.0
    return (x0, y0, x0 + side, y0 + side)


def resize_table(n_in, lo, hi, n_out, max_taps=65):
    """vh_resize_table: (first[n_out] int32, count[n_out] int32, weights[n_out, max_taps] float32) of one axis."""
    first, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, max_taps), np.float32)
    _check(lib().vh_resize_table(n_in, lo, hi, n_out, first.ctypes.data, count.ctypes.data, weights.ctypes.data, max_taps))
    return first, count, weights


def pack_frames(frames, boxes=None, channels=None):
    """A list of HWC (or HW) uint8 arrays -> (one uint8 buffer holding them back to back, the (Frame * n) descriptors).
    boxes: one (x0, y0, x1, y1) per frame, None = the whole frame."""
    frames = [np.asarray(f) for f in frames]
    if boxes is None:
        boxes = [None] * len(frames)
    if not frames or len(boxes) != len(frames):
        raise ValueError("pack_frames: one box (or None) per frame, at least one frame")
    desc = (Frame * len(frames))()
    parts, off = [], 0
    for i, (f, box) in enumerate(zip(frames, boxes)):
        if f.dtype != np.uint8 or f.ndim not in (2, 3):
            raise TypeError(f"pack_frames: frame {i} is not an HWC uint8 array")
        if f.ndim == 2:
            f = f[:, :, None]
        if channels is not None and f.shape[2] != channels:
            raise ValueError(f"pack_frames: frame {i} has {f.shape[2]} channels, the model takes {channels}")
        f = np.ascontiguousarray(f)
        h, w, ch = f.shape
        desc[i].offset, desc[i].height, desc[i].width, desc[i].row_stride = off, h, w, w * ch
        desc[i].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(v) for v in box)
        parts.append(f.reshape(-1))
        off += f.size
    return np.concatenate(parts), desc


def yuv_matrix(standard=YUV_BT709, full_range=False):
    """vh_yuv_matrix: the row-major 3 x 4 float32 matrix (rows R, G, B; columns y, u, v, 1) of a standard and range."""
    m = np.zeros(12, np.float32)
    _check(lib().vh_yuv_matrix(standard, 1 if full_range else 0, m.ctypes.data))
    return m.reshape(3, 4)


def _sample_bytes(a):
    """An array of samples as bytes: 16-bit words little-endian."""
    return np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<")).reshape(-1).view(np.uint8)


def _pack_semi_planar(name, dtype, planes, boxes):
    """The body of pack_frames_nv12 / pack_frames_p016: (Y, UV) pairs of `dtype` samples -> (bytes, (FrameNV12 * n)); offsets and
    strides in bytes."""
    sb, tn = np.dtype(dtype).itemsize, np.dtype(dtype).name
    planes = [(np.asarray(y), np.asarray(uv)) for y, uv in planes]
    if boxes is None:
        boxes = [None] * len(planes)
    if not planes or len(boxes) != len(planes):
        raise ValueError(f"{name}: one box (or None) per frame, at least one frame")
    desc = (FrameNV12 * len(planes))()
    parts, off = [], 0
    for i, ((y, uv), box) in enumerate(zip(planes, boxes)):
        if y.dtype != dtype or uv.dtype != dtype or y.ndim != 2 or uv.ndim != 3 or uv.shape[2] != 2:
            raise TypeError(f"{name}: frame {i} is not a ([H, W], [H/2, W/2, 2]) pair of {tn} arrays")
        h, w = y.shape
        if h % 2 or w % 2 or uv.shape[:2] != (h // 2, w // 2):
            raise ValueError(f"{name}: frame {i}: Y is {h} x {w}, UV is {uv.shape[0]} x {uv.shape[1]} pairs; want even sides and UV of half each")
        desc[i].y_offset, desc[i].uv_offset = off, off + sb * h * w
        desc[i].height, desc[i].width, desc[i].y_stride, desc[i].uv_stride = h, w, sb * w, sb * w
        desc[i].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(v) for v in box)
        parts += [_sample_bytes(y), _sample_bytes(uv)]
        off += sb * (h * w + h * w // 2)
    return np.concatenate(parts), desc


def pack_frames_nv12(planes, boxes=None):
    """A list of (Y [H, W] uint8, UV [H/2, W/2, 2] uint8) pairs -> (one uint8 buffer, the (FrameNV12 * n) descriptors).  Each frame
    lies as a decoder writes it: its Y plane, then its UV plane, rows unpadded (y_stride = uv_stride = W), frames back to back.
    boxes: one (x0, y0, x1, y1) per frame in luma pixels, None = the whole frame."""
    return _pack_semi_planar("pack_frames_nv12", np.uint8, planes, boxes)


def yuv_subsampling(y_shape, u_shape, v_shape):
    """(sub_x, sub_y) of a (Y, U, V) triple of plane shapes under the ceiling rule cw = ceil(W / sub_x), ch = ceil(H / sub_y), or
    ValueError.  Where a side is so short that both factors give the same chroma size (1 -> 1) the answer is 1."""
    (h, w), sub = y_shape, []
    if tuple(u_shape) != tuple(v_shape):
        raise ValueError(f"U is {tuple(u_shape)}, V is {tuple(v_shape)}: the chroma planes differ in size")
    for n, c, name in ((w, u_shape[1], "width"), (h, u_shape[0], "height")):
        s = 1 if c == n else 2 if c == (n + 1) // 2 else 0
        if not s:
            raise ValueError(f"luma {name} {n} with chroma {name} {c}: neither {n} (sub 1) nor {(n + 1) // 2} (sub 2)")
        sub.append(s)
    return sub[0], sub[1]


def _pack_planar(name, dtype, planes, boxes):
    """The body of pack_frames_yuv / pack_frames_yuv16: (Y, U, V) triples of `dtype` samples -> (bytes, (FrameYUV * n)); offsets and
    strides in bytes."""
    sb, tn = np.dtype(dtype).itemsize, np.dtype(dtype).name
    planes = [tuple(np.asarray(p) for p in t) for t in planes]
    if boxes is None:
        boxes = [None] * len(planes)
    if not planes or len(boxes) != len(planes):
        raise ValueError(f"{name}: one box (or None) per frame, at least one frame")
    desc = (FrameYUV * len(planes))()
    parts, off = [], 0
    for i, (t, box) in enumerate(zip(planes, boxes)):
        if len(t) != 3 or any(p.dtype != dtype or p.ndim != 2 or p.size == 0 for p in t):
            raise TypeError(f"{name}: frame {i} is not a (Y, U, V) triple of 2-d {tn} arrays")
        y, u, v = t
        try:
            sx, sy = yuv_subsampling(y.shape, u.shape, v.shape)
        except ValueError as e:
            raise ValueError(f"{name}: frame {i}: {e}") from None
        h, w = y.shape
        ch, cw = u.shape
        d = desc[i]
        d.y_offset, d.u_offset, d.v_offset = off, off + sb * h * w, off + sb * (h * w + ch * cw)
        d.height, d.width, d.y_stride, d.u_stride, d.v_stride, d.sub_x, d.sub_y = h, w, sb * w, sb * cw, sb * cw, sx, sy
        d.box[:] = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(b) for b in box)
        parts += [_sample_bytes(p) for p in (y, u, v)]
        off += sb * (h * w + 2 * ch * cw)
    return np.concatenate(parts), desc


def pack_frames_yuv(planes, boxes=None):
    """A list of (Y [H, W], U [ch, cw], V [ch, cw]) uint8 triples -> (one uint8 buffer, the (FrameYUV * n) descriptors).  The
    sub-sampling of each frame is inferred from the shapes (yuv_subsampling) and an inconsistent triple is refused.  Each frame
    lies as a decoder writes I420: Y, U, V, rows unpadded, frames back to back.  boxes: one (x0, y0, x1, y1) per frame in luma
    pixels, None = the whole frame."""
    return _pack_planar("pack_frames_yuv", np.uint8, planes, boxes)


def yuv_matrix16(standard=YUV_BT709, full_range=False, bits=10, msb_aligned=True):
    """vh_yuv_matrix16: the 3 x 4 float32 matrix for 16-bit words that carry `bits`-bit codes (8..16) in their high bits
    (msb_aligned: P010, P012, P016) or their low bits (yuv420p10le and its kin).  The default is P010 as a hardware decoder
    writes it."""
    m = np.zeros(12, np.float32)
    _check(lib().vh_yuv_matrix16(standard, 1 if full_range else 0, bits, 1 if msb_aligned else 0, m.ctypes.data))
    return m.reshape(3, 4)


def pack_frames_p016(planes, boxes=None):
    """pack_frames_nv12 for 16-bit samples (P010 / P012 / P016): a list of (Y [H, W] uint16, UV [H/2, W/2, 2] uint16) pairs ->
    (one uint8 buffer of little-endian words, the (FrameNV12 * n) descriptors).  Offsets and strides are bytes
    (y_stride = uv_stride = 2 W); width, height and box count samples."""
    return _pack_semi_planar("pack_frames_p016", np.uint16, planes, boxes)


def pack_frames_yuv16(planes, boxes=None):
    """pack_frames_yuv for 16-bit samples (yuv420p10le, yuv422p10le, yuv444p12le, ...): a list of (Y, U, V) uint16 triples -> (one
    uint8 buffer of little-endian words, the (FrameYUV * n) descriptors).  Offsets and strides are bytes; width, height, sub_x,
    sub_y and box count samples."""
    return _pack_planar("pack_frames_yuv16", np.uint16, planes, boxes)


def v210_rows(y, u, v):
    """(Y [H, W], U [H, cw], V [H, cw]) uint16 codes 0..1023, cw = (W + 1) // 2 -> the v210 rows as [H, 4 * ceil(W / 6)] uint32 words:
    twelve codes per block in the order U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5, three per word from bit 0, the unused slots of the
    last block zero."""
    y, u, v = (np.asarray(p).astype(np.uint32) for p in (y, u, v))
    h, w = y.shape
    cw = (w + 1) // 2
    if u.shape != (h, cw) or v.shape != (h, cw):
        raise ValueError(f"v210_rows: Y is {h} x {w}, U is {u.shape}, V is {v.shape}; want chroma planes of {h} x {cw}")
    if max(int(y.max()), int(u.max()), int(v.max())) > 1023:
        raise ValueError("v210_rows: a code is above 1023")
    blocks = (w + 5) // 6
    slots = np.zeros((h, 12 * blocks), np.uint32)
    slots[:, 1:2 * w:2] = y
    slots[:, 0:4 * cw:4] = u
    slots[:, 2:4 * cw:4] = v
    s3 = slots.reshape(h, 4 * blocks, 3)
    return s3[:, :, 0] | (s3[:, :, 1] << np.uint32(10)) | (s3[:, :, 2] << np.uint32(20))


def pack_frames_yuy2(planes, layouts=L422_YUYV, boxes=None):
    """A list of (Y [H, W], U [H, cw], V [H, cw]) triples, cw = (W + 1) // 2, interleaved into packed 4:2:2 frames -> (one uint8
    buffer, the (FrameYUY2 * n) descriptors).  layouts: one L422_* for all frames or one per frame.  uint8 planes give the 8-bit
    layouts (forward_frames_yuy2); uint16 planes give Y210 / Y216 words in the order of the layout, or, with L422_V210, v210 blocks
    of the 10-bit codes in the planes (forward_frames_y210).  Rows are unpadded, frames back to back, each v210 frame 4-byte and
    each 16-bit frame 8-byte aligned by construction.  With an odd width the second luma of the last macropixel is zero."""
    planes = [tuple(np.asarray(p) for p in t) for t in planes]
    if isinstance(layouts, int):
        layouts = [layouts] * len(planes)
    if boxes is None:
        boxes = [None] * len(planes)
    if not planes or len(boxes) != len(planes) or len(layouts) != len(planes):
        raise ValueError("pack_frames_yuy2: one layout and one box (or None) per frame, at least one frame")
    dtype = planes[0][0].dtype
    if dtype not in (np.uint8, np.uint16):
        raise TypeError("pack_frames_yuy2: planes must be uint8 or uint16 arrays")
    desc = (FrameYUY2 * len(planes))()
    parts, off = [], 0
    for i, (t, lay, box) in enumerate(zip(planes, layouts, boxes)):
        if len(t) != 3 or any(p.dtype != dtype or p.ndim != 2 or p.size == 0 for p in t):
            raise TypeError(f"pack_frames_yuy2: frame {i} is not a (Y, U, V) triple of 2-d {np.dtype(dtype).name} arrays")
        y, u, v = t
        h, w = y.shape
        cw = (w + 1) // 2
        if u.shape != (h, cw) or v.shape != (h, cw):
            raise ValueError(f"pack_frames_yuy2: frame {i}: Y is {h} x {w}, chroma is {u.shape} / {v.shape}; want {h} x {cw} (4:2:2)")
        if lay == L422_V210:
            if dtype != np.uint16:
                raise ValueError(f"pack_frames_yuy2: frame {i}: L422_V210 takes uint16 planes of 10-bit codes")
            rows = _sample_bytes(v210_rows(y, u, v))
        elif lay in (L422_YUYV, L422_UYVY, L422_YVYU, L422_VYUY):
            m = np.zeros((h, cw, 4), dtype)
            ypos, upos = lay & 1, (lay ^ 1) & 3
            m[:, :(w + 1) // 2, ypos] = y[:, 0::2]
            m[:, :w // 2, ypos + 2] = y[:, 1::2]
            m[:, :, upos] = u
            m[:, :, upos ^ 2] = v
            rows = _sample_bytes(m)
        else:
            raise ValueError(f"pack_frames_yuy2: frame {i}: layout {lay} is none of L422_*")
        d = desc[i]
        d.offset, d.height, d.width, d.row_stride, d.layout = off, h, w, rows.size // h, lay
        d.box[:] = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(b) for b in box)
        parts.append(rows)
        off += rows.size
    return np.concatenate(parts), desc


def word10_rows(c0, c1, c2, layout):
    """Three [H, W] arrays of 10-bit codes (Y, U, V) -> the Y410 / V410 rows as [H, W] uint32 words: component k at bits
    10 p_k .. 10 p_k + 9 (V410: two bits higher), the other bits zero."""
    comps = [np.asarray(p).astype(np.uint32) for p in (c0, c1, c2)]
    if max(int(p.max()) for p in comps) > 1023:
        raise ValueError("word10_rows: a code is above 1023")
    lsb = 2 if layout & 512 else 0
    word = np.zeros(comps[0].shape, np.uint32)
    for k, p in enumerate(comps):
        word |= p << np.uint32(10 * ((layout >> (2 * k)) & 3) + lsb)
    return word


def pack_frames_bgra(planes_or_pixels, layouts=L444_BGRA, boxes=None):
    """A list of frames, each an [H, W, 3] array or a triple of [H, W] planes whose components are in OUTPUT order (R, G, B, or
    Y, U, V for a layout with the yuv bit), interleaved into packed 4:4:4 frames -> (one uint8 buffer, the (FrameBGRA * n)
    descriptors).  layouts: one L444_* for all frames or one per frame.  uint8 samples give the 8-bit layouts (forward_frames_bgra);
    uint16 samples give four 16-bit words per pixel, or, with L444_Y410 / L444_V410, one 32-bit word of the 10-bit codes in the
    arrays (forward_frames_y410).  The 4th sample is 0xff.. .  Rows are unpadded, frames back to back: 16-bit frames are 8-byte and
    10-bit frames 4-byte aligned by construction."""
    frames = [np.stack([np.asarray(p) for p in t], axis=-1) if isinstance(t, (tuple, list)) else np.asarray(t) for t in planes_or_pixels]
    if isinstance(layouts, int):
        layouts = [layouts] * len(frames)
    if boxes is None:
        boxes = [None] * len(frames)
    if not frames or len(boxes) != len(frames) or len(layouts) != len(frames):
        raise ValueError("pack_frames_bgra: one layout and one box (or None) per frame, at least one frame")
    dtype = frames[0].dtype
    if dtype not in (np.uint8, np.uint16):
        raise TypeError("pack_frames_bgra: samples must be uint8 or uint16")
    desc = (FrameBGRA * len(frames))()
    parts, off = [], 0
    for i, (px, lay, box) in enumerate(zip(frames, layouts, boxes)):
        if px.dtype != dtype or px.ndim != 3 or px.shape[2] != 3 or px.size == 0:
            raise TypeError(f"pack_frames_bgra: frame {i} is not [H, W, 3] {np.dtype(dtype).name} samples (or three [H, W] planes)")
        h, w = px.shape[:2]
        pos = [(lay >> (2 * k)) & 3 for k in range(3)]
        if lay & 256:
            if dtype != np.uint16 or lay not in (L444_Y410, L444_V410):
                raise ValueError(f"pack_frames_bgra: frame {i}: a 10-bit layout is L444_Y410 or L444_V410 and takes uint16 codes")
            rows = _sample_bytes(word10_rows(px[..., 0], px[..., 1], px[..., 2], lay))
        else:
            ns = 4 if lay & 64 else 3
            if lay < 0 or lay > 255 or max(pos) >= ns:
                raise ValueError(f"pack_frames_bgra: frame {i}: layout {lay} is no VH_444 word")
            m = np.full((h, w, ns), np.iinfo(dtype).max, dtype)
            for k in range(3):
                m[:, :, pos[k]] = px[..., k]
            rows = _sample_bytes(m)
        d = desc[i]
        d.offset, d.height, d.width, d.row_stride, d.layout = off, h, w, rows.size // h, lay
        d.box[:] = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(b) for b in box)
        parts.append(rows)
        off += rows.size
    return np.concatenate(parts), desc


def make_config(cfg, dtype=DTYPE_BF16, max_batch=1, ln_eps=1e-6, flags=0):
    """vh_config of a model dict.  cfg.get("registers", 0) register tokens are folded into `flags`; a caller may put
    FLAG_REGISTERS(n) into `flags` itself instead (both, with different counts, is refused)."""
    r = int(cfg.get("registers", 0))
    if not 0 <= r <= 31:
        raise ValueError(f"make_config: cfg['registers'] = {r} is outside 0 .. 31 (the library takes 0 .. {MAX_REGISTERS})")
    if r and registers_of(flags) not in (0, r):
        raise ValueError(f"make_config: cfg['registers'] = {r} but flags carry FLAG_REGISTERS({registers_of(flags)})")
    flags |= FLAG_REGISTERS(r)
    return Config(cfg["image_size"], cfg["patch_size"], cfg["channels"], cfg["dim"], cfg["heads"],
                  cfg["mlp_dim"], cfg["layers"], cfg["classes"], dtype, max_batch, ln_eps, flags)


# ---- 16-bit helpers (host side, for building operator inputs / reading operator outputs) -------
def to_bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (r >> np.uint32(16)).astype(np.uint16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def to16(a, dtype):
    return to_bf16_bits(a) if dtype == DTYPE_BF16 else np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def from16(b, dtype):
    return from_bf16_bits(b) if dtype == DTYPE_BF16 else np.ascontiguousarray(b, dtype=np.uint16).view(np.float16).astype(np.float32)


# ---- the layouts q|k|v and the attention output take between the projections (test taps) ----
def pack_head_major(qkv, heads, hm_rows, fill=0):
    """Row-major q|k|v [rows][3 * heads * 64] (any element type) -> head-major [3][heads][hm_rows][64]; rows beyond the
    input's (hm_rows > rows: the padding of the persistent projection's row tiles) hold `fill`."""
    qkv = np.ascontiguousarray(qkv)
    rows = qkv.shape[0]
    assert qkv.shape[1] == 3 * heads * 64 and hm_rows >= rows
    out = np.full((3, heads, hm_rows, 64), fill, dtype=qkv.dtype)
    out[:, :, :rows] = qkv.reshape(rows, 3, heads, 64).transpose(1, 2, 0, 3)
    return out


def unpack_tiled(tiled, rows, dim, chunk=8):
    """The 16-row-blocked layout [ceil(rows / 16)][dim / chunk][16 rows][chunk] -> row-major [rows][dim].  chunk = elements per
    16-byte piece: 8 for 2-byte elements, 16 for e4m3 bytes (what launch_tile_bytes writes for weights)."""
    nb = (rows + 15) // 16
    t = np.ascontiguousarray(tiled).reshape(nb, dim // chunk, 16, chunk)
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3).reshape(nb * 16, dim)[:rows])


def pack_tiled(a, chunk=8, fill=0):
    """Inverse of unpack_tiled: row-major [rows][dim] -> [ceil(rows / 16)][dim / chunk][16][chunk]; the rows that pad the last
    block hold `fill`."""
    a = np.ascontiguousarray(a)
    rows, dim = a.shape
    assert dim % chunk == 0
    nb = (rows + 15) // 16
    full = np.full((nb * 16, dim), fill, dtype=a.dtype)
    full[:rows] = a
    return np.ascontiguousarray(full.reshape(nb, 16, dim // chunk, chunk).transpose(0, 2, 1, 3))


# numpy dtype -> ELEM_* (bf16 has no numpy dtype: uint16 bits with elem=ELEM_BF16 given)
_NUMPY_ELEM = {np.dtype(np.float32): ELEM_F32, np.dtype(np.float16): ELEM_F16, np.dtype(np.uint8): ELEM_U8}


class DeviceBuffer:
    """A raw HBM allocation owned through vh_malloc/vh_free."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        _check(lib().vh_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, device)
        _check(lib().vh_memcpy_h2d(device, b.ptr, a.ctypes.data, a.nbytes))
        return b

    def to_numpy(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _check(lib().vh_memcpy_d2h(self.device, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().vh_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


FILTER_BLUR3, FILTER_SOBEL3 = 0, 1


class FilterPipeline:
    """vh_filter wrapper: the filter_image / get_filtered_image ring."""

    def __init__(self, height, width, slots=24, kind=FILTER_BLUR3, device=0):
        self.shape = (height, width)
        h = C.c_void_p()
        _check(lib().vh_filter_create(device, height, width, slots, kind, C.byref(h)))
        self.h = h.value

    def _chk(self, rc):
        if rc != 0:
            raise VhError(rc, lib().vh_filter_last_error(self.h).decode())

    def free_slots(self):
        n = C.c_int(0)
        self._chk(lib().vh_filter_free_slots(self.h, C.byref(n)))
        return n.value

    def submit(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        assert frame.shape == self.shape
        self._chk(lib().vh_filter_submit(self.h, frame.ctypes.data))

    def collect(self):
        out = np.empty(self.shape, dtype=np.uint8)
        self._chk(lib().vh_filter_collect(self.h, out.ctypes.data))
        return out

    def close(self):
        if self.h:
            lib().vh_filter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VitContext:
    """vh_ctx wrapper: create / load weights / forward, mirroring hip::net_hip's ViT mode."""

    def __init__(self, cfg, dtype=DTYPE_BF16, max_batch=1, device=0, ln_eps=1e-6, flags=0):
        self.cfg, self.dtype, self.device = dict(cfg), dtype, device
        self.c = make_config(cfg, dtype, max_batch, ln_eps, flags)
        h = C.c_void_p()
        _check(lib().vh_create(C.byref(self.c), device, C.byref(h)))
        self.h = h.value
        self._ring_batch = 0

    def close(self):
        if self.h:
            lib().vh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def blob_bytes(self):
        return lib().vh_weight_blob_bytes(C.byref(self.c))

    def ln_fold(self):
        """True when this context folds its LayerNorms into the GEMMs (vh_config.flags, model shape, dtype)."""
        on = C.c_int(0)
        _check(lib().vh_get_ln_fold(self.h, C.byref(on)), self.h)
        return bool(on.value)

    def ln_guard(self):
        """(max |row mean| / sigma seen since the weights were loaded, threshold, tripped) -- the fold's run-time guard."""
        r, t, trip = C.c_float(0), C.c_float(0), C.c_int(0)
        _check(lib().vh_get_ln_guard(self.h, C.byref(r), C.byref(t), C.byref(trip)), self.h)
        return r.value, t.value, bool(trip.value)

    def fp8_guard(self):
        """(largest |x| bound seen on the raw residual rows of an fp8 context, e4m3's limit 448)."""
        a, lim = C.c_float(0), C.c_float(0)
        _check(lib().vh_get_fp8_guard(self.h, C.byref(a), C.byref(lim)), self.h)
        return a.value, lim.value

    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(lib().vh_load_weights(self.h, blob.ctypes.data, blob.nbytes), self.h)

    def load_weights_device(self, ptr, nbytes):
        _check(lib().vh_load_weights_device(self.h, ptr, nbytes), self.h)

    def init_weights_seeded(self, seed):
        _check(lib().vh_init_weights_seeded(self.h, seed), self.h)

    def export_weights(self):
        out = np.empty(self.blob_bytes, dtype=np.uint8)
        _check(lib().vh_export_weights(self.h, out.ctypes.data, out.nbytes), self.h)
        return out

    def export_weights_device(self, ptr, nbytes):
        _check(lib().vh_export_weights_device(self.h, ptr, nbytes), self.h)

    def save_weights_file(self, path):
        _check(lib().vh_save_weights_file(self.h, os.fsencode(path)), self.h)

    def load_weights_file(self, path):
        _check(lib().vh_load_weights_file(self.h, os.fsencode(path)), self.h)

    def forward(self, images):
        """images: [B, H, W, C] fp32 (host).  Returns [B, classes] fp32 logits."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        b = images.shape[0]
        out = np.empty((b, self.cfg["classes"]), dtype=np.float32)
        _check(lib().vh_forward(self.h, images.ctypes.data, b, out.ctypes.data), self.h)
        return out

    def forward_device(self, in_ptr, batch, out_ptr):
        _check(lib().vh_forward_device(self.h, in_ptr, batch, out_ptr), self.h)

    def forward_device_async(self, in_ptr, batch, out_ptr, steps=1):
        _check(lib().vh_forward_device_async(self.h, in_ptr, batch, out_ptr, steps), self.h)

    def synchronize(self):
        _check(lib().vh_synchronize(self.h), self.h)

    # ---- 8-bit images: pixel p of channel c enters as fmaf(float(p), scale[c], shift[c]), one rounding ----
    def set_input_norm(self, scale=None, shift=None):
        """Per-channel constants of the u8 entry points ([channels] each; None, None = the default 1/255, 0)."""
        if scale is None and shift is None:
            _check(lib().vh_set_input_norm(self.h, None, None), self.h)
            return
        ch = self.cfg["channels"]
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32).reshape(-1)
        for a in (sc, sh):
            if a is not None and a.size != ch:
                raise ValueError(f"set_input_norm: expected {ch} values per array, got {a.size}")
        _check(lib().vh_set_input_norm(self.h, None if sc is None else sc.ctypes.data, None if sh is None else sh.ctypes.data), self.h)

    def get_input_norm(self):
        ch = self.cfg["channels"]
        sc, sh = np.empty(ch, dtype=np.float32), np.empty(ch, dtype=np.float32)
        _check(lib().vh_get_input_norm(self.h, sc.ctypes.data, sh.ctypes.data), self.h)
        return sc, sh

    def forward_u8(self, images):
        """images: [B, H, W, C] uint8 (host).  Returns [B, classes] fp32 logits: the bits forward() gives for the fp32 array
        fmaf(p, scale[c], shift[c])."""
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise TypeError(f"forward_u8 takes uint8 images, got {images.dtype}")
        images = np.ascontiguousarray(images)
        b = images.shape[0]
        out = np.empty((b, self.cfg["classes"]), dtype=np.float32)
        _check(lib().vh_forward_u8(self.h, images.ctypes.data, b, out.ctypes.data), self.h)
        return out

    def forward_device_u8(self, in_ptr, batch, out_ptr):
        _check(lib().vh_forward_device_u8(self.h, in_ptr, batch, out_ptr), self.h)

    def forward_device_u8_async(self, in_ptr, batch, out_ptr, steps=1):
        _check(lib().vh_forward_device_u8_async(self.h, in_ptr, batch, out_ptr, steps), self.h)

    # ---- image tensors: one element type (ELEM_*) and one layout (LAYOUT_*), taken as they are ----
    def forward_tensor(self, array, layout, elem=None):
        """array: a dense host batch, [B, S, S, C] for LAYOUT_NHWC or [B, C, S, S] for LAYOUT_NCHW, of dtype float32, float16 or
        uint8 (elem inferred), or uint16 holding bf16 bits with elem=ELEM_BF16 given.  Returns [B, classes] fp32 logits: the
        bits forward() gives for the NHWC fp32 array of the widened (uint8: normalised, set_input_norm) elements."""
        array = np.asarray(array)
        if elem is None:
            elem = _NUMPY_ELEM.get(array.dtype)
            if elem is None:
                raise TypeError(f"forward_tensor takes float32, float16 or uint8 arrays, or uint16 with elem=ELEM_BF16; got {array.dtype}")
        elif elem in ELEM_BYTES and array.dtype.itemsize != ELEM_BYTES[elem]:
            raise TypeError(f"forward_tensor: elem {elem} has {ELEM_BYTES[elem]} bytes per element, {array.dtype} has {array.dtype.itemsize}")
        array = np.ascontiguousarray(array)
        b = array.shape[0]
        out = np.empty((b, self.cfg["classes"]), dtype=np.float32)
        _check(lib().vh_forward_tensor(self.h, array.ctypes.data, elem, layout, b, out.ctypes.data), self.h)
        return out

    def forward_device_tensor(self, in_ptr, elem, layout, batch, out_ptr):
        _check(lib().vh_forward_device_tensor(self.h, in_ptr, elem, layout, batch, out_ptr), self.h)

    def forward_device_tensor_async(self, in_ptr, elem, layout, batch, out_ptr, steps=1):
        _check(lib().vh_forward_device_tensor_async(self.h, in_ptr, elem, layout, batch, out_ptr, steps), self.h)

    def forward_torch(self, x):
        """x: a torch tensor [B, C, S, S] of dtype float32, float16, bfloat16 or uint8.  A contiguous tensor goes in as NCHW, a
        channels_last one as NHWC of the same memory; any other striding is made dense with .contiguous() first (one copy).
        A tensor on this context's GPU is read in place through data_ptr(), after torch.cuda.current_stream(x.device) has been
        synchronised (the context runs on its own stream), and the logits come back as a torch.float32 tensor on that device.
        A CPU tensor takes the host entry point and returns a CPU tensor; a tensor on another GPU raises ValueError.
        For GPU tensors import torch before this module loads libvithip.so (one HIP runtime per process), and
        mind that the library wants data_ptr() 16-byte aligned (a view with a storage offset may not be)."""
        import torch
        elems = {torch.float32: ELEM_F32, torch.float16: ELEM_F16, torch.bfloat16: ELEM_BF16, torch.uint8: ELEM_U8}
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise TypeError("forward_torch takes a 4-d torch tensor [B, C, S, S]")
        if x.dtype not in elems:
            raise TypeError(f"forward_torch takes float32, float16, bfloat16 or uint8 tensors, got {x.dtype}")
        elem = elems[x.dtype]
        if x.is_contiguous():
            layout = LAYOUT_NCHW
        elif x.is_contiguous(memory_format=torch.channels_last):
            layout = LAYOUT_NHWC
        else:
            x, layout = x.contiguous(), LAYOUT_NCHW
        b = x.shape[0]
        out = torch.empty((b, self.cfg["classes"]), dtype=torch.float32, device=x.device)
        if x.device.type == "cpu":
            _check(lib().vh_forward_tensor(self.h, x.data_ptr(), elem, layout, b, out.data_ptr()), self.h)
            return out
        if x.device.type != "cuda" or x.device.index != self.device:
            raise ValueError(f"forward_torch: the tensor lives on {x.device}, this context on GPU {self.device}")
        torch.cuda.current_stream(x.device).synchronize()   # x is complete (and `out` allocated) before the context's stream reads it
        _check(lib().vh_forward_device_tensor(self.h, x.data_ptr(), elem, layout, b, out.data_ptr()), self.h)
        return out

    # ---- frames of any format: one body per job; `fn` is the format's C entry point, `desc` its descriptor array ----
    def _forward_frames_host(self, fn, buf, desc):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        out = np.empty((len(desc), self.cfg["classes"]), dtype=np.float32)
        _check(fn(self.h, buf.ctypes.data, buf.nbytes, C.addressof(desc), len(desc), out.ctypes.data), self.h)
        return out

    def _forward_frames_device(self, fn, frames_ptr, nbytes, desc, out_ptr):
        _check(fn(self.h, frames_ptr, nbytes, C.addressof(desc), len(desc), out_ptr), self.h)

    def _ring_submit_frames(self, fn, buf, nbytes, desc):
        ptr = None
        if buf is not None:
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            ptr = buf.ctypes.data
        _check(fn(self.h, ptr, nbytes, C.addressof(desc), len(desc)), self.h)

    def _set_colour(self, name, fn, m, chroma_site):
        if m is None:
            _check(fn(self.h, None, 0), self.h)
            return
        m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
        if m.size != 12:
            raise ValueError(f"{name}: expected 12 values, got {m.size}")
        _check(fn(self.h, m.ctypes.data, chroma_site), self.h)

    def _get_colour(self, fn):
        m, site = np.empty(12, np.float32), C.c_int(0)
        _check(fn(self.h, m.ctypes.data, C.byref(site)), self.h)
        return m.reshape(3, 4), site.value

    # ---- 8-bit frames of any size: antialiased resize + crop on the GPU, then forward_u8 of the result ----
    def forward_frames(self, frames, boxes=None):
        """frames: a list of HWC uint8 arrays, any sizes; boxes: one (x0, y0, x1, y1) per frame in source pixels (None = the
        whole frame).  Returns [len(frames), classes] fp32 logits: the bits forward_u8 gives for op_resize_u8's output."""
        buf, desc = pack_frames(frames, boxes, self.cfg["channels"])
        return self.forward_frames_packed(buf, desc)

    def forward_frames_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_u8, buf, desc)

    def forward_device_frames_u8(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_u8, frames_ptr, nbytes, desc, out_ptr)

    # ---- NV12 video frames: both planes resized and the colour matrix applied on the GPU, then forward_u8 of the result ----
    def set_frame_colour(self, m=None, chroma_site=CHROMA_LEFT):
        """m: 12 floats (row-major 3 x 4, see yuv_matrix); None restores the default, BT.709 limited range with left siting."""
        self._set_colour("set_frame_colour", lib().vh_set_frame_colour, m, chroma_site)

    def get_frame_colour(self):
        return self._get_colour(lib().vh_get_frame_colour)

    def forward_frames_nv12(self, planes, boxes=None):
        """planes: a list of (Y [H, W], UV [H/2, W/2, 2]) uint8 pairs, any even sizes; boxes as forward_frames, in luma pixels.
        Returns [len(planes), classes] fp32 logits: the bits forward_u8 gives for op_resize_nv12's output."""
        buf, desc = pack_frames_nv12(planes, boxes)
        return self.forward_frames_nv12_packed(buf, desc)

    def forward_frames_nv12_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_nv12, buf, desc)

    def forward_device_frames_nv12(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_nv12, frames_ptr, nbytes, desc, out_ptr)

    # ---- planar YUV frames (I420 / YV12, JPEG's 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 planes): the same, from three planes ----
    def forward_frames_yuv(self, planes, boxes=None):
        """planes: a list of (Y [H, W], U [ch, cw], V [ch, cw]) uint8 triples, any sizes and sub-samplings; boxes as
        forward_frames, in luma pixels.  The colour matrix and siting are set_frame_colour's (a JPEG caller sets
        yuv_matrix(YUV_BT601, True) with CHROMA_CENTER).  Returns the bits forward_u8 gives for op_resize_yuv's output."""
        buf, desc = pack_frames_yuv(planes, boxes)
        return self.forward_frames_yuv_packed(buf, desc)

    def forward_frames_yuv_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_yuv, buf, desc)

    def forward_device_frames_yuv(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_yuv, frames_ptr, nbytes, desc, out_ptr)

    # ---- 16-bit YUV frames (P010 / P012 / P016 and planar yuv4xxpNNle): the same again, with a colour state of their own ----
    def set_frame_colour16(self, m=None, chroma_site=CHROMA_LEFT):
        """The colour state of the 16-bit entry points.  m: 12 floats (see yuv_matrix16); None restores the default, BT.709 limited
        range, 10 bits, MSB-aligned (P010), left siting.  set_frame_colour's state is not touched."""
        self._set_colour("set_frame_colour16", lib().vh_set_frame_colour16, m, chroma_site)

    def get_frame_colour16(self):
        return self._get_colour(lib().vh_get_frame_colour16)

    def forward_frames_p016(self, planes, boxes=None):
        """planes: a list of (Y [H, W], UV [H/2, W/2, 2]) uint16 pairs (P010 / P012 / P016 words), any even sizes.  Returns the
        bits forward_u8 gives for op_resize_p016's output under set_frame_colour16's state."""
        buf, desc = pack_frames_p016(planes, boxes)
        return self.forward_frames_p016_packed(buf, desc)

    def forward_frames_p016_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_p016, buf, desc)

    def forward_device_frames_p016(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_p016, frames_ptr, nbytes, desc, out_ptr)

    def forward_frames_yuv16(self, planes, boxes=None):
        """planes: a list of (Y [H, W], U [ch, cw], V [ch, cw]) uint16 triples, any sizes and sub-samplings.  Returns the bits
        forward_u8 gives for op_resize_yuv16's output under set_frame_colour16's state (a yuv420p10le caller sets
        yuv_matrix16(bits=10, msb_aligned=False))."""
        buf, desc = pack_frames_yuv16(planes, boxes)
        return self.forward_frames_yuv16_packed(buf, desc)

    def forward_frames_yuv16_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_yuv16, buf, desc)

    def forward_device_frames_yuv16(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_yuv16, frames_ptr, nbytes, desc, out_ptr)

    # ---- packed 4:2:2 frames (YUY2 / UYVY / YVYU / VYUY; Y210 / Y216 / v210): the planar 4:2:2 arithmetic on interleaved memory ----
    def forward_frames_yuy2(self, planes, layouts=L422_YUYV, boxes=None):
        """planes: a list of (Y [H, W], U [H, cw], V [H, cw]) uint8 triples, interleaved here (pack_frames_yuy2) in the order of
        `layouts`.  Returns the bits forward_u8 gives for op_resize_yuy2's output under set_frame_colour's state."""
        buf, desc = pack_frames_yuy2(planes, layouts, boxes)
        return self.forward_frames_yuy2_packed(buf, desc)

    def forward_frames_yuy2_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_yuy2, buf, desc)

    def forward_device_frames_yuy2(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_yuy2, frames_ptr, nbytes, desc, out_ptr)

    def forward_frames_y210(self, planes, layouts=L422_YUYV, boxes=None):
        """planes: uint16 triples as above: Y210 / Y216 words, or 10-bit codes with L422_V210.  Returns the bits forward_u8 gives
        for op_resize_y210's output under set_frame_colour16's state."""
        buf, desc = pack_frames_yuy2(planes, layouts, boxes)
        return self.forward_frames_y210_packed(buf, desc)

    def forward_frames_y210_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_y210, buf, desc)

    def forward_device_frames_y210(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_y210, frames_ptr, nbytes, desc, out_ptr)

    # ---- packed 4:4:4 frames (BGR / BGRA / RGBA / ARGB, YUV24 / VUYA / AYUV; Y416 / AYUV64 / Y410 / V410) ----
    def forward_frames_bgra(self, pixels, layouts=L444_BGRA, boxes=None):
        """pixels: a list of [H, W, 3] uint8 frames (or plane triples) in output order, interleaved here (pack_frames_bgra) as
        `layouts` say.  Returns the bits forward_u8 gives for op_resize_bgra's output under set_frame_colour's matrix."""
        buf, desc = pack_frames_bgra(pixels, layouts, boxes)
        return self.forward_frames_bgra_packed(buf, desc)

    def forward_frames_bgra_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_bgra, buf, desc)

    def forward_device_frames_bgra(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_bgra, frames_ptr, nbytes, desc, out_ptr)

    def forward_frames_y410(self, pixels, layouts=L444_Y410, boxes=None):
        """pixels: uint16 frames as above: 16-bit words, or 10-bit codes with L444_Y410 / L444_V410.  Returns the bits forward_u8
        gives for op_resize_y410's output under set_frame_colour16's matrix."""
        buf, desc = pack_frames_bgra(pixels, layouts, boxes)
        return self.forward_frames_y410_packed(buf, desc)

    def forward_frames_y410_packed(self, buf, desc):
        return self._forward_frames_host(lib().vh_forward_frames_y410, buf, desc)

    def forward_device_frames_y410(self, frames_ptr, nbytes, desc, out_ptr):
        self._forward_frames_device(lib().vh_forward_device_frames_y410, frames_ptr, nbytes, desc, out_ptr)

    def fill_input_seeded(self, seed, batch, in_ptr):
        _check(lib().vh_fill_input_seeded(self.h, seed, batch, in_ptr), self.h)

    def last_forward_us(self):
        v = C.c_int64(0)
        _check(lib().vh_last_forward_us(self.h, C.byref(v)), self.h)
        return v.value

    def last_kernel_ms(self):
        v = C.c_double(0)
        _check(lib().vh_last_kernel_ms(self.h, C.byref(v)), self.h)
        return v.value

    def profile_forward(self, in_ptr, batch, out_ptr):
        n = len(STAGES)
        arr = (C.c_double * (2 * n))()
        nw = C.c_int(0)
        _check(lib().vh_profile_forward(self.h, in_ptr, batch, out_ptr, arr, 2 * n, C.byref(nw)), self.h)
        return {STAGES[i]: (arr[i], int(arr[n + i])) for i in range(n)}

    # ---- pipelined host path (ring of in-flight batches) ----
    def ring_create(self, slots, batch_per_slot, u8=False):
        """u8=True: the slots stage 8-bit images (ring_input_u8 / ring_submit_u8); a quarter of the staging memory."""
        _check((lib().vh_ring_create_u8 if u8 else lib().vh_ring_create)(self.h, slots, batch_per_slot), self.h)
        self._ring_batch = batch_per_slot

    def ring_create_u8(self, slots, batch_per_slot):
        self.ring_create(slots, batch_per_slot, u8=True)

    def ring_input_u8(self, batch):
        """numpy uint8 view of the pinned staging buffer the next ring_submit_u8 will use."""
        p = C.POINTER(C.c_uint8)()
        _check(lib().vh_ring_input_u8(self.h, C.byref(p)), self.h)
        n = batch * self.cfg["image_size"] ** 2 * self.cfg["channels"]
        return np.ctypeslib.as_array(p, shape=(n,)).reshape(batch, self.cfg["image_size"], self.cfg["image_size"], self.cfg["channels"])

    def ring_submit_u8(self, images=None, batch=None):
        if images is None:
            _check(lib().vh_ring_submit_u8(self.h, None, batch), self.h)
            return
        images = np.asarray(images)
        if images.dtype != np.uint8:
            raise TypeError(f"ring_submit_u8 takes uint8 images, got {images.dtype}")
        images = np.ascontiguousarray(images)
        _check(lib().vh_ring_submit_u8(self.h, images.ctypes.data, images.shape[0]), self.h)

    def ring_create_tensor(self, slots, batch_per_slot, elem, layout):
        """A ring whose slots stage image tensors of one element type and layout (ring_input_tensor / ring_submit_tensor)."""
        _check(lib().vh_ring_create_tensor(self.h, slots, batch_per_slot, elem, layout), self.h)
        self._ring_batch = batch_per_slot

    def ring_input_tensor(self):
        """numpy uint8 view (the whole slot: batch_per_slot * S * S * C * sizeof(element) bytes) of the pinned staging buffer the
        next ring_submit_tensor will upload; .view() it as the element type."""
        p, cap = C.c_void_p(), C.c_size_t(0)
        _check(lib().vh_ring_input_tensor(self.h, C.byref(p), C.byref(cap)), self.h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cap.value,))

    def ring_submit_tensor(self, array=None, batch=None):
        """array: a dense host batch of the ring's element type and layout; None: the slot's pinned buffer already holds `batch` images."""
        if array is None:
            _check(lib().vh_ring_submit_tensor(self.h, None, batch), self.h)
            return
        array = np.ascontiguousarray(array)
        _check(lib().vh_ring_submit_tensor(self.h, array.ctypes.data, array.shape[0]), self.h)

    def ring_create_frames(self, slots, batch_per_slot, slot_bytes):
        """A ring whose slots stage up to slot_bytes of 8-bit frames each (ring_input_frames / ring_submit_frames)."""
        _check(lib().vh_ring_create_frames(self.h, slots, batch_per_slot, slot_bytes), self.h)
        self._ring_batch = batch_per_slot

    def ring_input_frames(self):
        """numpy uint8 view (all slot_bytes) of the pinned staging buffer the next ring_submit_frames will upload."""
        p, cap = C.POINTER(C.c_uint8)(), C.c_size_t(0)
        _check(lib().vh_ring_input_frames(self.h, C.byref(p), C.byref(cap)), self.h)
        return np.ctypeslib.as_array(p, shape=(cap.value,))

    def ring_submit_frames(self, frames, boxes=None):
        buf, desc = pack_frames(frames, boxes, self.cfg["channels"])
        self.ring_submit_frames_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of frames that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames, buf, nbytes, desc)

    def ring_submit_frames_nv12(self, planes, boxes=None):
        """NV12 frames into the next slot of a frames ring (ring_create_frames); RGB and NV12 submits may alternate."""
        buf, desc = pack_frames_nv12(planes, boxes)
        self.ring_submit_frames_nv12_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_nv12_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of planes that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_nv12, buf, nbytes, desc)

    def ring_submit_frames_yuv(self, planes, boxes=None):
        """Planar YUV frames into the next slot of a frames ring; RGB, NV12 and planar submits may alternate."""
        buf, desc = pack_frames_yuv(planes, boxes)
        self.ring_submit_frames_yuv_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_yuv_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of planes that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_yuv, buf, nbytes, desc)

    def ring_submit_frames_p016(self, planes, boxes=None):
        """P010 / P012 / P016 frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_p016(planes, boxes)
        self.ring_submit_frames_p016_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_p016_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of planes that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_p016, buf, nbytes, desc)

    def ring_submit_frames_yuv16(self, planes, boxes=None):
        """Planar 16-bit YUV frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_yuv16(planes, boxes)
        self.ring_submit_frames_yuv16_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_yuv16_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of planes that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_yuv16, buf, nbytes, desc)

    def ring_submit_frames_yuy2(self, planes, layouts=L422_YUYV, boxes=None):
        """8-bit packed 4:2:2 frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_yuy2(planes, layouts, boxes)
        self.ring_submit_frames_yuy2_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_yuy2_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of frames that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_yuy2, buf, nbytes, desc)

    def ring_submit_frames_y210(self, planes, layouts=L422_YUYV, boxes=None):
        """Y210 / Y216 / v210 frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_yuy2(planes, layouts, boxes)
        self.ring_submit_frames_y210_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_y210_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of frames that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_y210, buf, nbytes, desc)

    def ring_submit_frames_bgra(self, pixels, layouts=L444_BGRA, boxes=None):
        """8-bit packed 4:4:4 frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_bgra(pixels, layouts, boxes)
        self.ring_submit_frames_bgra_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_bgra_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of frames that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_bgra, buf, nbytes, desc)

    def ring_submit_frames_y410(self, pixels, layouts=L444_Y410, boxes=None):
        """Y416 / AYUV64 / Y410 / V410 frames into the next slot of a frames ring; every kind of frames submit may alternate."""
        buf, desc = pack_frames_bgra(pixels, layouts, boxes)
        self.ring_submit_frames_y410_packed(buf, buf.nbytes, desc)

    def ring_submit_frames_y410_packed(self, buf, nbytes, desc):
        """buf None: the slot's pinned buffer (ring_input_frames) already holds the nbytes of frames that desc describes."""
        self._ring_submit_frames(lib().vh_ring_submit_frames_y410, buf, nbytes, desc)

    def ring_free_slots(self):
        n = C.c_int(0)
        _check(lib().vh_ring_free_slots(self.h, C.byref(n)), self.h)
        return n.value

    def ring_input(self, batch):
        """numpy view of the pinned staging buffer the next submit will use."""
        p = C.POINTER(C.c_float)()
        _check(lib().vh_ring_input(self.h, C.byref(p)), self.h)
        n = batch * self.cfg["image_size"] ** 2 * self.cfg["channels"]
        return np.ctypeslib.as_array(p, shape=(n,)).reshape(batch, self.cfg["image_size"], self.cfg["image_size"], self.cfg["channels"])

    def ring_submit(self, images=None, batch=None):
        if images is None:
            _check(lib().vh_ring_submit(self.h, None, batch), self.h)
        else:
            images = np.ascontiguousarray(images, dtype=np.float32)
            _check(lib().vh_ring_submit(self.h, images.ctypes.data, images.shape[0]), self.h)

    def ring_collect(self):
        out = np.empty((max(self._ring_batch, 1), self.cfg["classes"]), dtype=np.float32)
        nb = C.c_int(0)
        _check(lib().vh_ring_collect(self.h, out.ctypes.data, C.byref(nb)), self.h)
        return out[:nb.value]

    def set_graph(self, enable=True):
        _check(lib().vh_set_graph(self.h, 1 if enable else 0), self.h)

    def get_graph(self):
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().vh_get_graph(self.h, C.byref(a), C.byref(b)), self.h)
        return bool(a.value), b.value

    def set_streams(self, n):
        _check(lib().vh_set_streams(self.h, n), self.h)

    def get_streams(self):
        n = C.c_int(0)
        _check(lib().vh_get_streams(self.h, C.byref(n)), self.h)
        return n.value

    def get_inflight(self):
        """2 when consecutive forwards (the steps of forward_device_async, image-ring submits) run two at a time, else 1."""
        n = C.c_int(0)
        _check(lib().vh_get_inflight(self.h, C.byref(n)), self.h)
        return n.value

    def set_stage_timing(self, stage_name):
        _check(lib().vh_set_stage_timing(self.h, TIMED_STAGES.index(stage_name) if stage_name else -1), self.h)

    def get_stage_timing(self):
        avg, mn, n = C.c_double(0), C.c_double(0), C.c_int(0)
        _check(lib().vh_get_stage_timing(self.h, C.byref(avg), C.byref(mn), C.byref(n)), self.h)
        return avg.value, mn.value, n.value

    def set_step_timing(self, on):
        _check(lib().vh_set_step_timing(self.h, 1 if on else 0), self.h)

    def get_step_timing(self, max_steps=4096):
        """Device time in ms of every step of the last forward_device_async call (step timing enabled)."""
        buf = (C.c_double * max_steps)()
        n = C.c_int(0)
        _check(lib().vh_get_step_timing(self.h, buf, max_steps, C.byref(n)), self.h)
        return [buf[i] for i in range(min(n.value, max_steps))]

    def debug_read(self, what, n_floats):
        out = np.empty(n_floats, dtype=np.float32)
        _check(lib().vh_debug_read(self.h, what, out.ctypes.data, n_floats), self.h)
        return out

    def debug_set_layers(self, n):
        _check(lib().vh_debug_set_layers(self.h, n), self.h)

    # ---- token features of the last forward (vithip.h "Token features") ----
    def register_tokens(self):
        """The context's number of register tokens (vh_get_register_tokens)."""
        return int(lib().vh_get_register_tokens(self.h))

    def features_dims(self):
        """(batch of the last forward, tokens, patches, dim); tokens = patches + 1 + register tokens (FLAG_NO_CLS: patches +
        register tokens)."""
        b, t, n, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().vh_features_dims(self.h, C.byref(b), C.byref(t), C.byref(n), C.byref(d)), self.h)
        return b.value, t.value, n.value, d.value

    def read_features(self, cls=True, patch=True, mean=False, elem=ELEM_F32, norm=FEAT_NORM):
        """The requested outputs of the last forward as numpy arrays: {"cls": [B, D], "patch": [B, NP, D], "mean": [B, D]} of
        float32 / float16, or uint16 holding bf16 bits for ELEM_BF16 (from16 widens them)."""
        b, _, n, d = self.features_dims()
        dt = {ELEM_F32: np.float32, ELEM_F16: np.float16, ELEM_BF16: np.uint16}.get(elem, np.float32)
        b1 = max(b, 1)   # (before the first forward the call is refused below, with the library's message)
        out = {}
        if cls:
            out["cls"] = np.empty((b1, d), dtype=dt)
        if patch:
            out["patch"] = np.empty((b1, n, d), dtype=dt)
        if mean:
            out["mean"] = np.empty((b1, d), dtype=dt)
        desc = Features(*(out[k].ctypes.data if k in out else None for k in ("cls", "patch", "mean")), elem, norm)
        _check(lib().vh_read_features(self.h, C.byref(desc)), self.h)
        return out

    def read_features_device(self, desc):
        """desc: a Features of device pointers (16-byte aligned); enqueues on the context's stream and waits."""
        _check(lib().vh_read_features_device(self.h, C.byref(desc)), self.h)

    def read_features_device_async(self, desc):
        """The same, enqueue only: synchronize(), or stream order with a following call on the context."""
        _check(lib().vh_read_features_device_async(self.h, C.byref(desc)), self.h)

    # ---- layer features: several layers of one forward (vithip.h "Layer features") ----
    def set_feature_layers(self, layers):
        """The layers every following forward captures: strictly ascending, each 1 .. layers (k = the residual stream after k
        layers, Hugging Face's hidden_states[k]); an empty list clears it and frees the capture store."""
        layers = [int(k) for k in layers]
        arr = (C.c_int * max(len(layers), 1))(*layers)
        _check(lib().vh_set_feature_layers(self.h, arr, len(layers)), self.h)

    def feature_layers(self):
        arr, n = (C.c_int * MAX_FEATURE_LAYERS)(), C.c_int(0)
        _check(lib().vh_get_feature_layers(self.h, arr, C.byref(n)), self.h)
        return [arr[i] for i in range(n.value)]

    def read_layer_features(self, layer=-1, cls=True, patch=True, mean=False, reg=False, elem=ELEM_F32, norm=FEAT_NORM, nchw=False):
        """read_features for `layer` of the last forward (-1 / the model's layer count: the final state; else a listed layer), plus
        "reg": [B, R, D], and with nchw the patch rows as [B, D, gh, gw]."""
        b, _, n, d = self.features_dims()
        dt = {ELEM_F32: np.float32, ELEM_F16: np.float16, ELEM_BF16: np.uint16}.get(elem, np.float32)
        b1 = max(b, 1)   # (before the first forward the call is refused below, with the library's message)
        g = self.cfg["image_size"] // self.cfg["patch_size"]
        out = {}
        if cls:
            out["cls"] = np.empty((b1, d), dtype=dt)
        if patch:
            out["patch"] = np.empty((b1, d, g, g) if nchw else (b1, n, d), dtype=dt)
        if mean:
            out["mean"] = np.empty((b1, d), dtype=dt)
        if reg:
            out["reg"] = np.empty((b1, max(self.register_tokens(), 1), d), dtype=dt)   # (no registers: refused below)
        desc = LayerFeatures(*(out[k].ctypes.data if k in out else None for k in ("cls", "patch", "mean", "reg")), elem, norm, layer,
                             FEAT_NCHW if nchw else FEAT_ROWS)
        _check(lib().vh_read_layer_features(self.h, C.byref(desc)), self.h)
        return out

    def read_layer_features_device(self, desc):
        """desc: a LayerFeatures of device pointers (16-byte aligned); enqueues on the context's stream and waits."""
        _check(lib().vh_read_layer_features_device(self.h, C.byref(desc)), self.h)

    def read_layer_features_device_async(self, desc):
        """The same, enqueue only: synchronize(), or stream order with a following call on the context."""
        _check(lib().vh_read_layer_features_device_async(self.h, C.byref(desc)), self.h)

    def get_intermediate_layers(self, n=1, reshape=False, return_class_token=False, norm=True):
        """DINOv2's get_intermediate_layers for the images of the LAST forward: n an int = the last n layers, or a list of 0-based
        block indices (block i = the residual stream after i + 1 layers).  Capture happens inside a forward: if the context's list
        differs it is set here and the read is refused (VhError, state) until the caller has run the forward again -- set the list
        first, or call this once before the first forward.  Returns a tuple with one entry per layer: the patch tokens
        [B, NP, D], or [B, D, gh, gw] with reshape; with return_class_token (patch, cls [B, D]) -- which a FLAG_NO_CLS context,
        having no class token, refuses (ValueError)."""
        if return_class_token and self.c.flags & FLAG_NO_CLS:
            raise ValueError("get_intermediate_layers: return_class_token on a context without a class token (FLAG_NO_CLS)")
        total = self.cfg["layers"]
        blocks = list(range(total - n, total)) if isinstance(n, int) else [int(i) for i in n]
        if not blocks or min(blocks) < 0 or max(blocks) >= total or blocks != sorted(set(blocks)):
            raise ValueError(f"get_intermediate_layers: blocks {blocks} are not ascending indices within 0..{total - 1}")
        want = [i + 1 for i in blocks]
        if self.feature_layers() != want:
            self.set_feature_layers(want)
        out = []
        for k in want:
            f = self.read_layer_features(k, cls=return_class_token, patch=True, norm=FEAT_NORM if norm else FEAT_RAW, nchw=reshape)
            out.append((f["patch"], f["cls"]) if return_class_token else f["patch"])
        return tuple(out)

    # ---- attention maps: the class-token / register rows of listed layers (vithip.h "Attention maps") ----
    def set_attention_layers(self, layers, queries=ATTN_Q_CLS):
        """The layers whose attention every following forward keeps: strictly ascending, each 1 .. layers (k = the k-th encoder layer,
        Hugging Face's attentions[k - 1]); queries ATTN_Q_CLS = row 0, ATTN_Q_LEAD = the class token and the registers.  An empty
        list clears it and frees the store."""
        layers = [int(k) for k in layers]
        arr = (C.c_int * max(len(layers), 1))(*layers)
        _check(lib().vh_set_attention_layers(self.h, arr, len(layers), queries), self.h)

    def attention_layers(self):
        """(the list, its queries constant)."""
        arr, n, q = (C.c_int * MAX_ATTENTION_LAYERS)(), C.c_int(0), C.c_int(0)
        _check(lib().vh_get_attention_layers(self.h, arr, C.byref(n), C.byref(q)), self.h)
        return [arr[i] for i in range(n.value)], q.value

    def attention_dims(self):
        """(batch of the last forward, heads, query rows Q of the list in force, tokens, patches)."""
        v = [C.c_int(0) for _ in range(5)]
        _check(lib().vh_attention_dims(self.h, *(C.byref(x) for x in v)), self.h)
        return tuple(x.value for x in v)

    def read_attention(self, layer=-1, probs=True, head_mean=False, elem=ELEM_F32, keys=ATTN_KEYS_ALL):
        """The attention maps of `layer` of the last forward as numpy arrays: {"probs": [B, H, Q, K], "head_mean": [B, Q, K]} of
        float32 / float16, or uint16 holding bf16 bits for ELEM_BF16; K = tokens, or the patches with ATTN_KEYS_PATCH."""
        b, h, q, t, n = self.attention_dims()
        dt = {ELEM_F32: np.float32, ELEM_F16: np.float16, ELEM_BF16: np.uint16}.get(elem, np.float32)
        b1, q1, k = max(b, 1), max(q, 1), (n if keys == ATTN_KEYS_PATCH else t)   # (no forward / no list: refused below)
        out = {}
        if probs:
            out["probs"] = np.empty((b1, h, q1, k), dtype=dt)
        if head_mean:
            out["head_mean"] = np.empty((b1, q1, k), dtype=dt)
        desc = AttentionMaps(*(out[x].ctypes.data if x in out else None for x in ("probs", "head_mean")), elem, layer, keys, 0)
        _check(lib().vh_read_attention(self.h, C.byref(desc)), self.h)
        return out

    def read_attention_device(self, desc):
        """desc: an AttentionMaps of device pointers (16-byte aligned); enqueues on the context's stream and waits."""
        _check(lib().vh_read_attention_device(self.h, C.byref(desc)), self.h)

    def read_attention_device_async(self, desc):
        """The same, enqueue only: synchronize(), or stream order with a following call on the context."""
        _check(lib().vh_read_attention_device_async(self.h, C.byref(desc)), self.h)

    def cls_attention(self, layer=-1, reshape=True):
        """DINO's get_last_selfattention for the images of the LAST forward: the class token's softmax row per head, [B, H, gh, gw]
        (attentions[:, :, 0, 1:] reshaped; the patch columns, not renormalised) or without reshape [B, H, tokens].  Capture happens
        inside a forward: if `layer` is not listed the list is set here (ATTN_Q_CLS) and the read is refused (VhError, state)
        until the caller has run the forward again."""
        k = self.cfg["layers"] if layer == -1 else int(layer)
        have, _ = self.attention_layers()
        if k not in have:
            self.set_attention_layers([k], ATTN_Q_CLS)
        p = self.read_attention(k, keys=ATTN_KEYS_PATCH if reshape else ATTN_KEYS_ALL)["probs"][:, :, 0]
        if not reshape:
            return p
        g = self.cfg["image_size"] // self.cfg["patch_size"]
        return p.reshape(p.shape[0], p.shape[1], g, g)


def group_shard_bounds(batch, n, r):
    lo, hi = C.c_int(0), C.c_int(0)
    lib().vh_group_shard_bounds(batch, n, r, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class VitGroup:
    """vh_group wrapper: the N GPUs of one node from one process (one context + host thread per device inside
    libvithip, one RCCL broadcast of the weight blob, contiguous image shards)."""

    def __init__(self, cfg, devices, dtype=DTYPE_BF16, max_batch_per_device=1, ln_eps=1e-6, flags=0):
        self.cfg, self.devices = dict(cfg), list(devices)
        self.c = make_config(cfg, dtype, max_batch_per_device, ln_eps, flags)
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(lib().vh_group_create(C.byref(self.c), arr, len(self.devices), C.byref(h)))
        self.h = h.value

    def _chk(self, rc):
        if rc != 0:
            msg = lib().vh_group_last_error(self.h)
            raise VhError(rc, msg.decode() if msg else "?")

    def close(self):
        if self.h:
            lib().vh_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        n = C.c_int(0)
        self._chk(lib().vh_group_size(self.h, C.byref(n)))
        return n.value

    def fp8_guard(self):
        """(largest |x| bound seen on the raw residual rows of an fp8 context, e4m3's limit 448)."""
        a, lim = C.c_float(0), C.c_float(0)
        _check(lib().vh_get_fp8_guard(self.h, C.byref(a), C.byref(lim)), self.h)
        return a.value, lim.value

    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._chk(lib().vh_group_load_weights(self.h, blob.ctypes.data, blob.nbytes))

    def init_weights_seeded(self, seed):
        self._chk(lib().vh_group_init_weights_seeded(self.h, seed))

    def forward(self, images):
        images = np.ascontiguousarray(images, dtype=np.float32)
        out = np.empty((images.shape[0], self.cfg["classes"]), dtype=np.float32)
        self._chk(lib().vh_group_forward(self.h, images.ctypes.data, images.shape[0], out.ctypes.data))
        return out

    def fill_inputs_seeded(self, seed, batch_per_device):
        self._chk(lib().vh_group_fill_inputs_seeded(self.h, seed, batch_per_device))

    def forward_resident(self, batch_per_device, steps=1):
        self._chk(lib().vh_group_forward_resident(self.h, batch_per_device, steps))

    def read_logits(self, batch_per_device):
        out = np.empty((len(self.devices) * batch_per_device, self.cfg["classes"]), dtype=np.float32)
        self._chk(lib().vh_group_read_logits(self.h, batch_per_device, out.ctypes.data))
        return out


class MlpContext:
    """vh_mlp wrapper — the reference's real launch_forward semantics (dense-layer chain)."""

    def __init__(self, n_ins, n_p_l, activation=ACT_RELU2, device=0):
        self.n_ins, self.n_p_l = n_ins, list(n_p_l)
        arr = (C.c_int * len(n_p_l))(*n_p_l)
        h = C.c_void_p()
        _check(lib().vh_mlp_create(device, n_ins, len(n_p_l), arr, activation, C.byref(h)))
        self.h = h.value

    def _chk(self, rc):
        if rc != 0:
            msg = lib().vh_mlp_last_error(self.h)
            raise VhError(rc, msg.decode() if msg else "?")

    def load_params(self, params, bias):
        p = np.ascontiguousarray(params, dtype=np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32)
        self._chk(lib().vh_mlp_load_params(self.h, p.ctypes.data, p.size, b.ctypes.data, b.size))

    def forward(self, inputs):
        x = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, self.n_ins)
        out = np.empty((x.shape[0], self.n_p_l[-1]), dtype=np.float32)
        self._chk(lib().vh_mlp_forward(self.h, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def init_gradient(self, set_ins, set_outs):
        si = np.ascontiguousarray(set_ins, dtype=np.float32).reshape(-1, self.n_ins)
        so = np.ascontiguousarray(set_outs, dtype=np.float32).reshape(si.shape[0], self.n_p_l[-1])
        self._chk(lib().vh_mlp_init_gradient(self.h, si.ctypes.data, so.ctypes.data, si.shape[0]))

    def launch_gradient(self, iterations, error_threshold, multiplier):
        err = np.zeros(max(iterations, 1), dtype=np.float32)
        self._chk(lib().vh_mlp_launch_gradient(self.h, iterations, error_threshold, multiplier, err.ctypes.data))
        return err[:iterations]

    def read_params(self):
        fan, n_params = self.n_ins, 0
        for n in self.n_p_l:
            n_params += n * fan
            fan = n
        p, b = np.empty(n_params, dtype=np.float32), np.empty(sum(self.n_p_l), dtype=np.float32)
        self._chk(lib().vh_mlp_read_params(self.h, p.ctypes.data, p.size, b.ctypes.data, b.size))
        return p, b

    def last_gradient_us(self):
        us = C.c_int64(0)
        self._chk(lib().vh_mlp_last_gradient_us(self.h, C.byref(us)))
        return us.value

    def close(self):
        if self.h:
            lib().vh_mlp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- operator-level wrappers (device pointers in, nothing hidden) ------------------------------------
def op_gemm(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, dtype, aux_ptr=None, aux_i=0, variant=0):
    _check(lib().vh_op_gemm(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, aux_ptr, aux_i, dtype, variant, None))


def op_gemm_fp8(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, variant=0):
    _check(lib().vh_op_gemm_fp8(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, variant, None))


def op_quantize_rows(w_ptr, rows, cols, post_scale, w8_ptr, scale_ptr):
    _check(lib().vh_op_quantize_rows(w_ptr, rows, cols, post_scale, w8_ptr, scale_ptr, None))


def op_gemm_fp8_ex(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, c_ptr=None, stats_ptr=None, out16_ptr=None,
                   partials_ptr=None, variant=0):
    _check(lib().vh_op_gemm_fp8_ex(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, c_ptr, stats_ptr, out16_ptr,
                                   partials_ptr, variant, None))


# ---- OCP e4m3fn on the host (table-driven; used to build / read fp8 operator operands in tests) ----
def e4m3_table():
    b = np.arange(256, dtype=np.uint32)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b >> 7 == 1, -v, v).astype(np.float32)


def from_e4m3(b):
    return e4m3_table()[np.ascontiguousarray(b, dtype=np.uint8)]


def to_e4m3(x):
    """fp32 -> OCP e4m3fn bytes: round to nearest even, saturating at +-448 (what pack4_e4m3 does on the device)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    pos = e4m3_table()[:127].astype(np.float64)          # codes 0x00 .. 0x7E, ascending (0x7F is NaN)
    a = np.minimum(np.abs(x).astype(np.float64), 448.0)
    hi = np.clip(np.searchsorted(pos, a, side="left"), 1, 126)
    lo = hi - 1
    dl, dh = a - pos[lo], pos[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


# ---- the lo plane of the split residual: one e4m3 byte per element, scaled (csrc/vh_common.h Lo8) ----
LO8_SCALE = {DTYPE_BF16: 32.0, DTYPE_FP16: 256.0}


def to_lo8(residue, dtype):
    return to_e4m3(np.asarray(residue, dtype=np.float32) * np.float32(LO8_SCALE[dtype]))


def from_lo8(b, dtype):
    return from_e4m3(b) / np.float32(LO8_SCALE[dtype])


def op_gemm_ex(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, dtype, aux_ptr=None, aux_i=0, stats_ptr=None,
               out16_ptr=None, partials_ptr=None, variant=0):
    _check(lib().vh_op_gemm_ex(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, aux_ptr, aux_i, stats_ptr, out16_ptr,
                               partials_ptr, dtype, variant, None))


def op_gemm_layout(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, dtype, aux_ptr=None, aux_i=0, stats_ptr=None,
                   out16_ptr=None, partials_ptr=None, variant=0, out_tiled=False, ab_tiled=False, tile_begin=0, tile_count=0):
    """Test tap: op_gemm_ex with the tiled / head-major result (out_tiled: unpack_tiled, pack_head_major), tiled A and W
    (ab_tiled: pack_tiled, op_tile_rows) or a range of the 256 x 256 tiles (variants 5 and 7)."""
    _check(lib().vh_op_gemm_layout(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, aux_ptr, aux_i, stats_ptr, out16_ptr,
                                   partials_ptr, dtype, variant, 1 if out_tiled else 0, 1 if ab_tiled else 0, tile_begin, tile_count, None))


def op_gemm_lead(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, dtype, pos_ptr, patches, lead, out16_ptr=None, partials_ptr=None,
                 prow=0, variant=0):
    """Test tap: the EPI_PATCH / EPI_PATCH_SPLIT epilogues with `lead` = 1 + R rows in front of an image's `patches` patch rows:
    GEMM row img * patches + p lands on output row img * (patches + lead) + lead + p and adds pos row 1 + p."""
    _check(lib().vh_op_gemm_lead(a_ptr, w_ptr, bias_ptr, out_ptr, M, N, K, epilogue, pos_ptr, patches, lead, out16_ptr, partials_ptr,
                                 prow, dtype, variant, None))


def op_lead_rows(x_or_hi_ptr, cls_ptr, pos_ptr, reg_ptr, lead, batch, tokens, dim, lo_ptr=None, partials_ptr=None, prow=0,
                 dtype=DTYPE_BF16):
    """Test tap: the kernels that write the `lead` leading rows of every image (row 0 = cls + pos[0], row 1 + r = reg[r]): fp32
    rows (lo_ptr None), or the split planes and the rows' per-64-column partial sums [dim / 64][prow][2]."""
    _check(lib().vh_op_lead_rows(x_or_hi_ptr, lo_ptr, partials_ptr, prow, cls_ptr, pos_ptr, reg_ptr, lead, batch, tokens, dim, dtype, None))


def op_gemm_fp8_layout(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, c_ptr=None, stats_ptr=None, out16_ptr=None,
                       partials_ptr=None, variant=0, out_tiled=False, ab_tiled=False, tile_begin=0, tile_count=0):
    """Test tap: op_gemm_fp8 / op_gemm_fp8_ex with the same four extras as op_gemm_layout (e4m3 chunks are 16 bytes)."""
    _check(lib().vh_op_gemm_fp8_layout(a8_ptr, w8_ptr, scale_ptr, bias_ptr, out_ptr, M, N, K, epilogue, c_ptr, stats_ptr, out16_ptr,
                                       partials_ptr, variant, 1 if out_tiled else 0, 1 if ab_tiled else 0, tile_begin, tile_count, None))


def op_tile_rows(in_ptr, rows, cols, out_ptr, dtype):
    """Test tap: fp32 [rows, cols] -> 16-bit tiled (pack_tiled(to16(.), 8)), or with DTYPE_FP8 bytes -> tiled bytes (chunk 16)."""
    _check(lib().vh_op_tile_rows(in_ptr, rows, cols, out_ptr, dtype, None))


def op_rowstats_cast(x_ptr, rows, dim, eps, x16_ptr, stats_ptr, dtype):
    _check(lib().vh_op_rowstats_cast(x_ptr, rows, dim, eps, x16_ptr, stats_ptr, dtype, None))


def op_rowstats_split(x_ptr, rows, dim, eps, hi_ptr, lo_ptr, stats_ptr, dtype):
    _check(lib().vh_op_rowstats_split(x_ptr, rows, dim, eps, hi_ptr, lo_ptr, stats_ptr, dtype, None))


def op_pre_layernorm(x_ptr, rows, dim, gamma_ptr, beta_ptr, eps, y32_ptr, hi_ptr, lo_ptr, stats_ptr, dtype):
    _check(lib().vh_op_pre_layernorm(x_ptr, rows, dim, gamma_ptr, beta_ptr, eps, y32_ptr, hi_ptr, lo_ptr, stats_ptr, dtype, None))


def op_finalize_stats(partials_ptr, nblk, rows, dim, eps, stats_ptr):
    _check(lib().vh_op_finalize_stats(partials_ptr, nblk, rows, dim, eps, stats_ptr, None))


def op_fold_ln(w_ptr, b_ptr, gamma_ptr, beta_ptr, rows, dim, scale, w16_ptr, c_ptr, d_ptr, dtype):
    _check(lib().vh_op_fold_ln(w_ptr, b_ptr, gamma_ptr, beta_ptr, rows, dim, scale, w16_ptr, c_ptr, d_ptr, dtype, None))


# ---- test taps of the row kernels (include/vithip.h, "Test taps of the row kernels"; tests/rows_exact.py) ----
def op_rowstats_guard(x_ptr, rows, dim, eps, hi_ptr, lo_ptr, stats_ptr, dtype, guard_rows=0, amax_guard_ptr=None):
    """op_rowstats_cast (lo_ptr None) / op_rowstats_split with the e4m3 form's |x| guard word over the first guard_rows rows."""
    _check(lib().vh_op_rowstats_guard(x_ptr, rows, dim, eps, hi_ptr, lo_ptr, stats_ptr, dtype, guard_rows, amax_guard_ptr, None))


def op_pre_layernorm_guard(x_ptr, rows, dim, gamma_ptr, beta_ptr, eps, y32_ptr, hi_ptr, lo_ptr, stats_ptr, dtype, guard_rows=0,
                           guard_ptr=None, amax_guard_ptr=None):
    _check(lib().vh_op_pre_layernorm_guard(x_ptr, rows, dim, gamma_ptr, beta_ptr, eps, y32_ptr, hi_ptr, lo_ptr, stats_ptr, dtype,
                                           guard_rows, guard_ptr, amax_guard_ptr, None))


def op_finalize_stats_guard(partials_ptr, nblk, rows, dim, eps, stats_ptr, guard_rows=0, guard_ptr=None, amax_guard_ptr=None):
    _check(lib().vh_op_finalize_stats_guard(partials_ptr, nblk, rows, dim, eps, stats_ptr, guard_rows, guard_ptr, amax_guard_ptr, None))


def op_ln_guard(stats_ptr, rows, guard_ptr):
    _check(lib().vh_op_ln_guard(stats_ptr, rows, guard_ptr, None))


def op_layernorm_f32(x_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out32_ptr):
    _check(lib().vh_op_layernorm_f32(x_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out32_ptr, None))


def op_layernorm_split(hi_ptr, lo_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out32_ptr, dtype):
    """LayerNorm of rows of the split residual -> fp32: 16-bit hi + lo8 byte (DTYPE_BF16 / DTYPE_FP16), or e4m3 hi + bf16 lo (DTYPE_FP8)."""
    _check(lib().vh_op_layernorm_split(hi_ptr, lo_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out32_ptr, dtype, None))


def op_head_f32(y_ptr, w_ptr, bias_ptr, out_ptr, batch, classes, dim):
    _check(lib().vh_op_head_f32(y_ptr, w_ptr, bias_ptr, out_ptr, batch, classes, dim, None))


def op_fold_ln_f8(w_ptr, b_ptr, gamma_ptr, beta_ptr, rows, dim, scale, w8_ptr, wscale_ptr, c_ptr, d_ptr):
    _check(lib().vh_op_fold_ln_f8(w_ptr, b_ptr, gamma_ptr, beta_ptr, rows, dim, scale, w8_ptr, wscale_ptr, c_ptr, d_ptr, None))


def op_fake_quant_rows(w_ptr, rows, cols, out_ptr):
    _check(lib().vh_op_fake_quant_rows(w_ptr, rows, cols, out_ptr, None))


def bench_gemm(M, N, K, epilogue, dtype=DTYPE_BF16, variant=0, iters=20, device=0):
    """Average launch time in ms of one GEMM shape (synthetic operands generated in HBM)."""
    ms = C.c_double(0)
    _check(lib().vh_bench_gemm(device, M, N, K, epilogue, dtype, variant, iters, C.byref(ms)))
    return ms.value


def op_token_features(hi_ptr, lo_ptr, form, batch, tokens, dim, gamma_ptr, beta_ptr, eps, elem, norm, patch_ptr, mean_ptr):
    """The token-feature kernels on rows made by the caller: split planes (form DTYPE_BF16 / DTYPE_FP16 / DTYPE_FP8) or fp32 rows
    (FEAT_FORM_F32, lo_ptr None) -> patch [batch, tokens - 1, dim] and / or mean [batch, dim] of `elem`."""
    _check(lib().vh_op_token_features(hi_ptr, lo_ptr, form, batch, tokens, dim, gamma_ptr, beta_ptr, eps, elem, norm, patch_ptr, mean_ptr, None))


def op_token_features2(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, elem, norm, patch_ptr, patch_layout,
                       mean_ptr, reg_ptr):
    """op_token_features with `lead` rows in front of an image's patch rows (1 + the register rows), reg [batch, lead - 1, dim] and
    patch_layout FEAT_ROWS ([batch, tokens - lead, dim]) / FEAT_NCHW ([batch, dim, tokens - lead])."""
    _check(lib().vh_op_token_features2(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, elem, norm, patch_ptr,
                                       patch_layout, mean_ptr, reg_ptr, None))


def op_pool_rows(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, norm, mean_ptr):
    """The pooled head's one-pass kernel on its own (vh_op_pool_rows): mean [batch, dim] fp32 over rows lead .. tokens - 1 of every image
    (lead 0 .. tokens - 1), FEAT_RAW or through LayerNorm(gamma, beta, eps) -- the bits op_token_features2 writes for ELEM_F32."""
    _check(lib().vh_op_pool_rows(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, norm, mean_ptr, None))


def op_map_pool(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, qk_ptr, heads, z_ptr):
    """The attention-pooling head's one-pass kernel on its own (vh_op_map_pool): z [batch, heads, dim] fp32 = the softmax(qk[h] . y_t)-
    weighted sum of y_t = LayerNorm(row t; gamma, beta, eps) over rows lead .. tokens - 1 of every image; qk [heads, dim] fp32."""
    _check(lib().vh_op_map_pool(hi_ptr, lo_ptr, form, batch, tokens, lead, dim, gamma_ptr, beta_ptr, eps, qk_ptr, heads, z_ptr, None))


def op_rope(qkv_ptr, dtype, batch, tokens, heads, head_dim, lead, hm_rows, cos_ptr, sin_ptr):
    """The VH_FLAG_ROPE rotation on its own (vh_op_rope), in place: q and k of rows lead .. tokens - 1 of every image and head of the
    q|k|v at qkv_ptr (`dtype` elements; hm_rows = 0: row-major [batch * tokens, 3 * heads * head_dim], else head-major
    [3, heads, hm_rows, 64]) are rotated by the fp32 tables cos / sin [tokens - lead, head_dim / 2]."""
    _check(lib().vh_op_rope(qkv_ptr, dtype, batch, tokens, heads, head_dim, lead, hm_rows, cos_ptr, sin_ptr, None))


def op_swiglu(gu_ptr, dtype, rows, mlp_dim, h_ptr, out_tiled=False):
    """The VH_FLAG_SWIGLU gate pass on its own (vh_op_swiglu): gu [rows, 2 * mlp_dim] row-major `dtype` elements (gate columns first) ->
    h = silu(g) * u [rows, mlp_dim], row-major or (out_tiled; rows a multiple of 16) in the layout unpack_tiled reads."""
    _check(lib().vh_op_swiglu(gu_ptr, dtype, rows, mlp_dim, h_ptr, 1 if out_tiled else 0, None))


def op_layernorm(x_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out_ptr, dtype):
    _check(lib().vh_op_layernorm(x_ptr, rows, dim, row_stride, gamma_ptr, beta_ptr, eps, out_ptr, dtype, None))


def op_attention(qkv_ptr, batch, tokens, heads, out_ptr, dtype):
    _check(lib().vh_op_attention(qkv_ptr, batch, tokens, heads, out_ptr, dtype, None))


def op_attention_stream(qkv_ptr, batch, tokens, heads, out_ptr, dtype):
    """The K/V-streaming attention kernel at any token count 1..4097 (op_attention uses it above 640 tokens)."""
    _check(lib().vh_op_attention_stream(qkv_ptr, batch, tokens, heads, out_ptr, dtype, None))


def op_attention_hd(qkv_ptr, batch, tokens, heads, head_dim, out_ptr, dtype):
    """Attention at head dim 32, 48, ..., 128 (q pre-scaled by head_dim^-1/2 * log2(e)), any token count 1..4097."""
    _check(lib().vh_op_attention_hd(qkv_ptr, batch, tokens, heads, head_dim, out_ptr, dtype, None))


def op_attention_cls(qkv_ptr, batch, tokens, heads, out_ptr, dtype):
    """Test tap: attention of every image's row 0 only (the VH_FLAG_CLS_TAIL kernel): out [batch][heads * 64], tokens <= 1024."""
    _check(lib().vh_op_attention_cls(qkv_ptr, batch, tokens, heads, out_ptr, dtype, None))


def op_attention_layout(qkv_ptr, batch, tokens, heads, out_ptr, dtype, out_tiled=False, in_hm_rows=0):
    """Test tap: op_attention with the 16-row-blocked output (unpack_tiled) and / or head-major q|k|v (pack_head_major)."""
    _check(lib().vh_op_attention_layout(qkv_ptr, batch, tokens, heads, out_ptr, dtype, 1 if out_tiled else 0, in_hm_rows, None))


def op_attention_probs(qkv_ptr, batch, tokens, heads, head_dim, queries, dtype, probs_ptr, in_hm_rows=0):
    """The capture kernel of the attention maps alone: the softmax rows of every image's first `queries` rows -> probs_ptr fp32
    [batch, heads, queries, tokens]; q|k|v row-major, or head-major (pack_head_major) with in_hm_rows at head_dim 64."""
    _check(lib().vh_op_attention_probs(qkv_ptr, batch, tokens, heads, head_dim, queries, in_hm_rows, dtype, probs_ptr, None))


def op_attention_readout(store_ptr, batch, heads, queries, tokens, lead, elem, keys, probs_ptr, head_mean_ptr):
    """The read-out kernel of the attention maps alone: store fp32 [batch, heads, queries, tokens] -> probs [batch, heads, queries, K]
    and / or head_mean [batch, queries, K] in `elem`; K = tokens, or tokens - lead with ATTN_KEYS_PATCH."""
    _check(lib().vh_op_attention_readout(store_ptr, batch, heads, queries, tokens, lead, elem, keys, probs_ptr, head_mean_ptr, None))


def op_im2col(in_ptr, batch, image, patch, channels, out_ptr, dtype):
    _check(lib().vh_op_im2col(in_ptr, batch, image, patch, channels, out_ptr, dtype, None))


def op_im2col_padded(in_ptr, batch, image, patch, channels, kpad, out_ptr, dtype):
    """Patch matrix [batch*np, kpad] for any patch and channel count: columns patch^2*channels..kpad-1 are zero.
    kpad >= patch^2*channels and a multiple of 8; dtype bf16 or fp16."""
    _check(lib().vh_op_im2col_padded(in_ptr, batch, image, patch, channels, kpad, out_ptr, dtype, None))


def op_im2col_u8(in_ptr, batch, image, patch, channels, kpad, scale, shift, out_ptr, dtype):
    """Patch matrix [batch*np, kpad] of uint8 NHWC images: element = dtype(fmaf(float(p), scale[c], shift[c])), pad columns
    zero.  scale / shift: host arrays [channels]; in_ptr 16-byte aligned."""
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32).reshape(-1)
    for a in (sc, sh):
        if a is not None and a.size != channels:
            raise ValueError(f"op_im2col_u8: expected {channels} values per array, got {a.size}")
    _check(lib().vh_op_im2col_u8(in_ptr, batch, image, patch, channels, kpad, None if sc is None else sc.ctypes.data,
                                 None if sh is None else sh.ctypes.data, out_ptr, dtype, None))


def op_im2col_tensor(in_ptr, elem, layout, batch, image, patch, channels, kpad, out_ptr, dtype, scale=None, shift=None):
    """Patch matrix [batch*np, kpad] of an image tensor (ELEM_*, LAYOUT_*) at in_ptr (device, 16-byte aligned): the bits
    op_im2col_padded gives for the NHWC fp32 array of its widened elements; scale / shift: [channels], ELEM_U8 only."""
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32).reshape(-1)
    for a in (sc, sh):
        if a is not None and a.size != channels:
            raise ValueError(f"op_im2col_tensor: expected {channels} values per array, got {a.size}")
    _check(lib().vh_op_im2col_tensor(in_ptr, elem, layout, batch, image, patch, channels, kpad, None if sc is None else sc.ctypes.data,
                                     None if sh is None else sh.ctypes.data, out_ptr, dtype, None))


def op_resize_u8(frames_ptr, nbytes, desc, channels, out_size, out_ptr):
    """The resize of the frames entry points on its own: the frames at frames_ptr (device, any alignment) described by the
    (Frame * n) array desc -> [n, out_size, out_size, channels] bytes at out_ptr."""
    _check(lib().vh_op_resize_u8(frames_ptr, nbytes, C.addressof(desc), len(desc), channels, out_size, out_ptr, None))


def _op_resize_colour(name, fn, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """The body of the taps that take a colour matrix; `fn` is the format's C tap."""
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    if m.size != 12:
        raise ValueError(f"{name}: expected 12 matrix entries, got {m.size}")
    _check(fn(frames_ptr, nbytes, C.addressof(desc), len(desc), out_size, m.ctypes.data, chroma_site, out_ptr, None))


def op_resize_yuv(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """The resize + colour conversion of the planar YUV entry points on its own: the planes at frames_ptr (device, any alignment)
    described by the (FrameYUV * n) array desc -> [n, out_size, out_size, 3] bytes at out_ptr.  m: 12 floats, row-major 3 x 4."""
    _op_resize_colour("op_resize_yuv", lib().vh_op_resize_yuv, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_p016(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_nv12 for 16-bit samples: frames_ptr (device, 2-byte aligned), offsets and strides in bytes and even."""
    _op_resize_colour("op_resize_p016", lib().vh_op_resize_p016, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_yuv16(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_yuv for 16-bit samples: frames_ptr (device, 2-byte aligned), offsets and strides in bytes and even."""
    _op_resize_colour("op_resize_yuv16", lib().vh_op_resize_yuv16, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_yuy2(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_yuv for 8-bit packed 4:2:2 frames: (FrameYUY2 * n) descriptors, frames_ptr of any alignment."""
    _op_resize_colour("op_resize_yuy2", lib().vh_op_resize_yuy2, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_y210(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_yuv16 for Y210 / Y216 / v210 frames: frames_ptr 2-byte aligned, offsets and strides even (v210: multiples of 4)."""
    _op_resize_colour("op_resize_y210", lib().vh_op_resize_y210, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_bgra(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_yuv for 8-bit packed 4:4:4 frames: (FrameBGRA * n) descriptors, frames_ptr of any alignment.  RGB layouts ignore
    m, and every layout ignores chroma_site."""
    _op_resize_colour("op_resize_bgra", lib().vh_op_resize_bgra, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_y410(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """op_resize_yuv16 for Y416 / AYUV64 / Y410 / V410 frames: frames_ptr 2-byte aligned, offsets and strides even (Y410 / V410:
    multiples of 4)."""
    _op_resize_colour("op_resize_y410", lib().vh_op_resize_y410, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_resize_nv12(frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr):
    """The resize + colour conversion of the NV12 entry points on its own: the planes at frames_ptr (device, any alignment)
    described by the (FrameNV12 * n) array desc -> [n, out_size, out_size, 3] bytes at out_ptr.  m: 12 floats, row-major 3 x 4."""
    _op_resize_colour("op_resize_nv12", lib().vh_op_resize_nv12, frames_ptr, nbytes, desc, out_size, m, chroma_site, out_ptr)


def op_cast(in_ptr, out_ptr, n, dtype):
    _check(lib().vh_op_cast(in_ptr, out_ptr, n, dtype, None))


def op_fill(out_ptr, n, seed, tensor_id, kind, sigma=0.0):
    _check(lib().vh_op_fill(out_ptr, n, seed, tensor_id, kind, sigma, None))
