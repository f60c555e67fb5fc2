"""Host reference of the token features (include/vithip.h, "Token features"), numpy only: the fp64 LayerNorm the normalised rows
are compared against, the sequential fp32 mean chain (exact: the device must give its bits), round-to-nearest-even to the 16-bit
element types, and the synthetic split planes the operator tap is driven with."""
import numpy as np

import vithip

NORM_BOUND = 2.0 ** -18   # max|got - ref| <= NORM_BOUND * max|ref| for a normalised row against the fp64 LayerNorm

# the small models of the feature tests.  feat_fold: T = 37 (odd: a 4-rows-per-block kernel has a ragged last block), dim and mlp_dim
# multiples of 256, so it folds and splits under default flags and is eligible for VH_DTYPE_FP8
FEAT_FOLD = dict(image_size=96, patch_size=16, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=8)


def layernorm64(x, gamma, beta, eps):
    """fp64 LayerNorm of the rows of x (last axis), returned in fp64."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + np.float64(eps)) * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)


def mean_chain(patch32):
    """patch32 [B, NP, D] fp32 -> [B, D]: (((0 + v1) + v2) + ... + vNP) * (float)(1.0 / NP), every operation in fp32."""
    p = np.ascontiguousarray(patch32, dtype=np.float32)
    acc = np.zeros((p.shape[0], p.shape[2]), dtype=np.float32)
    for t in range(p.shape[1]):
        acc = acc + p[:, t, :]
    return acc * np.float32(1.0 / p.shape[1])


def rne16(a32, elem):
    """fp32 -> the bits of the 16-bit element type (uint16), round to nearest even."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if elem == vithip.ELEM_BF16:
        return vithip.to_bf16_bits(a32)
    assert elem == vithip.ELEM_F16
    return a32.astype(np.float16).view(np.uint16)


def bits(a):
    """The storage bits of an output array (float32 -> uint32, float16 -> uint16, uint16 as it is), for exact comparisons."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def split_planes(x32, form):
    """fp32 rows -> (hi, lo, x) as the residual paths keep them: x = (float)hi + lo with one fp32 add, the value the device
    reconstructs.  form DTYPE_BF16 / DTYPE_FP16: 16-bit hi + one scaled e4m3 byte; DTYPE_FP8: e4m3 hi + bf16 lo;
    FEAT_FORM_F32: the rows themselves (lo None)."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if form == vithip.FEAT_FORM_F32:
        return x32, None, x32
    if form == vithip.DTYPE_FP8:
        hi = vithip.to_e4m3(x32)
        hv = vithip.from_e4m3(hi).astype(np.float32)
        lo = vithip.to_bf16_bits(x32 - hv)
        return hi, lo, hv + vithip.from_bf16_bits(lo)
    hi = vithip.to16(x32, form)
    hv = vithip.from16(hi, form)
    lo = vithip.to_lo8(x32 - hv, form)
    return hi, lo, hv + vithip.from_lo8(lo, form).astype(np.float32)


def rows_with_outlier(rng, batch, tokens, dim, scale=1.0):
    """[batch * tokens, dim] fp32 rows of sigma `scale` with a common-mode offset below sigma; one patch row carries a 300 sigma element."""
    x = (rng.standard_normal((batch * tokens, dim)) * scale + rng.uniform(-0.8, 0.8, (batch * tokens, 1)) * scale).astype(np.float32)
    x[(batch - 1) * tokens + 1, dim // 3] = np.float32(300.0 * scale)
    return x
