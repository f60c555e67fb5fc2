"""The resize contract of the frames entry points (include/vithip.h, "8-bit frames") stated in numpy float64.

Per axis, with n the source length, [lo, hi) the box, S outputs, scale = (hi - lo) / S and sup = max(scale, 1), output i has
    centre   c = lo + (i + 0.5) scale
    taps     j in [max(floor(c - sup + 0.5), 0), min(floor(c + sup + 0.5), n))
    weights  w_j = max(0, 1 - |(j + 0.5 - c) / sup|), zero weights dropped, the rest divided by their sum (summed in tap order)
in double, each weight then rounded once to float32.  The horizontal pass runs first, then the vertical pass, with no rounding
between them; the byte is rint(min(max(v, 0), 255)).  The library accumulates both passes in fp32; resize_f64 below accumulates the
same float32 weights in float64, so what separates the two is the fp32 accumulation error alone."""
import math

import numpy as np

MAX_TAPS = 65
MAX_SCALE = 32


def axis_table(n, lo, hi, s):
    """first[s], count[s] (int32) and weights[s, MAX_TAPS] (float32, zero padded) of one axis."""
    lo, hi = float(lo), float(hi)
    assert 0.0 <= lo < hi <= n
    scale = (hi - lo) / s
    assert scale <= MAX_SCALE
    sup = max(scale, 1.0)
    first, count = np.zeros(s, np.int32), np.zeros(s, np.int32)
    weights = np.zeros((s, MAX_TAPS), np.float32)
    for i in range(s):
        c = lo + (i + 0.5) * scale
        j0 = max(math.floor(c - sup + 0.5), 0)
        j1 = min(math.floor(c + sup + 0.5), n)
        w = [max(0.0, 1.0 - abs((j + 0.5 - c) / sup)) for j in range(j0, j1)]
        nz = [k for k, v in enumerate(w) if v != 0.0]
        a, b = nz[0], nz[-1]
        w = w[a:b + 1]
        total = 0.0
        for v in w:          # in tap order, as the library sums
            total += v
        first[i], count[i] = j0 + a, len(w)
        weights[i, :len(w)] = np.array([v / total for v in w], dtype=np.float64).astype(np.float32)
    return first, count, weights


def _pass(src, first, count, weights):
    """src [n, ...] float64 -> [s, ...]: out[i] = sum_t weights[i, t] * src[first[i] + t]."""
    out = np.zeros((len(first),) + src.shape[1:], np.float64)
    for i in range(len(first)):
        k = int(count[i])
        w = weights[i, :k].astype(np.float64)
        out[i] = np.tensordot(w, src[first[i]:first[i] + k], axes=1)
    return out


def resize_f64(frame, box, s):
    """frame: [H, W, C] uint8 (or [H, W]); box (x0, y0, x1, y1) or None = the whole frame.  Returns the UNROUNDED float64 values
    [s, s, C] of the contract: horizontal pass, then vertical pass."""
    frame = np.asarray(frame)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, _ = frame.shape
    x0, y0, x1, y1 = (0.0, 0.0, float(w), float(h)) if box is None else [float(np.float32(v)) for v in box]   # the ABI carries float32
    xf, xc, xw = axis_table(w, x0, x1, s)
    yf, yc, yw = axis_table(h, y0, y1, s)
    hor = _pass(frame.astype(np.float64).transpose(1, 0, 2), xf, xc, xw)   # [s (x), H, C]
    return _pass(hor.transpose(1, 0, 2), yf, yc, yw)                        # [s (y), s (x), C]


def to_bytes(v64):
    return np.rint(np.clip(v64, 0.0, 255.0)).astype(np.uint8)
