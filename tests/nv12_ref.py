"""The contract of the NV12 entry points (include/vithip.h, "NV12 frames") stated in numpy float64, on top of
frames_ref's axis table and pass.

Each plane is resampled under the axis contract of the 8-bit frames: Y over the box as given, UV as a 2-channel image of
width/2 x height/2 over (lo / 2 + delta, hi / 2 + delta), delta = 0.25 horizontally for left-sited chroma and 0 otherwise.  The
unrounded y, u, v then pass the 3 x 4 matrix; the byte is rint(min(max(v, 0), 255)).  The library accumulates the passes and the
matrix in fp32; resize_nv12_f64 runs the same float32 weights and matrix entries in float64, so what separates the two is the fp32
accumulation error alone.  resize_nv12_f32 emulates the library's own fmaf order in float32."""
import math

import numpy as np

import frames_ref as R

CHROMA_CENTER, CHROMA_LEFT = 0, 1
BT601, BT709, BT2020 = 0, 1, 2
KR_KB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}


def yuv_matrix64(standard, full_range):
    """The matrix in float64, in the expression order the header states; rows R, G, B, columns y, u, v, 1."""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    sy, sc, oy = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    rv = 2.0 * (1.0 - kr) * sc
    bu = 2.0 * (1.0 - kb) * sc
    gu = -(2.0 * kb * (1.0 - kb) / kg) * sc
    gv = -(2.0 * kr * (1.0 - kr) / kg) * sc
    yo = -(sy * oy)
    return np.array([[sy, 0.0, rv, yo - 128.0 * rv],
                     [sy, gu, gv, yo - 128.0 * gu - 128.0 * gv],
                     [sy, bu, 0.0, yo - 128.0 * bu]], dtype=np.float64)


def yuv_matrix(standard, full_range):
    """yuv_matrix64 followed by the one rounding to float32."""
    return yuv_matrix64(standard, full_range).astype(np.float32)


def axis_table(n, lo, hi, s):
    """frames_ref.axis_table, and the same statement for a box that overhangs the last sample (left-sited chroma, by at most a
    quarter of a sample): the tap clamp min(.., n) and the renormalisation are what takes the overhang."""
    lo, hi = float(lo), float(hi)
    if hi <= n:
        return R.axis_table(n, lo, hi, s)
    assert 0.0 <= lo < hi <= n + 0.25
    scale = (hi - lo) / s
    assert scale <= R.MAX_SCALE
    sup = max(scale, 1.0)
    first, count = np.zeros(s, np.int32), np.zeros(s, np.int32)
    weights = np.zeros((s, R.MAX_TAPS), np.float32)
    for i in range(s):
        c = lo + (i + 0.5) * scale
        j0 = max(math.floor(c - sup + 0.5), 0)
        j1 = min(math.floor(c + sup + 0.5), n)
        w = [max(0.0, 1.0 - abs((j + 0.5 - c) / sup)) for j in range(j0, j1)]
        nz = [k for k, v in enumerate(w) if v != 0.0]
        a, b = nz[0], nz[-1]
        w = w[a:b + 1]
        total = 0.0
        for v in w:
            total += v
        first[i], count[i] = j0 + a, len(w)
        weights[i, :len(w)] = np.array([v / total for v in w], dtype=np.float64).astype(np.float32)
    return first, count, weights


def box_of(y, box):
    h, w = y.shape
    return (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(np.float32(v)) for v in box)   # the ABI carries float32


def tables(y, box, s, site):
    """The four tables of one frame: luma x, luma y, chroma x, chroma y."""
    h, w = y.shape
    x0, y0, x1, y1 = box_of(y, box)
    dx = 0.25 if site == CHROMA_LEFT else 0.0
    return (axis_table(w, x0, x1, s), axis_table(h, y0, y1, s),
            axis_table(w // 2, x0 / 2.0 + dx, x1 / 2.0 + dx, s), axis_table(h // 2, y0 / 2.0, y1 / 2.0, s))


def resample_f64(y, uv, box, s, site):
    """Unrounded float64 planes: Y [s, s] and UV [s, s, 2], horizontal pass then vertical pass."""
    tx, ty, tcx, tcy = tables(y, box, s, site)
    yy = R._pass(R._pass(y.astype(np.float64).T, *tx).T, *ty)
    cc = R._pass(R._pass(uv.astype(np.float64).transpose(1, 0, 2), *tcx).transpose(1, 0, 2), *tcy)
    return yy, cc


def apply_matrix64(yy, cc, m):
    m = np.asarray(m, dtype=np.float32).reshape(3, 4).astype(np.float64)
    return np.stack([m[k, 0] * yy + m[k, 1] * cc[..., 0] + m[k, 2] * cc[..., 1] + m[k, 3] for k in range(3)], axis=-1)


def resize_nv12_f64(y, uv, box, s, m, site):
    """y [H, W] uint8, uv [H/2, W/2, 2] uint8, box in luma pixels (None = whole frame), m = 12 float32 entries.  Returns the
    UNROUNDED float64 values [s, s, 3] of the contract."""
    y, uv = np.asarray(y), np.asarray(uv)
    yy, cc = resample_f64(y, uv, box, s, site)
    return apply_matrix64(yy, cc, m)


def max_taps(y, box, s, site):
    """(taps_y, taps_c): the largest tap count of the horizontal plus that of the vertical table, per plane."""
    tx, ty, tcx, tcy = tables(np.asarray(y), box, s, site)
    return int(tx[1].max()) + int(ty[1].max()), int(tcx[1].max()) + int(tcy[1].max())


# ---- the library's arithmetic in float32 ----------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32
    (a double rounding that differs from a true fmaf only on a float64 tie, about one value in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _pass32(src, first, count, weights):
    """src [n, ...] float32 -> [s, ...] float32: acc = fmaf(w[t], src[first + t], acc) in ascending tap order from 0."""
    out = np.zeros((len(first),) + src.shape[1:], np.float32)
    for i in range(len(first)):
        acc = np.zeros(src.shape[1:], np.float32)
        for t in range(int(count[i])):
            acc = _fma32(np.broadcast_to(weights[i, t], acc.shape), src[first[i] + t], acc)
        out[i] = acc
    return out


def resize_nv12_f32(y, uv, box, s, m, site):
    """The kernel's own order in float32 -> bytes [s, s, 3]."""
    y, uv = np.asarray(y), np.asarray(uv)
    tx, ty, tcx, tcy = tables(y, box, s, site)
    yy = _pass32(np.ascontiguousarray(_pass32(y.astype(np.float32).T, *tx).T), *ty)
    cc = _pass32(np.ascontiguousarray(_pass32(uv.astype(np.float32).transpose(1, 0, 2), *tcx).transpose(1, 0, 2)), *tcy)
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    out = np.empty((s, s, 3), np.float32)
    for k in range(3):
        b = lambda v: np.broadcast_to(v, yy.shape)
        out[..., k] = _fma32(b(m[k, 0]), yy, _fma32(b(m[k, 1]), cc[..., 0], _fma32(b(m[k, 2]), cc[..., 1], b(m[k, 3]))))
    return np.rint(np.clip(out, 0.0, 255.0)).astype(np.uint8)


def margin(taps_y, taps_c):
    """fp32 accumulation bound of the two fmaf chains per plane plus the matrix, scaled by the largest absolute row sum of a
    video matrix (about 3.3), on the 0..255 scale."""
    return max(1e-3, 3.3 * (taps_y + taps_c + 4) * 255 * 2.0 ** -24)


# ---- test inputs ----------------------------------------------------------------------------------------------------------------
def rgb_to_nv12(rgb, standard=BT709, full_range=False):
    """Test-only: [H, W, 3] uint8 (even H, W) -> (Y [H, W], UV [H/2, W/2, 2]) uint8 through the inverse matrix and a 2 x 2 chroma
    mean."""
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    assert h % 2 == 0 and w % 2 == 0
    m = yuv_matrix64(standard, full_range)
    inv = np.linalg.inv(m[:, :3])
    yuv = (rgb.astype(np.float64) - m[:, 3]) @ inv.T
    y = np.rint(np.clip(yuv[..., 0], 0, 255)).astype(np.uint8)
    c = yuv[..., 1:].reshape(h // 2, 2, w // 2, 2, 2).mean(axis=(1, 3))
    return y, np.rint(np.clip(c, 0, 255)).astype(np.uint8)
