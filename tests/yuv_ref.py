"""The contract of the planar YUV entry points (include/vithip.h, "Planar YUV frames") stated in numpy float64,
on top of nv12_ref (and, through it, frames_ref's axis table and pass).

A frame is three byte planes: Y [H, W] and U, V [ch, cw] with cw = ceil(W / sub_x), ch = ceil(H / sub_y), sub 1 or 2 per axis.
Each plane is resampled under the axis contract of the 8-bit frames: Y over the box as given, U and V each as a 1-channel image over
(lo / sub + delta, hi / sub + delta), delta = 0.25 on the horizontal axis only when sub_x == 2 and the siting is CHROMA_LEFT.  The
unrounded y, u, v pass the 3 x 4 matrix; the byte is rint(min(max(v, 0), 255)).  resize_yuv_f64 runs the float32 weights and
matrix entries in float64 (what separates it from the library is the fp32 accumulation alone); resize_yuv_f32 emulates the
library's own fmaf order in float32."""
import numpy as np

import nv12_ref as N

CHROMA_CENTER, CHROMA_LEFT = N.CHROMA_CENTER, N.CHROMA_LEFT
SUBSAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}


def chroma_size(h, w, sub_x, sub_y):
    """(ch, cw) by the ceiling rule of JPEG and ffmpeg."""
    return (h + sub_y - 1) // sub_y, (w + sub_x - 1) // sub_x


def chroma_box(box, sub_x, sub_y, site):
    """The box of the U and V planes, in chroma samples."""
    x0, y0, x1, y1 = box
    dx = 0.25 if (sub_x == 2 and site == CHROMA_LEFT) else 0.0
    return (x0 / sub_x + dx, y0 / sub_y, x1 / sub_x + dx, y1 / sub_y)


def tables(y, u, box, s, site, sub=None):
    """The four tables of one frame: luma x, luma y, chroma x, chroma y.  sub = (sub_x, sub_y); None: taken from the shapes (a side
    of 1 is then read as sub 1; the planes cannot tell, and the tables differ only in the box of a one-sample axis)."""
    h, w = y.shape
    ch, cw = u.shape
    sub_x, sub_y = subsampling(y.shape, u.shape) if sub is None else sub
    assert (ch, cw) == chroma_size(h, w, sub_x, sub_y)
    x0, y0, x1, y1 = N.box_of(y, box)
    cx0, cy0, cx1, cy1 = chroma_box((x0, y0, x1, y1), sub_x, sub_y, site)
    return (N.axis_table(w, x0, x1, s), N.axis_table(h, y0, y1, s), N.axis_table(cw, cx0, cx1, s), N.axis_table(ch, cy0, cy1, s))


def subsampling(y_shape, c_shape):
    h, w = y_shape
    ch, cw = c_shape
    sub = []
    for n, c in ((w, cw), (h, ch)):
        assert c in (n, (n + 1) // 2), (y_shape, c_shape)
        sub.append(1 if c == n else 2)
    return sub[0], sub[1]


def resample_f64(y, u, v, box, s, site, sub=None):
    """Unrounded float64 planes: Y [s, s] and UV [s, s, 2], horizontal pass then vertical pass."""
    tx, ty, tcx, tcy = tables(y, u, box, s, site, sub)
    yy = N.R._pass(N.R._pass(y.astype(np.float64).T, *tx).T, *ty)
    uv = np.stack([u, v], axis=-1).astype(np.float64)
    cc = N.R._pass(N.R._pass(uv.transpose(1, 0, 2), *tcx).transpose(1, 0, 2), *tcy)
    return yy, cc


def resize_yuv_f64(y, u, v, box, s, m, site, sub=None):
    """y [H, W], u and v [ch, cw] uint8, box in luma pixels (None = whole frame), m = 12 float32 entries.  Returns the UNROUNDED
    float64 values [s, s, 3] of the contract."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    assert u.shape == v.shape
    yy, cc = resample_f64(y, u, v, box, s, site, sub)
    return N.apply_matrix64(yy, cc, m)


def max_taps(y, u, box, s, site, sub=None):
    """(taps_y, taps_c): the largest tap count of the horizontal plus that of the vertical table, per plane."""
    tx, ty, tcx, tcy = tables(np.asarray(y), np.asarray(u), box, s, site, sub)
    return int(tx[1].max()) + int(ty[1].max()), int(tcx[1].max()) + int(tcy[1].max())


def resize_yuv_f32(y, u, v, box, s, m, site, sub=None):
    """The kernel's own order in float32 -> bytes [s, s, 3]."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    tx, ty, tcx, tcy = tables(y, u, box, s, site, sub)
    yy = N._pass32(np.ascontiguousarray(N._pass32(y.astype(np.float32).T, *tx).T), *ty)
    uv = np.stack([u, v], axis=-1).astype(np.float32)
    cc = N._pass32(np.ascontiguousarray(N._pass32(uv.transpose(1, 0, 2), *tcx).transpose(1, 0, 2)), *tcy)
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    out = np.empty((s, s, 3), np.float32)
    for k in range(3):
        b = lambda t: np.broadcast_to(t, yy.shape)
        out[..., k] = N._fma32(b(m[k, 0]), yy, N._fma32(b(m[k, 1]), cc[..., 0], N._fma32(b(m[k, 2]), cc[..., 1], b(m[k, 3]))))
    return np.rint(np.clip(out, 0.0, 255.0)).astype(np.uint8)


# ---- test inputs ----------------------------------------------------------------------------------------------------------------
def rgb_to_yuv_planes(rgb, sub_x, sub_y, standard=N.BT709, full_range=False):
    """Test-only: [H, W, 3] uint8, any H and W -> (Y [H, W], U [ch, cw], V [ch, cw]) uint8 through the inverse matrix; a chroma sample
    is the mean of the luma positions it covers (an odd last row / column covers one)."""
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    m = N.yuv_matrix64(standard, full_range)
    inv = np.linalg.inv(m[:, :3])
    yuv = (rgb.astype(np.float64) - m[:, 3]) @ inv.T
    y = np.rint(np.clip(yuv[..., 0], 0, 255)).astype(np.uint8)
    ch, cw = chroma_size(h, w, sub_x, sub_y)
    c = yuv[..., 1:]
    c = np.pad(c, ((0, ch * sub_y - h), (0, cw * sub_x - w), (0, 0)), mode="edge")
    c = c.reshape(ch, sub_y, cw, sub_x, 2).mean(axis=(1, 3))
    c = np.rint(np.clip(c, 0, 255)).astype(np.uint8)
    return y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1])


def interleave(u, v):
    """U, V [ch, cw] -> NV12's UV plane [ch, cw, 2]."""
    return np.ascontiguousarray(np.stack([u, v], axis=-1))
