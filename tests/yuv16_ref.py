"""The 16-bit side of the YUV contract (include/vithip.h, "16-bit YUV frames") in numpy float64.

The resampling and the conversion are nv12_ref's and yuv_ref's, which take uint16 planes unchanged (a word enters as the value of
its integer); what is new is the matrix of a depth and an alignment, the error margin for words larger than 255, and a maker of
N-bit test planes."""
import numpy as np

import nv12_ref as N
import yuv_ref as Y


def yuv_matrix16_64(standard, full_range, bits, msb_aligned):
    """vh_yuv_matrix16 in float64, in the expression order the header states; rows R, G, B, columns y, u, v, 1."""
    kr, kb = N.KR_KB[standard]
    kg = 1.0 - kr - kb
    a = 2.0 ** (16 - bits) if msb_aligned else 1.0
    q = 2.0 ** (bits - 8)
    if full_range:
        sy = sc = 255.0 / ((2.0 ** bits - 1.0) * a)
        oy = 0.0
    else:
        sy, sc, oy = 255.0 / (219.0 * q * a), 255.0 / (224.0 * q * a), 16.0 * q * a
    mid = 2.0 ** (bits - 1) * a
    rv = 2.0 * (1.0 - kr) * sc
    bu = 2.0 * (1.0 - kb) * sc
    gu = -(2.0 * kb * (1.0 - kb) / kg) * sc
    gv = -(2.0 * kr * (1.0 - kr) / kg) * sc
    yo = -(sy * oy)
    return np.array([[sy, 0.0, rv, yo - mid * rv],
                     [sy, gu, gv, yo - mid * gu - mid * gv],
                     [sy, bu, 0.0, yo - mid * bu]], dtype=np.float64)


def yuv_matrix16(standard, full_range, bits, msb_aligned):
    """yuv_matrix16_64 followed by the one rounding to float32."""
    return yuv_matrix16_64(standard, full_range, bits, msb_aligned).astype(np.float32)


def largest_word(bits, msb_aligned):
    return (2 ** bits - 1) << (16 - bits if msb_aligned else 0)


def margin(m, taps_y, taps_c, vmax):
    """nv12_ref.margin with 3.3 x 255 replaced by what it stood for: the largest absolute row sum A of the matrix's first three
    columns times the largest word V of the format, i.e. the magnitude the fp32 chains carry on the output's 0..255 scale."""
    a = float(np.abs(np.asarray(m, np.float64).reshape(3, 4)[:, :3]).sum(axis=1).max())
    return max(1e-3, a * (taps_y + taps_c + 4) * vmax * 2.0 ** -24)


def statement_figures(got, planes, box, s, m, site, sub, vmax):
    """(largest |byte - clamp(v64)|, its bound, share of bytes equal to rint(clamp(v64))) of one planar frame of uint16 planes."""
    v64 = np.clip(Y.resize_yuv_f64(*planes, box, s, m, site, sub), 0.0, 255.0)
    bound = 0.5 + margin(m, *Y.max_taps(planes[0], planes[1], box, s, site, sub), vmax)
    err = float(np.abs(got.astype(np.float64) - v64).max())
    same = float((got == np.rint(v64).astype(np.uint8)).mean())
    return err, bound, same


# ---- test inputs ----------------------------------------------------------------------------------------------------------------
def rgb_to_yuv16_planes(rgb, sub_x, sub_y, bits, msb_aligned, standard=N.BT709, full_range=False):
    """Test-only: [H, W, 3] uint8, any H and W -> (Y [H, W], U [ch, cw], V [ch, cw]) uint16 words holding `bits`-bit codes: through
    the inverse of the LSB-aligned matrix, a chroma sample the mean of the luma positions it covers (yuv_ref.rgb_to_yuv_planes),
    rounded and clipped to the code range, then shifted into the high bits for MSB alignment."""
    rgb = np.asarray(rgb)
    h, w, _ = rgb.shape
    m = yuv_matrix16_64(standard, full_range, bits, False)
    inv = np.linalg.inv(m[:, :3])
    yuv = (rgb.astype(np.float64) - m[:, 3]) @ inv.T
    top = 2 ** bits - 1
    ch, cw = Y.chroma_size(h, w, sub_x, sub_y)
    c = yuv[..., 1:]
    c = np.pad(c, ((0, ch * sub_y - h), (0, cw * sub_x - w), (0, 0)), mode="edge")
    c = c.reshape(ch, sub_y, cw, sub_x, 2).mean(axis=(1, 3))
    shift = 16 - bits if msb_aligned else 0
    code = lambda t: (np.rint(np.clip(t, 0, top)).astype(np.uint16) << shift).astype(np.uint16)
    return code(yuv[..., 0]), np.ascontiguousarray(code(c[..., 0])), np.ascontiguousarray(code(c[..., 1]))
