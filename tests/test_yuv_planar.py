"""CPU suite of the planar YUV entry points (include/vithip.h, "Planar YUV frames"): every refusal decided on the
host with its own message, the binding's layout, the packing, and yuv_ref's fp32 emulation of the kernel's fmaf order against the
NV12 emulation (byte for byte) and against the bounds the GPU suite asserts."""
import ctypes as C

import numpy as np
import pytest

import nv12_ref as N
import vithip
import yuv_ref as Y
from test_nv12 import make_nv12, make_rgb
from vh_testlib import last_error

VH_ERR_INVALID = 1
COLOURS = {"bt709_limited_left": (N.BT709, False, N.CHROMA_LEFT), "bt601_full_centre": (N.BT601, True, N.CHROMA_CENTER)}
SUBS = Y.SUBSAMPLINGS

# (h, w, box, S): the smallest shapes that reach each path; every one runs at all four sub-samplings
OP_CASES = {
    "odd_37x53_16": (37, 53, None, 16),                                           # odd sides: the last chroma row and column half covered
    "odd_37x53_box_16": (37, 53, (0.0, 0.0, 52.0, 37.0), 16),                     # ... and a box that ends on a chroma sample boundary
    "down_38x54_16": (38, 54, None, 16),                                          # non-integer down-scale; left siting overhangs by 0.25
    "up_20x24_32": (20, 24, None, 32),                                            # up-scale: one chroma row feeds four output rows
    "fractional_box_98x132_28": (98, 132, (10.25, 5.5, 101.75, 95.125), 28),      # fractional box
    "taps29_270x480_32": (270, 480, None, 32),                                    # 29 luma taps
    "one_pixel_4": (1, 1, None, 4),                                               # degenerate sizes
    "two_by_two_4": (2, 2, None, 4),
}


def make_yuv(h, w, sub, seed):
    """(Y, U, V) planes of a synthetic picture (test_nv12.make_rgb) at sub = (sub_x, sub_y), any h and w."""
    return Y.rgb_to_yuv_planes(make_rgb(h, w, seed), *sub)


# ---- refusals without a device --------------------------------------------------------------------------------------------------
def one_yuv(h=41, w=61, sub=(2, 2), y_stride=None, u_stride=None, v_stride=None, y_off=0, u_off=None, v_off=None, box=None):
    d = (vithip.FrameYUV * 1)()
    ch, cw = Y.chroma_size(h, w, max(sub[0], 1), max(sub[1], 1))
    d[0].height, d[0].width, d[0].sub_x, d[0].sub_y = h, w, sub[0], sub[1]
    d[0].y_stride = w if y_stride is None else y_stride
    d[0].u_stride = cw if u_stride is None else u_stride
    d[0].v_stride = cw if v_stride is None else v_stride
    d[0].y_offset = y_off
    d[0].u_offset = y_off + h * d[0].y_stride if u_off is None else u_off
    d[0].v_offset = d[0].u_offset + ch * d[0].u_stride if v_off is None else v_off
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def test_every_refusal_is_decided_on_the_host_with_its_own_message():
    """vh_op_resize_yuv checks and plans before its first device call: a bad argument is VH_ERR_INVALID whether or not a device
    exists, and the pointers (0x1000 here) are never read (so no call here is a valid one)."""
    L = vithip.lib()
    fake = C.c_void_p(0x1000)
    m709 = np.ascontiguousarray(vithip.yuv_matrix().reshape(-1))
    full = 41 * 61 + 2 * 21 * 31                                                       # 41 x 61 at 4:2:0: chroma 21 x 31

    def rc(d, nbytes=full, s=16, batch=1, m=m709, site=vithip.CHROMA_LEFT):
        return L.vh_op_resize_yuv(fake, nbytes, C.addressof(d), batch, s, m.ctypes.data, site, fake, None)

    ok = one_yuv()
    bad = {                                                                            # rule -> (descriptor, a word of its message)
        "zero width": (one_yuv(w=0), "1..8192"),
        "width 8193": (one_yuv(w=8193), "1..8192"),
        "zero height": (one_yuv(h=0), "1..8192"),
        "height 8193": (one_yuv(h=8193), "1..8192"),
        "sub_x 0": (one_yuv(sub=(0, 2)), "sub_x and sub_y"),
        "sub_x 3": (one_yuv(sub=(3, 2)), "sub_x and sub_y"),
        "sub_y 4": (one_yuv(sub=(2, 4)), "sub_x and sub_y"),
        "sub_y -1": (one_yuv(sub=(1, -1)), "sub_x and sub_y"),
        "y_stride < width": (one_yuv(y_stride=60), "y_stride < width"),
        "u_stride < cw": (one_yuv(u_stride=30), "u_stride or v_stride"),
        "v_stride < cw": (one_yuv(v_stride=30), "u_stride or v_stride"),
        "u_stride = width / 2 rounded down at 4:2:2": (one_yuv(sub=(2, 1), u_stride=30), "u_stride or v_stride"),
        "empty box": (one_yuv(box=(5.0, 0.0, 5.0, 41.0)), "box outside the frame, or empty"),
        "box beyond the frame": (one_yuv(box=(0.0, 0.0, 61.5, 41.0)), "box outside the frame, or empty"),
        "negative box": (one_yuv(box=(0.0, -0.5, 61.0, 41.0)), "box outside the frame, or empty"),
        "nan box": (one_yuv(box=(float("nan"), 0.0, 61.0, 41.0)), "box outside the frame, or empty"),
    }
    for why, (d, word) in bad.items():
        assert rc(d, nbytes=1 << 30) == VH_ERR_INVALID, why
        assert word in last_error(), (why, last_error())
    # each plane's last byte beyond nbytes, with the plane named
    assert rc(ok, nbytes=full - 1) == VH_ERR_INVALID and "a V plane ends beyond nbytes" in last_error()
    assert rc(one_yuv(u_off=full - 651, v_off=41 * 61), nbytes=full - 1) == VH_ERR_INVALID and "a U plane ends beyond nbytes" in last_error()
    assert rc(one_yuv(y_off=1302, u_off=0, v_off=651), nbytes=full - 1) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    assert rc(one_yuv(y_off=1 << 40), nbytes=full) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    # at 4:4:4 the chroma planes are full size
    assert rc(one_yuv(sub=(1, 1)), nbytes=3 * 41 * 61 - 1) == VH_ERR_INVALID and "a V plane ends beyond nbytes" in last_error()
    # scale > 32 on an axis
    assert rc(one_yuv(h=1041, w=17), nbytes=1 << 30, s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    assert rc(one_yuv(h=17, w=1041), nbytes=1 << 30, s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    for i in (0, 5, 11):
        for v in (np.inf, -np.inf, np.nan):
            m = m709.copy()
            m[i] = v
            assert rc(ok, m=m) == VH_ERR_INVALID and "not finite" in last_error()
    assert rc(ok, site=2) == VH_ERR_INVALID and rc(ok, site=-1) == VH_ERR_INVALID
    assert rc(ok, batch=0) == VH_ERR_INVALID and rc(ok, s=0) == VH_ERR_INVALID and rc(ok, s=4097) == VH_ERR_INVALID
    for args in ((None, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, fake, None), (fake, full, None, 1, 16, m709.ctypes.data, 1, fake, None),
                 (fake, full, C.addressof(ok), 1, 16, None, 1, fake, None), (fake, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, None, None)):
        assert L.vh_op_resize_yuv(*args) == VH_ERR_INVALID and "null" in last_error()


def test_yuv_calls_without_a_context_are_refused():
    L = vithip.lib()
    d = one_yuv()
    buf, out = np.zeros(4000, np.uint8), np.zeros(8, np.float32)
    assert L.vh_forward_frames_yuv(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    assert L.vh_forward_device_frames_yuv(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    assert L.vh_ring_submit_frames_yuv(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1) == VH_ERR_INVALID


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_frame_yuv_layout_is_the_header_s():
    """include/vithip.h: sizeof 72; y_offset 0, u_offset 8, v_offset 16, height 24, width 28, y_stride 32, u_stride 36, v_stride 40,
    sub_x 44, sub_y 48, box 52, reserved 68."""
    F = vithip.FrameYUV
    assert C.sizeof(F) == 72
    want = dict(y_offset=0, u_offset=8, v_offset=16, height=24, width=28, y_stride=32, u_stride=36, v_stride=40, sub_x=44, sub_y=48,
                box=52, reserved=68)
    assert {n: getattr(F, n).offset for n, _ in F._fields_} == want
    import os, re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vithip.h")).read()
    assert "sizeof(vh_frame_yuv) == 72" in hdr
    body = re.search(r"typedef struct vh_frame_yuv \{(.*?)\} vh_frame_yuv;", hdr, re.S).group(1)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [n for n, _ in F._fields_]


def test_pack_frames_yuv_infers_the_subsampling_from_the_shapes():
    rng = np.random.default_rng(5)
    plane = lambda h, w: rng.integers(0, 256, (h, w), dtype=np.uint8)
    frames = {(1, 1): (plane(37, 53), plane(37, 53), plane(37, 53)),               # odd sizes at every sub-sampling
              (2, 1): (plane(37, 53), plane(37, 27), plane(37, 27)),
              (2, 2): (plane(37, 53), plane(19, 27), plane(19, 27)),
              (1, 2): (plane(37, 53), plane(19, 53), plane(19, 53)),
              "even 420": (plane(6, 8), plane(3, 4), plane(3, 4))}
    boxes = [None, (1.0, 0.5, 9.0, 3.5), None, None, None]
    buf, desc = vithip.pack_frames_yuv(list(frames.values()), boxes)
    off = 0
    for d, (key, (y, u, v)), box in zip(desc, frames.items(), boxes):
        h, w = y.shape
        ch, cw = u.shape
        assert (d.sub_x, d.sub_y) == (key if isinstance(key, tuple) else (2, 2))
        assert (d.y_offset, d.u_offset, d.v_offset) == (off, off + h * w, off + h * w + ch * cw)
        assert (d.height, d.width, d.y_stride, d.u_stride, d.v_stride) == (h, w, w, cw, cw)
        assert list(d.box) == ([0.0, 0.0, float(w), float(h)] if box is None else list(box))
        assert np.array_equal(buf[d.y_offset:d.y_offset + h * w].reshape(h, w), y)
        assert np.array_equal(buf[d.u_offset:d.u_offset + ch * cw].reshape(ch, cw), u)
        assert np.array_equal(buf[d.v_offset:d.v_offset + ch * cw].reshape(ch, cw), v)
        off += h * w + 2 * ch * cw
    assert buf.dtype == np.uint8 and buf.size == off
    z = lambda h, w: np.zeros((h, w), np.uint8)
    for bad in ((z(37, 53), z(18, 27), z(18, 27)),         # floor instead of ceiling
                (z(37, 53), z(19, 26), z(19, 26)),
                (z(37, 53), z(19, 27), z(19, 53)),         # U and V differ
                (z(36, 52), z(9, 13), z(9, 13)),           # 4:1:0
                (z(36, 52), z(36, 13), z(36, 13))):        # 4:1:1
        with pytest.raises(ValueError):
            vithip.pack_frames_yuv([bad])
    with pytest.raises(TypeError):
        vithip.pack_frames_yuv([(z(6, 8).astype(np.float32), z(3, 4), z(3, 4))])
    with pytest.raises(TypeError):
        vithip.pack_frames_yuv([(z(6, 8), np.zeros((3, 4, 2), np.uint8))])           # an NV12 pair
    with pytest.raises(ValueError):
        vithip.pack_frames_yuv([frames[(2, 2)]], [None, None])


# ---- the emulation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", [N.CHROMA_CENTER, N.CHROMA_LEFT], ids=["centre", "left"])
@pytest.mark.parametrize("name", [n for n, c in OP_CASES.items() if c[0] % 2 == 0 and c[1] % 2 == 0])
def test_i420_emulation_equals_the_nv12_emulation(name, site):
    h, w, box, s = OP_CASES[name]
    y, uv = make_nv12(h, w, seed=h + w)
    u, v = np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
    for std, full in ((N.BT709, False), (N.BT601, True)):
        m = N.yuv_matrix(std, full)
        want = N.resize_nv12_f32(y, uv, box, s, m, site)
        assert np.array_equal(Y.resize_yuv_f32(y, u, v, box, s, m, site, (2, 2)), want)
        # YV12 read as I420 with the matrix's chroma columns exchanged: the G row then adds its two chroma terms in the other order,
        # which is the same byte on these inputs, not by construction (the GPU suite asserts the same tie)
        assert np.array_equal(Y.resize_yuv_f32(y, v, u, box, s, m[:, [0, 2, 1, 3]], site, (2, 2)), want)
    assert np.array_equal(Y.resize_yuv_f64(y, u, v, box, s, m, site, (2, 2)), N.resize_nv12_f64(y, uv, box, s, m, site))


def statement_figures(got, planes, box, s, m, site, sub):
    """(largest |byte - clamp(v64)|, its bound, share of bytes equal to rint(clamp(v64))) of one frame: the two conditions of
    the GPU suite.  The contract clamps before it rounds, and the clamp is 1-Lipschitz, so the bound is that of the unclamped
    arithmetic."""
    v64 = np.clip(Y.resize_yuv_f64(*planes, box, s, m, site, sub), 0.0, 255.0)
    margin = N.margin(*Y.max_taps(planes[0], planes[1], box, s, site, sub))
    err = float(np.abs(got.astype(np.float64) - v64).max())
    same = float((got == np.rint(v64).astype(np.uint8)).mean())
    return err, 0.5 + margin, same


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_fp32_emulation_meets_the_gpu_bounds(name, sub, colour):
    h, w, box, s = OP_CASES[name]
    std, full, site = COLOURS[colour]
    planes = make_yuv(h, w, SUBS[sub], seed=h + w)
    m = N.yuv_matrix(std, full)
    got = Y.resize_yuv_f32(*planes, box, s, m, site, SUBS[sub])
    err, bound, same = statement_figures(got, planes, box, s, m, site, SUBS[sub])
    print(f"emulated yuv{sub} {h}x{w} box {box} -> {s} {colour}: max |byte - v64| = {err:.6f} (bound {bound:.6f}), {100 * same:.3f} % equal rint(v64)")
    assert err <= bound
    assert same >= 0.995
