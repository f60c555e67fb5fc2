"""CPU suite of the NV12 entry points (include/vithip.h, "NV12 frames"): the colour matrix bit for bit, the
float64 statement against torch, every refusal decided on the host, the binding's layout, and the fp32 emulation of the kernel's
fmaf order against the bounds the GPU suite asserts."""
import ctypes as C

import numpy as np
import pytest

import nv12_ref as N
import vithip

VH_ERR_INVALID = 1
STANDARDS = [(N.BT601, "bt601"), (N.BT709, "bt709"), (N.BT2020, "bt2020")]


def make_rgb(h, w, seed):
    """Smooth structure plus noise, as test_gpu_frames.make_frame: a shifted or transposed result is far from the reference."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 96.0 + 80.0 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0) + 0.11 * x - 0.07 * y
    img = base[:, :, None] + 13.0 * np.arange(3)[None, None, :] + rng.normal(0.0, 40.0, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make_nv12(h, w, seed):
    return N.rgb_to_nv12(make_rgb(h, w, seed))


def convert_bytes(m, yuv):
    """The contract's conversion of one (y, u, v) triple in float32 fmaf order -> three bytes."""
    m = np.asarray(m, np.float32).reshape(3, 4)
    y, u, v = (np.float32(t) for t in yuv)
    out = [N._fma32(m[k, 0], y, N._fma32(m[k, 1], u, N._fma32(m[k, 2], v, m[k, 3]))) for k in range(3)]
    return [int(np.rint(min(max(float(o), 0.0), 255.0))) for o in out]


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standard,name", STANDARDS)
@pytest.mark.parametrize("full", [False, True])
def test_yuv_matrix_is_the_float64_formula_rounded_once(standard, name, full):
    got = vithip.yuv_matrix(standard, full)
    want = N.yuv_matrix(standard, full)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    if full:
        for y in (0, 1, 77, 128, 254, 255):
            assert convert_bytes(got, (y, 128, 128)) == [y, y, y]
    else:
        assert convert_bytes(got, (16, 128, 128)) == [0, 0, 0]
        assert convert_bytes(got, (235, 128, 128)) == [255, 255, 255]


def test_yuv_matrix_anchors_and_refusals():
    r, g, b = convert_bytes(vithip.yuv_matrix(vithip.YUV_BT709, False), (63, 102, 240))   # BT.709 limited-range red
    assert abs(r - 255) <= 1 and g <= 1 and b <= 1
    L = vithip.lib()
    m = np.zeros(12, np.float32)
    assert L.vh_yuv_matrix(3, 0, m.ctypes.data) == VH_ERR_INVALID
    assert L.vh_yuv_matrix(-1, 0, m.ctypes.data) == VH_ERR_INVALID
    assert L.vh_yuv_matrix(1, 2, m.ctypes.data) == VH_ERR_INVALID
    assert L.vh_yuv_matrix(1, 0, None) == VH_ERR_INVALID


# ---- the statement against an independent implementation ------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 48), (64, 64)])
def test_statement_equals_torch_bilinear_chroma_upsample(h, w):
    """At S = width = height (the whole frame, scale 1) and centre siting the luma pass is the identity and our chroma pass is a 2x
    up-sample with two taps: torch's bilinear interpolate (align_corners=False).  1e-3 on the 0..255 scale bounds torch's fp32
    arithmetic (a few ulp x 255 x the largest row sum of |m|, about 3.3), not ours."""
    import torch
    y, uv = make_nv12(h, w, seed=h + w)
    m = vithip.yuv_matrix(vithip.YUV_BT709, False)
    # the output is S x S: of the 32 x 48 frame the box is the left 32 x 32 (its chroma taps still reach into the rest of the frame,
    # so torch up-samples the whole plane and the same columns are cut out afterwards)
    s = min(h, w)
    yy, cc = N.resample_f64(y, uv, (0.0, 0.0, float(s), float(s)), s, N.CHROMA_CENTER)
    assert np.array_equal(yy, y[:s, :s].astype(np.float64))
    t = torch.from_numpy(uv.astype(np.float32)).permute(2, 0, 1)[None]
    up = torch.nn.functional.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    want = N.apply_matrix64(y[:s, :s].astype(np.float64), up[:s, :s].astype(np.float64), m)
    got = N.apply_matrix64(yy, cc, m)
    err = float(np.abs(got - want).max())
    print(f"statement vs torch at {h}x{w}: max |d| = {err:.3e}")
    assert err <= 1e-3


# ---- refusals without a device --------------------------------------------------------------------------------------------------
def one_nv12(h=40, w=60, y_stride=None, uv_stride=None, y_off=0, uv_off=None, box=None):
    d = (vithip.FrameNV12 * 1)()
    d[0].height, d[0].width = h, w
    d[0].y_stride = w if y_stride is None else y_stride
    d[0].uv_stride = w if uv_stride is None else uv_stride
    d[0].y_offset = y_off
    d[0].uv_offset = y_off + h * d[0].y_stride if uv_off is None else uv_off
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def test_every_refusal_is_decided_on_the_host():
    """vh_op_resize_nv12 checks and plans before its first device call: a bad argument is VH_ERR_INVALID whether or not a device
    exists, and the pointers (0x1000 here) are never read."""
    L = vithip.lib()
    fake = C.c_void_p(0x1000)
    m709 = np.ascontiguousarray(vithip.yuv_matrix().reshape(-1))
    full = 40 * 60 * 3 // 2

    def rc(d, nbytes=full, s=16, batch=1, m=m709, site=vithip.CHROMA_LEFT):
        return L.vh_op_resize_nv12(fake, nbytes, C.addressof(d), batch, s, m.ctypes.data, site, fake, None)

    bad = {
        "odd width": one_nv12(w=59, y_stride=60, uv_stride=60),
        "odd height": one_nv12(h=39),
        "y_stride < width": one_nv12(y_stride=59, uv_off=2400),
        "uv_stride < width": one_nv12(uv_stride=59),
        "empty box": one_nv12(box=(5.0, 0.0, 5.0, 40.0)),
        "box beyond the frame": one_nv12(box=(0.0, 0.0, 60.5, 40.0)),
        "negative box": one_nv12(box=(-0.5, 0.0, 60.0, 40.0)),
        "nan box": one_nv12(box=(float("nan"), 0.0, 60.0, 40.0)),
        "zero width": one_nv12(w=0),
        "width 8194": one_nv12(w=8194),
    }
    for why, d in bad.items():
        assert rc(d, nbytes=1 << 30) == VH_ERR_INVALID, why
    ok = one_nv12()
    assert rc(ok, nbytes=full - 1) == VH_ERR_INVALID                                   # the UV plane ends beyond nbytes
    assert rc(one_nv12(uv_off=0, y_off=1200), nbytes=full - 1) == VH_ERR_INVALID       # the Y plane ends beyond nbytes
    assert rc(one_nv12(y_off=1 << 31), nbytes=full) == VH_ERR_INVALID
    assert rc(one_nv12(h=1040, w=16), nbytes=1 << 30, s=32) == VH_ERR_INVALID          # scale 32.5 > 32
    for i in (0, 5, 11):
        for v in (np.inf, -np.inf, np.nan):
            m = m709.copy()
            m[i] = v
            assert rc(ok, m=m) == VH_ERR_INVALID
    assert rc(ok, site=2) == VH_ERR_INVALID and rc(ok, site=-1) == VH_ERR_INVALID
    assert rc(ok, batch=0) == VH_ERR_INVALID and rc(ok, s=0) == VH_ERR_INVALID and rc(ok, s=4097) == VH_ERR_INVALID
    assert L.vh_op_resize_nv12(None, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, fake, None) == VH_ERR_INVALID
    assert L.vh_op_resize_nv12(fake, full, None, 1, 16, m709.ctypes.data, 1, fake, None) == VH_ERR_INVALID
    assert L.vh_op_resize_nv12(fake, full, C.addressof(ok), 1, 16, None, 1, fake, None) == VH_ERR_INVALID
    assert L.vh_op_resize_nv12(fake, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, None, None) == VH_ERR_INVALID


def test_nv12_calls_without_a_context_are_refused():
    L = vithip.lib()
    d = one_nv12()
    buf, out, m = np.zeros(3600, np.uint8), np.zeros(8, np.float32), np.zeros(12, np.float32)
    assert L.vh_forward_frames_nv12(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    assert L.vh_forward_device_frames_nv12(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    assert L.vh_ring_submit_frames_nv12(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1) == VH_ERR_INVALID
    assert L.vh_set_frame_colour(None, m.ctypes.data, 0) == VH_ERR_INVALID
    assert L.vh_get_frame_colour(None, m.ctypes.data, None) == VH_ERR_INVALID


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_pack_frames_nv12_lays_out_offsets_and_strides():
    assert C.sizeof(vithip.FrameNV12) == 48
    a, b = make_nv12(6, 8, seed=1), make_nv12(4, 10, seed=2)
    buf, desc = vithip.pack_frames_nv12([a, b], [None, (1.0, 0.5, 9.0, 3.5)])
    assert buf.dtype == np.uint8 and buf.size == 6 * 8 * 3 // 2 + 4 * 10 * 3 // 2 and len(desc) == 2
    assert (desc[0].y_offset, desc[0].uv_offset, desc[0].height, desc[0].width, desc[0].y_stride, desc[0].uv_stride) == (0, 48, 6, 8, 8, 8)
    assert (desc[1].y_offset, desc[1].uv_offset, desc[1].height, desc[1].width, desc[1].y_stride, desc[1].uv_stride) == (72, 112, 4, 10, 10, 10)
    assert list(desc[0].box) == [0.0, 0.0, 8.0, 6.0] and list(desc[1].box) == [1.0, 0.5, 9.0, 3.5]
    assert np.array_equal(buf[0:48].reshape(6, 8), a[0]) and np.array_equal(buf[48:72].reshape(3, 4, 2), a[1])
    assert np.array_equal(buf[72:112].reshape(4, 10), b[0]) and np.array_equal(buf[112:132].reshape(2, 5, 2), b[1])
    with pytest.raises(ValueError):
        vithip.pack_frames_nv12([(np.zeros((5, 8), np.uint8), np.zeros((2, 4, 2), np.uint8))])
    with pytest.raises(ValueError):
        vithip.pack_frames_nv12([(np.zeros((6, 8), np.uint8), np.zeros((3, 3, 2), np.uint8))])
    with pytest.raises(TypeError):
        vithip.pack_frames_nv12([(np.zeros((6, 8), np.float32), np.zeros((3, 4, 2), np.uint8))])


# ---- the kernel's arithmetic, emulated in float32, meets the bounds the GPU suite asserts ---------------------------------------
# (h, w, box, S): the operator cases of test_gpu_nv12
OP_CASES = {
    "down_38x54_16": (38, 54, None, 16),
    "up_20x24_32": (20, 24, None, 32),
    "fractional_box_98x132_28": (98, 132, (10.25, 5.5, 101.75, 95.125), 28),
    "taps29_270x480_32": (270, 480, None, 32),
}
COLOURS = {"bt709_limited_left": (N.BT709, False, N.CHROMA_LEFT), "bt601_full_centre": (N.BT601, True, N.CHROMA_CENTER)}


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_fp32_emulation_meets_the_gpu_bounds(name, colour):
    h, w, box, s = OP_CASES[name]
    std, full, site = COLOURS[colour]
    y, uv = make_nv12(h, w, seed=h + w)
    m = N.yuv_matrix(std, full)
    v64 = N.resize_nv12_f64(y, uv, box, s, m, site)
    got = N.resize_nv12_f32(y, uv, box, s, m, site)
    margin = N.margin(*N.max_taps(y, box, s, site))
    # the contract clamps before it rounds and a colour matrix leaves 0..255 (saturated colours): the byte is compared with the
    # clamped value, which moves no in-range value and is 1-Lipschitz, so the bound is the one of the unclamped arithmetic
    err = float(np.abs(got.astype(np.float64) - np.clip(v64, 0.0, 255.0)).max())
    same = float((got == np.rint(np.clip(v64, 0.0, 255.0)).astype(np.uint8)).mean())
    print(f"emulated nv12 {h}x{w} box {box} -> {s} {colour}: max |byte - v64| = {err:.6f} (bound {0.5 + margin:.6f}), {100 * same:.3f} % equal rint(v64)")
    assert err <= 0.5 + margin
    assert same >= 0.995
