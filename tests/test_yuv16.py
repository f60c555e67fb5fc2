"""CPU suite of the 16-bit YUV entry points (include/vithip.h, "16-bit YUV frames"): vh_yuv_matrix16 against its
float64 statement bit for bit, its two identities, every refusal decided on the host with its own message, the packing, and the
fp32 emulation of the kernel's fmaf order on uint16 planes against the bounds the GPU suite asserts."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nv12_ref as N
import vithip
import yuv16_ref as W
import yuv_ref as Y
from test_nv12 import make_rgb
from test_yuv_planar import OP_CASES, SUBS
from vh_testlib import last_error

VH_ERR_INVALID = 1
# name -> (standard, full_range, bits, msb_aligned, chroma_site)
COLOURS16 = {"bt709_limited_10_msb_left": (N.BT709, False, 10, True, N.CHROMA_LEFT),
             "bt2020_limited_10_lsb_left": (N.BT2020, False, 10, False, N.CHROMA_LEFT),
             "bt601_full_12_lsb_centre": (N.BT601, True, 12, False, N.CHROMA_CENTER),
             "bt709_full_16_msb_centre": (N.BT709, True, 16, True, N.CHROMA_CENTER)}


def make_yuv16(h, w, sub, seed, colour):
    """(Y, U, V) uint16 planes of a synthetic picture (test_nv12.make_rgb) in the format of COLOURS16[colour]."""
    std, full, bits, msb, _ = COLOURS16[colour]
    return W.rgb_to_yuv16_planes(make_rgb(h, w, seed), *sub, bits, msb, std, full)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msb", [False, True], ids=["lsb", "msb"])
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("std", [N.BT601, N.BT709, N.BT2020], ids=["bt601", "bt709", "bt2020"])
def test_yuv_matrix16_is_the_float64_statement_bit_for_bit(std, full, bits, msb):
    got = vithip.yuv_matrix16(std, full, bits, msb)
    want = W.yuv_matrix16(std, full, bits, msb)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_eight_bits_lsb_aligned_is_vh_yuv_matrix():
    for std, full in itertools.product((N.BT601, N.BT709, N.BT2020), (False, True)):
        assert np.array_equal(vithip.yuv_matrix16(std, full, 8, False).view(np.uint32), vithip.yuv_matrix(std, full).view(np.uint32))


def test_limited_p010_matrix_is_the_8_bit_one_with_its_first_three_columns_scaled_by_2_to_the_minus_8():
    for std in (N.BT601, N.BT709, N.BT2020):
        want = vithip.yuv_matrix(std, False).copy()
        want[:, :3] *= np.float32(2.0 ** -8)                                       # a power of two: exact
        assert np.array_equal(vithip.yuv_matrix16(std, False, 10, True).view(np.uint32), want.view(np.uint32))
    # the default of the 16-bit colour state is this matrix at BT.709
    assert np.array_equal(vithip.yuv_matrix16(), vithip.yuv_matrix16(vithip.YUV_BT709, False, 10, True))


def test_yuv_matrix16_refuses_bad_arguments():
    L = vithip.lib()
    m = np.zeros(12, np.float32)
    for args in ((3, 0, 10, 1), (-1, 0, 10, 1), (1, 2, 10, 1), (1, -1, 10, 1), (1, 0, 7, 1), (1, 0, 17, 1), (1, 0, 0, 0), (1, 0, 10, 2), (1, 0, 10, -1)):
        assert L.vh_yuv_matrix16(*args, m.ctypes.data) == VH_ERR_INVALID, args
        assert "yuv matrix16" in last_error()
    assert L.vh_yuv_matrix16(1, 0, 10, 1, None) == VH_ERR_INVALID
    assert not m.any()
    for bits in range(8, 17):
        assert L.vh_yuv_matrix16(2, 1, bits, 0, m.ctypes.data) == 0


# ---- refusals without a device --------------------------------------------------------------------------------------------------
def one_yuv16(h=41, w=61, sub=(2, 2), y_stride=None, u_stride=None, v_stride=None, y_off=0, u_off=None, v_off=None, box=None):
    """One planar 16-bit descriptor, planes back to back; strides and offsets in bytes."""
    d = (vithip.FrameYUV * 1)()
    ch, cw = Y.chroma_size(h, w, max(sub[0], 1), max(sub[1], 1))
    d[0].height, d[0].width, d[0].sub_x, d[0].sub_y = h, w, sub[0], sub[1]
    d[0].y_stride = 2 * w if y_stride is None else y_stride
    d[0].u_stride = 2 * cw if u_stride is None else u_stride
    d[0].v_stride = 2 * cw if v_stride is None else v_stride
    d[0].y_offset = y_off
    d[0].u_offset = y_off + h * d[0].y_stride if u_off is None else u_off
    d[0].v_offset = d[0].u_offset + ch * d[0].u_stride if v_off is None else v_off
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def one_p016(h=40, w=60, y_stride=None, uv_stride=None, y_off=0, uv_off=None, box=None):
    d = (vithip.FrameNV12 * 1)()
    d[0].height, d[0].width = h, w
    d[0].y_stride = 2 * w if y_stride is None else y_stride
    d[0].uv_stride = 2 * w if uv_stride is None else uv_stride
    d[0].y_offset = y_off
    d[0].uv_offset = y_off + h * d[0].y_stride if uv_off is None else uv_off
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def test_every_planar_16_bit_refusal_is_decided_on_the_host_with_its_own_message():
    """vh_op_resize_yuv16 checks and plans before its first device call: a bad argument is VH_ERR_INVALID whether or not a device
    exists, and the pointers (0x1000 here) are never read (so no call here is a valid one)."""
    L = vithip.lib()
    fake = C.c_void_p(0x1000)
    m = np.ascontiguousarray(vithip.yuv_matrix16().reshape(-1))
    full = 2 * (41 * 61 + 2 * 21 * 31)                                                 # 41 x 61 at 4:2:0: chroma 21 x 31, 2 bytes a sample

    def rc(d, nbytes=full, s=16, batch=1, m=m, site=vithip.CHROMA_LEFT, frames=fake):
        return L.vh_op_resize_yuv16(frames, nbytes, C.addressof(d), batch, s, m.ctypes.data, site, fake, None)

    ok = one_yuv16()
    bad = {                                                                            # rule -> (descriptor, a word of its message)
        "odd y_offset": (one_yuv16(y_off=1, u_off=2 * 41 * 61 + 2, v_off=2 * 41 * 61 + 2 * 21 * 31 + 2), "offset is odd"),
        "odd u_offset": (one_yuv16(u_off=2 * 41 * 61 + 1, v_off=2 * 41 * 61 + 2 * 21 * 31 + 2), "offset is odd"),
        "odd v_offset": (one_yuv16(v_off=2 * 41 * 61 + 2 * 21 * 31 + 1), "offset is odd"),
        "odd y_stride": (one_yuv16(y_stride=123, u_off=6000, v_off=8000), "stride is odd"),
        "odd u_stride": (one_yuv16(u_stride=63, v_off=8000), "stride is odd"),
        "odd v_stride": (one_yuv16(v_stride=65), "stride is odd"),
        "y_stride = width: the 8-bit stride": (one_yuv16(y_stride=62), "y_stride < 2 * width"),
        "y_stride = 2 width - 2": (one_yuv16(y_stride=120), "y_stride < 2 * width"),
        "u_stride = 2 cw - 2": (one_yuv16(u_stride=60), "u_stride or v_stride < 2 * cw"),
        "v_stride = cw rounded up to even: the 8-bit stride": (one_yuv16(v_stride=32), "u_stride or v_stride < 2 * cw"),
        "u_stride = 2 (width / 2 rounded down) at 4:2:2": (one_yuv16(sub=(2, 1), u_stride=60), "u_stride or v_stride < 2 * cw"),
        "zero width": (one_yuv16(w=0), "1..8192"),
        "width 8193": (one_yuv16(w=8193), "1..8192"),
        "zero height": (one_yuv16(h=0), "1..8192"),
        "height 8193": (one_yuv16(h=8193), "1..8192"),
        "sub_x 0": (one_yuv16(sub=(0, 2)), "sub_x and sub_y"),
        "sub_x 3": (one_yuv16(sub=(3, 2)), "sub_x and sub_y"),
        "sub_y 4": (one_yuv16(sub=(2, 4)), "sub_x and sub_y"),
        "empty box": (one_yuv16(box=(5.0, 0.0, 5.0, 41.0)), "box outside the frame, or empty"),
        "box beyond the frame": (one_yuv16(box=(0.0, 0.0, 61.5, 41.0)), "box outside the frame, or empty"),
        "negative box": (one_yuv16(box=(0.0, -0.5, 61.0, 41.0)), "box outside the frame, or empty"),
        "nan box": (one_yuv16(box=(float("nan"), 0.0, 61.0, 41.0)), "box outside the frame, or empty"),
    }
    for why, (d, word) in bad.items():
        assert rc(d, nbytes=1 << 30) == VH_ERR_INVALID, why
        assert word in last_error() and last_error().startswith("resize_yuv16:"), (why, last_error())
    # each plane's last byte beyond nbytes, with the plane named; the byte count of the 8-bit layout is half of what is needed
    assert rc(ok, nbytes=full - 1) == VH_ERR_INVALID and "a V plane ends beyond nbytes" in last_error()
    assert rc(ok, nbytes=full // 2) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    assert rc(one_yuv16(u_off=full - 1302, v_off=2 * 41 * 61), nbytes=full - 1) == VH_ERR_INVALID and "a U plane ends beyond nbytes" in last_error()
    assert rc(one_yuv16(y_off=2604, u_off=0, v_off=1302), nbytes=full - 1) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    assert rc(one_yuv16(y_off=1 << 40), nbytes=full) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    assert rc(one_yuv16(sub=(1, 1)), nbytes=6 * 41 * 61 - 1) == VH_ERR_INVALID and "a V plane ends beyond nbytes" in last_error()
    # an odd device base
    assert rc(ok, frames=C.c_void_p(0x1001)) == VH_ERR_INVALID and "frames pointer is odd" in last_error()
    # scale > 32 on an axis
    assert rc(one_yuv16(h=1041, w=17), nbytes=1 << 30, s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    assert rc(one_yuv16(h=17, w=1041), nbytes=1 << 30, s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    for i in (0, 5, 11):
        for v in (np.inf, -np.inf, np.nan):
            mm = m.copy()
            mm[i] = v
            assert rc(ok, m=mm) == VH_ERR_INVALID and "not finite" in last_error()
    assert rc(ok, site=2) == VH_ERR_INVALID and "chroma_site" in last_error() and rc(ok, site=-1) == VH_ERR_INVALID
    assert rc(ok, batch=0) == VH_ERR_INVALID and rc(ok, s=0) == VH_ERR_INVALID and rc(ok, s=4097) == VH_ERR_INVALID
    for args in ((None, full, C.addressof(ok), 1, 16, m.ctypes.data, 1, fake, None), (fake, full, None, 1, 16, m.ctypes.data, 1, fake, None),
                 (fake, full, C.addressof(ok), 1, 16, None, 1, fake, None), (fake, full, C.addressof(ok), 1, 16, m.ctypes.data, 1, None, None)):
        assert L.vh_op_resize_yuv16(*args) == VH_ERR_INVALID and "null" in last_error()


def test_every_p016_refusal_is_decided_on_the_host_with_its_own_message():
    L = vithip.lib()
    fake = C.c_void_p(0x1000)
    m = np.ascontiguousarray(vithip.yuv_matrix16().reshape(-1))
    full = 3 * 40 * 60                                                                 # 40 x 60: Y 2 bytes a sample, UV 20 rows of 30 pairs of 4

    def rc(d, nbytes=full, s=16, batch=1, m=m, site=vithip.CHROMA_LEFT, frames=fake):
        return L.vh_op_resize_p016(frames, nbytes, C.addressof(d), batch, s, m.ctypes.data, site, fake, None)

    ok = one_p016()
    bad = {
        "odd y_offset": (one_p016(y_off=1, uv_off=4802), "offset is odd"),
        "odd uv_offset": (one_p016(uv_off=4801), "offset is odd"),
        "odd y_stride": (one_p016(y_stride=121), "stride is odd"),
        "odd uv_stride": (one_p016(uv_stride=123), "stride is odd"),
        "y_stride = width: the NV12 stride": (one_p016(y_stride=60), "y_stride or uv_stride < 2 * width"),
        "uv_stride = 2 width - 2": (one_p016(uv_stride=118), "y_stride or uv_stride < 2 * width"),
        "odd width": (one_p016(w=61), "even and 2..8192"),
        "odd height": (one_p016(h=41), "even and 2..8192"),
        "zero width": (one_p016(w=0), "even and 2..8192"),
        "height 8194": (one_p016(h=8194), "even and 2..8192"),
        "empty box": (one_p016(box=(5.0, 0.0, 5.0, 40.0)), "box outside the frame, empty, or scale > 32"),
        "box beyond the frame": (one_p016(box=(0.0, 0.0, 60.5, 40.0)), "box outside the frame, empty, or scale > 32"),
        "scale > 32": (one_p016(h=1042, w=18), "box outside the frame, empty, or scale > 32"),
    }
    for why, (d, word) in bad.items():
        assert rc(d, nbytes=1 << 30, s=32 if why == "scale > 32" else 16) == VH_ERR_INVALID, why
        assert word in last_error() and last_error().startswith("resize_p016:"), (why, last_error())
    assert rc(ok, nbytes=full - 1) == VH_ERR_INVALID and "a UV plane ends beyond nbytes" in last_error()
    assert rc(ok, nbytes=full // 2) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()      # NV12's byte count
    assert rc(one_p016(y_off=2400, uv_off=0), nbytes=full - 1) == VH_ERR_INVALID and "a Y plane ends beyond nbytes" in last_error()
    assert rc(ok, frames=C.c_void_p(0x1001)) == VH_ERR_INVALID and "frames pointer is odd" in last_error()
    assert rc(ok, frames=C.c_void_p(0x1003)) == VH_ERR_INVALID and "frames pointer is odd" in last_error()
    mm = m.copy()
    mm[7] = np.nan
    assert rc(ok, m=mm) == VH_ERR_INVALID and "not finite" in last_error()
    assert rc(ok, site=2) == VH_ERR_INVALID and "chroma_site" in last_error()
    assert rc(ok, batch=0) == VH_ERR_INVALID and rc(ok, s=0) == VH_ERR_INVALID and rc(ok, s=4097) == VH_ERR_INVALID
    for args in ((None, full, C.addressof(ok), 1, 16, m.ctypes.data, 1, fake, None), (fake, full, None, 1, 16, m.ctypes.data, 1, fake, None),
                 (fake, full, C.addressof(ok), 1, 16, None, 1, fake, None), (fake, full, C.addressof(ok), 1, 16, m.ctypes.data, 1, None, None)):
        assert L.vh_op_resize_p016(*args) == VH_ERR_INVALID and "null" in last_error()


def test_16_bit_calls_without_a_context_are_refused():
    L = vithip.lib()
    dy, dn = one_yuv16(), one_p016()
    buf, out, m = np.zeros(8000, np.uint8), np.zeros(8, np.float32), np.zeros(12, np.float32)
    for name, d in (("yuv16", dy), ("p016", dn)):
        assert getattr(L, "vh_forward_frames_" + name)(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
        assert getattr(L, "vh_forward_device_frames_" + name)(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
        assert getattr(L, "vh_ring_submit_frames_" + name)(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1) == VH_ERR_INVALID
    assert L.vh_set_frame_colour16(None, m.ctypes.data, 0) == VH_ERR_INVALID
    assert L.vh_get_frame_colour16(None, m.ctypes.data, None) == VH_ERR_INVALID


# ---- the packing ----------------------------------------------------------------------------------------------------------------
def test_pack_frames_16_bit_lays_little_endian_words_with_byte_offsets():
    rng = np.random.default_rng(5)
    plane = lambda *shape: rng.integers(0, 65536, shape, dtype=np.uint16)
    triples = [(plane(37, 53), plane(19, 27), plane(19, 27)), (plane(6, 8), plane(6, 4), plane(6, 4)), (plane(5, 3), plane(5, 3), plane(5, 3))]
    boxes = [None, (1.0, 0.5, 7.0, 3.5), None]
    buf, desc = vithip.pack_frames_yuv16(triples, boxes)
    off = 0
    for d, (y, u, v), box, sub in zip(desc, triples, boxes, ((2, 2), (2, 1), (1, 1))):
        (h, w), (ch, cw) = y.shape, u.shape
        assert (d.sub_x, d.sub_y) == sub
        assert (d.y_offset, d.u_offset, d.v_offset) == (off, off + 2 * h * w, off + 2 * (h * w + ch * cw))
        assert (d.height, d.width, d.y_stride, d.u_stride, d.v_stride) == (h, w, 2 * w, 2 * cw, 2 * cw)
        assert list(d.box) == ([0.0, 0.0, float(w), float(h)] if box is None else list(box))
        for o, p in ((d.y_offset, y), (d.u_offset, u), (d.v_offset, v)):
            b = buf[o:o + 2 * p.size].astype(np.uint16)
            assert np.array_equal((b[0::2] | (b[1::2] << 8)).reshape(p.shape), p)      # low byte first
        off += 2 * (h * w + 2 * ch * cw)
    assert buf.dtype == np.uint8 and buf.size == off
    pairs = [(plane(6, 8), plane(3, 4, 2)), (plane(2, 2), plane(1, 1, 2))]
    buf, desc = vithip.pack_frames_p016(pairs)
    assert (desc[0].y_offset, desc[0].uv_offset, desc[0].y_stride, desc[0].uv_stride) == (0, 96, 16, 16)
    assert (desc[1].y_offset, desc[1].uv_offset, desc[1].y_stride, desc[1].uv_stride) == (144, 152, 4, 4)
    assert buf.size == 156 and np.array_equal(buf[96:144].view("<u2").reshape(3, 4, 2), pairs[0][1])
    z8, z16 = (lambda *s: np.zeros(s, np.uint8)), (lambda *s: np.zeros(s, np.uint16))
    with pytest.raises(TypeError):
        vithip.pack_frames_yuv16([(z8(6, 8), z8(3, 4), z8(3, 4))])                     # byte planes belong to pack_frames_yuv
    with pytest.raises(TypeError):
        vithip.pack_frames_p016([(z8(6, 8), z8(3, 4, 2))])
    with pytest.raises(TypeError):
        vithip.pack_frames_p016([(z16(6, 8), z16(3, 4))])                              # a chroma plane without pairs
    with pytest.raises(ValueError):
        vithip.pack_frames_p016([(z16(5, 8), z16(2, 4, 2))])                           # odd height
    with pytest.raises(ValueError):
        vithip.pack_frames_yuv16([(z16(37, 53), z16(18, 27), z16(18, 27))])            # floor instead of ceiling
    with pytest.raises(ValueError):
        vithip.pack_frames_yuv16([triples[0]], [None, None])


# ---- the emulation --------------------------------------------------------------------------------------------------------------
def test_the_test_planes_use_the_format_s_range():
    for colour, (std, full, bits, msb, _) in COLOURS16.items():
        y, u, v = make_yuv16(98, 132, (2, 2), seed=1, colour=colour)
        low = (1 << (16 - bits)) - 1 if msb else 0
        assert y.dtype == np.uint16 and not (y & low).any() and int(y.max()) <= W.largest_word(bits, msb)
        assert int(y.max()) > W.largest_word(bits, msb) // 2                           # real N-bit codes, not 8-bit ones
        if bits == 16:
            assert int(y.max()) > 0x7fff                                               # words a sign-extending load would break


@pytest.mark.parametrize("colour", list(COLOURS16))
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_fp32_emulation_meets_the_gpu_bounds(name, sub, colour):
    h, w, box, s = OP_CASES[name]
    std, full, bits, msb, site = COLOURS16[colour]
    planes = make_yuv16(h, w, SUBS[sub], seed=h + w, colour=colour)
    m = W.yuv_matrix16(std, full, bits, msb)
    got = Y.resize_yuv_f32(*planes, box, s, m, site, SUBS[sub])
    err, bound, same = W.statement_figures(got, planes, box, s, m, site, SUBS[sub], W.largest_word(bits, msb))
    print(f"emulated yuv{sub} 16-bit {h}x{w} box {box} -> {s} {colour}: max |byte - v64| = {err:.6f} (bound {bound:.6f}), {100 * same:.3f} % equal rint(v64)")
    assert err <= bound
    assert same >= 0.995
