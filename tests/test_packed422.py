"""CPU suite of the packed 4:2:2 entry points (include/vithip.h, "Packed 4:2:2 frames"): every refusal decided on the
host with its own message for both planners, the binding's layout, and packed422_ref's memory layouts (round trips, the v210 bit
layout pinned by one hand-written block)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packed422_ref as P
import vithip
from test_yuv_planar import OP_CASES
from vh_testlib import last_error

VH_ERR_INVALID = 1
# (h, w, box, S) of the packed taps, shared with the GPU suite and tools/yuv_host_check.py: the planar operator cases, the widths
# either side of one and of 26 / 27 macropixels (53 and 54 are also 8 5/6 and 9 v210 blocks), a box with an odd x0 (it starts on the
# second luma of a macropixel), and fractional boxes that under left siting reach the last chroma column at an odd and an even width
PACKED_CASES = dict(OP_CASES, **{f"w{w}_5x{w}_16": (5, w, None, 16) for w in (1, 2, 3, 53, 54)},
                    odd_x0_box_38x54_16=(38, 54, (3.0, 1.0, 51.0, 37.0), 16),
                    left_last_chroma_37x53_32=(37, 53, (10.5, 0.25, 53.0, 36.5), 32),
                    left_last_chroma_38x54_32=(38, 54, (10.5, 0.25, 54.0, 37.5), 32))
V210_WIDTHS = (1, 5, 6, 7, 11, 12, 13, 53, 54, 1918)


def row_of(w, layout, sample_bytes):
    """Bytes of one unpadded row."""
    return 16 * ((w + 5) // 6) if layout == P.V210 else 4 * sample_bytes * ((w + 1) // 2)


def one(h=41, w=61, layout=P.YUYV, sample_bytes=1, stride=None, off=0, box=None):
    d = (vithip.FrameYUY2 * 1)()
    d[0].offset, d[0].height, d[0].width, d[0].layout = off, h, w, layout
    d[0].row_stride = row_of(w, layout, sample_bytes) if stride is None else stride
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def tap_rc(fn, d, nbytes=1 << 30, s=16, batch=1, m=None, site=vithip.CHROMA_LEFT, frames=0x1000, out=0x1000):
    """One call of a tap with pointers that are never read (so no call here may be a valid one)."""
    m = np.ascontiguousarray(vithip.yuv_matrix().reshape(-1)) if m is None else m
    return fn(C.c_void_p(frames), nbytes, C.addressof(d), batch, s, m.ctypes.data, site, C.c_void_p(out), None)


# ---- refusals without a device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_bytes", [1, 2], ids=["yuy2", "y210"])
def test_every_refusal_is_decided_on_the_host_with_its_own_message(sample_bytes):
    """Both planners check and plan before the first device call: a bad argument is VH_ERR_INVALID whether or not a device exists."""
    L = vithip.lib()
    fn, tag = (L.vh_op_resize_yuy2, "resize_yuy2") if sample_bytes == 1 else (L.vh_op_resize_y210, "resize_y210")
    mk = lambda **kw: one(sample_bytes=sample_bytes, **kw)
    bad = {                                                                            # rule -> (descriptor, a word of its message)
        "zero width": (mk(w=0, stride=64), "1..8192"),
        "width 8193": (mk(w=8193), "1..8192"),
        "zero height": (mk(h=0), "1..8192"),
        "height 8193": (mk(h=8193), "1..8192"),
        "layout -1": (mk(layout=-1, stride=1024), "layout must be"),
        "layout 5": (mk(layout=5, stride=1024), "layout must be"),
        "empty box": (mk(box=(5.0, 0.0, 5.0, 41.0)), "box outside the frame, or empty"),
        "box beyond the frame": (mk(box=(0.0, 0.0, 61.5, 41.0)), "box outside the frame, or empty"),
        "negative box": (mk(box=(0.0, -0.5, 61.0, 41.0)), "box outside the frame, or empty"),
        "nan box": (mk(box=(float("nan"), 0.0, 61.0, 41.0)), "box outside the frame, or empty"),
    }
    # the stride one byte (one 16-bit word: an odd stride has a message of its own) short, at an odd and an even width, every layout
    for lay in (P.YUYV, P.UYVY, P.YVYU, P.VYUY):
        for w in (61, 62):
            bad[f"stride short, width {w}, layout {lay}"] = (mk(w=w, layout=lay, stride=row_of(w, lay, sample_bytes) - sample_bytes), "row_stride <")
    for why, (d, word) in bad.items():
        assert tap_rc(fn, d) == VH_ERR_INVALID, why
        assert word in last_error() and last_error().startswith(tag), (why, last_error())
    # the last macropixel (its unread second luma included) beyond nbytes; one byte more is enough for the plan (scale is checked later)
    for w in (61, 62):
        full = 41 * row_of(w, P.UYVY, sample_bytes)
        assert tap_rc(fn, mk(w=w, layout=P.UYVY), nbytes=full - 1) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error()
        lead = 4 * sample_bytes
        assert tap_rc(fn, mk(w=w, layout=P.UYVY, off=lead), nbytes=full + lead - 1) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error()
    assert tap_rc(fn, mk(off=1 << 40), nbytes=1 << 20) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error()
    # scale > 32 on an axis
    assert tap_rc(fn, mk(h=1041, w=17), s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    assert tap_rc(fn, mk(h=17, w=1041), s=32) == VH_ERR_INVALID and "scale > 32" in last_error()
    ok = mk()
    m709 = np.ascontiguousarray(vithip.yuv_matrix().reshape(-1))
    for i in (0, 5, 11):
        for v in (np.inf, -np.inf, np.nan):
            m = m709.copy()
            m[i] = v
            assert tap_rc(fn, ok, m=m) == VH_ERR_INVALID and "not finite" in last_error()
    assert tap_rc(fn, ok, site=2) == VH_ERR_INVALID and "chroma_site" in last_error()
    assert tap_rc(fn, ok, site=-1) == VH_ERR_INVALID
    assert tap_rc(fn, ok, batch=0) == VH_ERR_INVALID and tap_rc(fn, ok, s=0) == VH_ERR_INVALID and tap_rc(fn, ok, s=4097) == VH_ERR_INVALID
    fake, full = C.c_void_p(0x1000), 1 << 20
    for args in ((None, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, fake, None), (fake, full, None, 1, 16, m709.ctypes.data, 1, fake, None),
                 (fake, full, C.addressof(ok), 1, 16, None, 1, fake, None), (fake, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, None, None)):
        assert fn(*args) == VH_ERR_INVALID and "null" in last_error()


def test_v210_is_refused_by_the_8_bit_entry_points():
    L = vithip.lib()
    d = one(layout=P.V210, stride=1024)
    assert tap_rc(L.vh_op_resize_yuy2, d) == VH_ERR_INVALID
    assert "VH_422_V210" in last_error() and "16-bit" in last_error()
    # ... and is a layout of its own to the 16-bit ones: the same descriptor passes every check but the span
    assert tap_rc(L.vh_op_resize_y210, d, nbytes=16) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error()


def test_alignment_refusals_of_the_16_bit_entry_points():
    fn = vithip.lib().vh_op_resize_y210
    # Y210: odd offset, odd stride, odd device pointer
    assert tap_rc(fn, one(sample_bytes=2, off=1)) == VH_ERR_INVALID and "offset is odd" in last_error()
    assert tap_rc(fn, one(sample_bytes=2, stride=8 * 31 + 1)) == VH_ERR_INVALID and "row_stride is odd" in last_error()
    assert tap_rc(fn, one(sample_bytes=2), frames=0x1001) == VH_ERR_INVALID and "frames pointer is odd" in last_error()
    # ... while 2 mod 4 and 2 mod 8 are taken: the next refusal is the span
    for kw in (dict(off=2), dict(off=6), dict(stride=8 * 31 + 2)):
        assert tap_rc(fn, one(sample_bytes=2, **kw), nbytes=8) == VH_ERR_INVALID and "ends beyond nbytes" in last_error(), kw
    assert tap_rc(fn, one(sample_bytes=2), nbytes=8, frames=0x1002) == VH_ERR_INVALID and "ends beyond nbytes" in last_error()
    # v210: offset, stride and device pointer of 2 mod 4 (and odd ones)
    v = lambda **kw: one(layout=P.V210, **kw)
    for off in (1, 2, 3, 6):
        assert tap_rc(fn, v(off=off)) == VH_ERR_INVALID and "offset is no multiple of 4" in last_error(), off
    for extra in (1, 2, 3, 6):
        assert tap_rc(fn, v(stride=16 * 11 + extra)) == VH_ERR_INVALID and "row_stride is no multiple of 4" in last_error(), extra
    for frames in (0x1001, 0x1002, 0x1003):
        assert tap_rc(fn, v(), frames=frames) == VH_ERR_INVALID and "frames pointer is no multiple of 4" in last_error(), frames
    for kw in (dict(off=4), dict(off=12), dict(stride=16 * 11 + 4)):
        assert tap_rc(fn, v(**kw), nbytes=8) == VH_ERR_INVALID and "ends beyond nbytes" in last_error(), kw
    # the 8-bit entry points take any of them
    fn8 = vithip.lib().vh_op_resize_yuy2
    for kw in (dict(off=1), dict(off=3), dict(stride=4 * 31 + 1)):
        assert tap_rc(fn8, one(**kw), nbytes=8, frames=0x1001) == VH_ERR_INVALID and "ends beyond nbytes" in last_error(), kw


@pytest.mark.parametrize("w", [6, 7, 12])
def test_v210_stride_one_block_short(w):
    fn = vithip.lib().vh_op_resize_y210
    blocks = (w + 5) // 6
    assert blocks == {6: 1, 7: 2, 12: 2}[w]
    d = one(h=9, w=w, layout=P.V210, stride=16 * (blocks - 1))
    assert tap_rc(fn, d, s=4) == VH_ERR_INVALID and "row_stride < 16 * ceil(width / 6)" in last_error()
    # four bytes short is refused by the same rule; the full row passes it
    assert tap_rc(fn, one(h=9, w=w, layout=P.V210, stride=16 * blocks - 4), s=4) == VH_ERR_INVALID and "row_stride < 16" in last_error()
    assert tap_rc(fn, one(h=9, w=w, layout=P.V210), s=4, nbytes=9 * 16 * blocks - 1) == VH_ERR_INVALID and "ends beyond nbytes" in last_error()


def test_packed_calls_without_a_context_are_refused():
    L = vithip.lib()
    d = one()
    buf, out = np.zeros(41 * 124, np.uint8), np.zeros(8, np.float32)
    for fn in (L.vh_forward_frames_yuy2, L.vh_forward_device_frames_yuy2, L.vh_forward_frames_y210, L.vh_forward_device_frames_y210):
        assert fn(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    for fn in (L.vh_ring_submit_frames_yuy2, L.vh_ring_submit_frames_y210):
        assert fn(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1) == VH_ERR_INVALID


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_frame_yuy2_layout_is_the_header_s():
    """include/vithip.h: sizeof 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24."""
    F = vithip.FrameYUY2
    assert C.sizeof(F) == 40
    assert {n: getattr(F, n).offset for n, _ in F._fields_} == dict(offset=0, height=8, width=12, row_stride=16, layout=20, box=24)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vithip.h")).read()
    assert "sizeof(vh_frame_yuy2) == 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24" in hdr
    body = re.search(r"typedef struct vh_frame_yuy2 \{(.*?)\} vh_frame_yuy2;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [n for n, _ in F._fields_]
    for name, value in (("YUYV", 0), ("UYVY", 1), ("YVYU", 2), ("VYUY", 3), ("V210", 4)):
        assert re.search(rf"#define VH_422_{name} {value}\b", hdr) and getattr(vithip, "L422_" + name) == value and getattr(P, name) == value


def planes_of(rng, h, w, dtype, top):
    cw = (w + 1) // 2
    return tuple(rng.integers(0, top + 1, shape, dtype=dtype) for shape in ((h, w), (h, cw), (h, cw)))


# ---- the layouts ----------------------------------------------------------------------------------------------------------------
def test_macropixel_orders_by_hand():
    y = np.array([[10, 11, 12]], np.uint8)
    u, v = np.array([[20, 21]], np.uint8), np.array([[30, 31]], np.uint8)
    assert P.interleave(y, u, v, P.YUYV).tolist() == [[10, 20, 11, 30, 12, 21, 0, 31]]
    assert P.interleave(y, u, v, P.UYVY).tolist() == [[20, 10, 30, 11, 21, 12, 31, 0]]
    assert P.interleave(y, u, v, P.YVYU).tolist() == [[10, 30, 11, 20, 12, 31, 0, 21]]
    assert P.interleave(y, u, v, P.VYUY).tolist() == [[30, 10, 20, 11, 31, 12, 21, 0]]


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)], ids=["u8", "u16"])
def test_interleave_round_trips_and_pack_frames_yuy2_agrees(dtype, top):
    rng = np.random.default_rng(7)
    frames, layouts = [], []
    for i, (h, w) in enumerate(((5, 1), (5, 2), (3, 3), (4, 53), (2, 54))):
        for lay in (P.YUYV, P.UYVY, P.YVYU, P.VYUY):
            yuv = planes_of(rng, h, w, dtype, top)
            back = P.deinterleave(P.interleave(*yuv, lay), w, lay)
            assert all(np.array_equal(a, b) for a, b in zip(back, yuv)), (h, w, lay)
            frames.append(yuv); layouts.append(lay)
    buf, desc = vithip.pack_frames_yuy2(frames, layouts)
    sb, off = np.dtype(dtype).itemsize, 0
    for d, yuv, lay in zip(desc, frames, layouts):
        h, w = yuv[0].shape
        assert (d.offset, d.height, d.width, d.row_stride, d.layout) == (off, h, w, 4 * sb * ((w + 1) // 2), lay)
        assert list(d.box) == [0.0, 0.0, float(w), float(h)]
        rows = buf[off:off + h * d.row_stride].view(np.dtype(dtype).newbyteorder("<")).reshape(h, -1)
        assert np.array_equal(rows, P.interleave(*yuv, lay))
        off += h * d.row_stride
    assert buf.dtype == np.uint8 and buf.size == off
    ref, rdesc = P.lay_out(frames, [None] * len(frames), layouts)
    assert bytes(rdesc) == bytes(desc)
    with pytest.raises(ValueError):
        vithip.pack_frames_yuy2([(frames[12][0], frames[0][1], frames[0][2])])         # a 4 x 53 luma plane with 5 x 1 chroma planes
    with pytest.raises(ValueError):
        vithip.pack_frames_yuy2(frames[:1], [7])
    with pytest.raises(ValueError):
        vithip.pack_frames_yuy2(frames[:1], [P.YUYV], [None, None])
    if dtype == np.uint8:
        with pytest.raises(ValueError):
            vithip.pack_frames_yuy2(frames[:1], P.V210)                                  # v210 takes uint16 codes


def test_v210_bit_layout_is_pinned_by_one_hand_written_block():
    """Twelve distinct codes, U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5, three to a little-endian word from bit 0."""
    y = np.array([[0x101, 0x102, 0x103, 0x104, 0x105, 0x106]], np.uint16)
    u = np.array([[0x201, 0x202, 0x203]], np.uint16)
    v = np.array([[0x301, 0x302, 0x3FF]], np.uint16)
    want = [0x201 | 0x101 << 10 | 0x301 << 20, 0x102 | 0x202 << 10 | 0x103 << 20, 0x302 | 0x104 << 10 | 0x203 << 20, 0x105 | 0x3FF << 10 | 0x106 << 20]
    raw = bytes([0x01, 0x06, 0x14, 0x30, 0x02, 0x09, 0x38, 0x10, 0x02, 0x13, 0x34, 0x20, 0x05, 0xFD, 0x6F, 0x10])
    assert np.frombuffer(raw, "<u4").tolist() == want
    assert P.to_v210(y, u, v).tolist() == [want]
    assert P.row_bytes(y, u, v, P.V210).tobytes() == raw
    assert vithip.v210_rows(y, u, v).tolist() == [want]
    assert P.to_v210(y, u, v, high_bits=3).tolist() == [[x | 0xC0000000 for x in want]]
    back = P.from_v210(np.array([[x | 0x80000000 for x in want]], np.uint32), 6)
    assert all(np.array_equal(a, b) for a, b in zip(back, (y, u, v)))


def test_v210_round_trips_at_every_width_mod_6():
    rng = np.random.default_rng(11)
    frames = []
    for w in (1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 53, 54):
        yuv = planes_of(rng, 3, w, np.uint16, 1023)
        yuv[0][0, 0], yuv[1][0, -1], yuv[2][-1, 0] = 1023, 0, 1023
        words = P.to_v210(*yuv, high_bits=w % 4)
        assert words.shape == (3, 4 * ((w + 5) // 6)) and words.dtype == np.uint32
        assert all(np.array_equal(a, b) for a, b in zip(P.from_v210(words, w), yuv)), w
        assert np.array_equal(vithip.v210_rows(*yuv), P.to_v210(*yuv))
        frames.append(yuv)
    buf, desc = vithip.pack_frames_yuy2(frames, P.V210)
    ref, rdesc = P.lay_out(frames, [None] * len(frames), P.V210)
    assert np.array_equal(buf, ref) and bytes(desc) == bytes(rdesc)
    assert all(d.offset % 4 == 0 and d.row_stride == 16 * ((d.width + 5) // 6) and d.layout == P.V210 for d in desc)
    with pytest.raises(ValueError):
        vithip.v210_rows(np.full((1, 2), 1024, np.uint16), np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint16))


def test_lay_out_places_lead_padding_and_gaps():
    rng = np.random.default_rng(3)
    frames = [planes_of(rng, 4, 5, np.uint8, 255), planes_of(rng, 3, 6, np.uint8, 255)]
    buf, desc = P.lay_out(frames, [None, (1.0, 0.0, 5.0, 3.0)], [P.UYVY, P.YVYU], pad=3, lead=5, gap=2)
    assert (desc[0].offset, desc[0].row_stride, desc[1].offset, desc[1].row_stride) == (5, 15, 5 + 3 * 15 + 12 + 2, 15)
    assert buf.size == desc[1].offset + 2 * 15 + 12 + 2 and list(desc[1].box) == [1.0, 0.0, 5.0, 3.0]
    for d, yuv in zip(desc, frames):
        rows = np.stack([buf[d.offset + r * d.row_stride:d.offset + r * d.row_stride + 12] for r in range(d.height)])
        assert all(np.array_equal(a, b) for a, b in zip(P.deinterleave(rows, d.width, d.layout), yuv))
    assert (buf[:5] == P.FILL).all() and (buf[-2:] == P.FILL).all()
