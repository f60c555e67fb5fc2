"""CPU suite of the packed 4:4:4 entry points (include/vithip.h, "Packed 4:4:4 frames"): every refusal decided on the
host with its own message for both planners, the binding's layout and every VH_444_* value against the header, and packed444_ref's
memory layouts (round trips, the Y410 and V410 bit layouts each pinned by one hand-written word)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packed444_ref as P
import vithip
from test_yuv_planar import OP_CASES
from vh_testlib import last_error

VH_ERR_INVALID = 1
# (h, w, box, S) of the packed taps, shared with the GPU suite and tools/yuv_host_check.py: the planar operator cases, the widths
# either side of one pixel and of 53 / 54, a box with an odd x0, a fractional box, and scales above and below 1 at outputs 16 and 32
PACKED_CASES = dict(OP_CASES, **{f"w{w}_5x{w}_16": (5, w, None, 16) for w in (1, 2, 3, 53, 54)},
                    odd_x0_box_38x54_16=(38, 54, (3.0, 1.0, 51.0, 37.0), 16),
                    fractional_box_37x53_32=(37, 53, (10.5, 0.25, 52.75, 36.5), 32),
                    upscale_9x11_32=(9, 11, (1.0, 0.5, 10.0, 8.5), 32))
HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vithip.h")).read()


def row_of(w, layout, sample_bytes):
    """Bytes of one unpadded row."""
    return w * P.pixel_bytes(layout, sample_bytes)


def one(h=41, w=61, layout=None, sample_bytes=1, stride=None, off=0, box=None):
    layout = (P.BGRA if sample_bytes == 1 else P.Y416) if layout is None else layout
    d = (vithip.FrameBGRA * 1)()
    d[0].offset, d[0].height, d[0].width, d[0].layout = off, h, w, layout
    d[0].row_stride = row_of(w, layout, sample_bytes) if stride is None else stride
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def tap_rc(fn, d, nbytes=1 << 30, s=16, batch=1, m=None, site=vithip.CHROMA_LEFT, frames=0x1000, out=0x1000):
    """One call of a tap with pointers that are never read (so no call here may be a valid one)."""
    m = np.ascontiguousarray(vithip.yuv_matrix().reshape(-1)) if m is None else m
    return fn(C.c_void_p(frames), nbytes, C.addressof(d), batch, s, m.ctypes.data, site, C.c_void_p(out), None)


EMPTY = (5.0, 0.0, 5.0, 41.0)   # a descriptor with this box passes every check in front of the box: "accepted so far"


def reaches_the_box(fn, d, **kw):
    return tap_rc(fn, d, **kw) == VH_ERR_INVALID and "box outside the frame, or empty" in last_error()


# ---- refusals without a device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_bytes", [1, 2], ids=["bgra", "y410"])
def test_every_refusal_is_decided_on_the_host_with_its_own_message(sample_bytes):
    """Both planners check and plan before the first device call: a bad argument is VH_ERR_INVALID whether or not a device exists."""
    L = vithip.lib()
    fn, tag = (L.vh_op_resize_bgra, "resize_bgra") if sample_bytes == 1 else (L.vh_op_resize_y410, "resize_y410")
    mk = lambda **kw: one(sample_bytes=sample_bytes, **kw)
    bad = {                                                                            # rule -> (descriptor, a word of its message)
        "zero width": (mk(w=0, stride=64), "1..8192"),
        "width 8193": (mk(w=8193), "1..8192"),
        "zero height": (mk(h=0), "1..8192"),
        "height 8193": (mk(h=8193), "1..8192"),
        "layout -1": (mk(layout=-1, stride=1024), "bits outside"),
        "layout bit 10": (mk(layout=P.VUYA | 1024, stride=1024), "bits outside"),
        "layout bit 9 without bit 8": (mk(layout=P.VUYA | 512, stride=1024), "bits outside"),
        "position 3 of three": (mk(layout=vithip.layout_444(0, 1, 3, False, True), stride=1024), "position 3 in a pixel of three samples"),
        "position 3 of three, first": (mk(layout=vithip.layout_444(3, 1, 0, False, True), stride=1024), "position 3 in a pixel of three samples"),
        "empty box": (mk(box=EMPTY), "box outside the frame, or empty"),
        "box beyond the frame": (mk(box=(0.0, 0.0, 61.5, 41.0)), "box outside the frame, or empty"),
        "negative box": (mk(box=(0.0, -0.5, 61.0, 41.0)), "box outside the frame, or empty"),
        "nan box": (mk(box=(float("nan"), 0.0, 61.0, 41.0)), "box outside the frame, or empty"),
    }
    if sample_bytes == 1:
        bad["Y410 on the 8-bit entry points"] = (mk(layout=P.Y410, stride=1024), "10-bit layouts; they go to the 16-bit (_y410) entry points")
        bad["V410 on the 8-bit entry points"] = (mk(layout=P.V410, stride=1024), "10-bit layouts; they go to the 16-bit (_y410) entry points")
    else:
        bad["RGB words"] = (mk(layout=P.BGRA, stride=1024), "RGB words of 10 / 16 bits are not taken")
        bad["three words"] = (mk(layout=P.YUV24, stride=1024), "a pixel of 16-bit words has four samples")
        bad["a 10-bit layout of other positions"] = (mk(layout=P.VUYA | 256, stride=1024), "a 10-bit layout must be VH_444_Y410 or VH_444_V410")
        bad["a 10-bit layout without yuv"] = (mk(layout=P.BGRA | 256, stride=1024), "a 10-bit layout must be VH_444_Y410 or VH_444_V410")
    for why, (d, word) in bad.items():
        assert tap_rc(fn, d) == VH_ERR_INVALID, why
        assert word in last_error() and last_error().startswith(tag + ":"), (why, last_error())
    assert len({word for _, word in bad.values()}) >= 5
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
    assert tap_rc(fn, ok, batch=0) == VH_ERR_INVALID and tap_rc(fn, ok, s=0) == VH_ERR_INVALID and tap_rc(fn, ok, s=4097) == VH_ERR_INVALID
    fake, full = C.c_void_p(0x1000), 1 << 20
    for args in ((None, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, fake, None), (fake, full, None, 1, 16, m709.ctypes.data, 1, fake, None),
                 (fake, full, C.addressof(ok), 1, 16, None, 1, fake, None), (fake, full, C.addressof(ok), 1, 16, m709.ctypes.data, 1, None, None)):
        assert fn(*args) == VH_ERR_INVALID and "null" in last_error() and last_error().startswith(tag + ":")


def test_the_messages_of_the_two_planners_are_all_different():
    """Every refusal has a message of ITS OWN: collect one per rule and per planner; no two are the same text."""
    L = vithip.lib()
    seen = []
    for fn, sb in ((L.vh_op_resize_bgra, 1), (L.vh_op_resize_y410, 2)):
        mk = lambda **kw: one(sample_bytes=sb, **kw)
        calls = [(mk(w=0, stride=64), {}), (mk(layout=-1, stride=1024), {}), (mk(layout=vithip.layout_444(0, 1, 3, False, True), stride=1024), {}),
                 (mk(stride=8), {}), (mk(), dict(nbytes=8)), (mk(box=EMPTY), {}), (mk(h=1041, w=17), dict(s=32)), (mk(), dict(batch=0))]
        if sb == 1:
            calls += [(mk(layout=P.Y410, stride=1024), {}), (mk(layout=P.BGR, stride=8), {})]
        else:
            calls += [(mk(layout=P.BGRA), {}), (mk(layout=P.YUV24, stride=1024), {}), (mk(layout=P.VUYA | 256, stride=1024), {}),
                      (mk(layout=P.Y410, stride=8), {}), (mk(off=1), {}), (mk(stride=8 * 61 + 1), {}), (mk(), dict(frames=0x1001)),
                      (mk(layout=P.Y410, off=2), {}), (mk(layout=P.Y410, stride=4 * 61 + 2), {}), (mk(layout=P.Y410), dict(frames=0x1002))]
        for d, kw in calls:
            assert tap_rc(fn, d, **kw) == VH_ERR_INVALID
            seen.append(last_error())
    assert len(set(seen)) == len(seen), sorted(seen)


@pytest.mark.parametrize("w", [1, 2, 3, 54])
def test_strides_one_byte_short(w):
    """One byte (one 16-bit word, one 32-bit word: an unaligned stride has a message of its own) short of the row is refused; the row
    itself passes."""
    L = vithip.lib()
    for fn, sb, layouts in ((L.vh_op_resize_bgra, 1, (P.RGB, P.BGR, P.YUV24, P.RGBA, P.BGRA, P.ARGB, P.ABGR, P.VUYA, P.AYUV)),
                            (L.vh_op_resize_y410, 2, (P.Y416, P.AYUV64, P.Y410, P.V410))):
        for lay in layouts:
            row = row_of(w, lay, sb)
            assert row == w * {1: 4 if lay & 64 else 3, 2: 4 if lay & 256 else 8}[sb]
            unit = 4 if lay & 256 else sb
            assert tap_rc(fn, one(h=9, w=w, layout=lay, sample_bytes=sb, stride=row - unit), s=4) == VH_ERR_INVALID, (w, lay)
            assert "row_stride <" in last_error() and f"{row // w} * width" in last_error(), (w, lay, last_error())
            assert reaches_the_box(fn, one(h=9, w=w, layout=lay, sample_bytes=sb, box=(0.0, 0.0, 0.0, 9.0)), s=4), (w, lay, last_error())


def test_a_span_that_ends_at_nbytes_is_accepted_and_one_byte_short_is_refused():
    L = vithip.lib()
    for fn, sb, layouts in ((L.vh_op_resize_bgra, 1, (P.BGR, P.BGRA)), (L.vh_op_resize_y410, 2, (P.Y416, P.V410))):
        for lay in layouts:
            for w in (1, 61):
                row = row_of(w, lay, sb)
                for off, pad in ((0, 0), (8, 0), (8, 8)):
                    span = 40 * (row + pad) + row
                    d = one(w=w, layout=lay, sample_bytes=sb, off=off, stride=row + pad, box=EMPTY if w == 61 else (0.0, 0.0, 0.0, 41.0))
                    assert reaches_the_box(fn, d, nbytes=off + span), (lay, w, off, pad, last_error())
                    assert tap_rc(fn, d, nbytes=off + span - 1) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error(), (lay, w, off, pad)
        assert tap_rc(fn, one(sample_bytes=sb, off=1 << 40), nbytes=1 << 20) == VH_ERR_INVALID and "a frame ends beyond nbytes" in last_error()


def test_offsets_strides_and_bases_of_every_residue():
    """1, 2, 3, 4 and 6 mod 8 as offset, as row padding and as device base: taken or refused as the header says, each separately."""
    L = vithip.lib()
    fn8, fn16 = L.vh_op_resize_bgra, L.vh_op_resize_y410
    for k in (1, 2, 3, 4, 6):
        # 8-bit layouts take everything
        for lay in (P.BGR, P.BGRA, P.VUYA):
            row = row_of(61, lay, 1)
            assert reaches_the_box(fn8, one(layout=lay, off=k, box=EMPTY)), (k, lay)
            assert reaches_the_box(fn8, one(layout=lay, stride=row + k, box=EMPTY)), (k, lay)
            assert reaches_the_box(fn8, one(layout=lay, box=EMPTY), frames=0x1000 + k), (k, lay)
        # 16-bit words: even
        for lay in (P.Y416, P.AYUV64):
            calls = ((dict(off=k), {}, "offset is odd"), (dict(stride=8 * 61 + k), {}, "row_stride is odd"),
                     ({}, dict(frames=0x1000 + k), "frames pointer is odd"))
            for dkw, ckw, word in calls:
                d = one(layout=lay, sample_bytes=2, box=EMPTY, **dkw)
                if k % 2:
                    assert tap_rc(fn16, d, **ckw) == VH_ERR_INVALID and word in last_error(), (k, lay, word, last_error())
                else:
                    assert reaches_the_box(fn16, d, **ckw), (k, lay, word, last_error())
        # one 32-bit word per pixel: multiples of 4
        for lay in (P.Y410, P.V410):
            calls = ((dict(off=k), {}, "offset is no multiple of 4"), (dict(stride=4 * 61 + k), {}, "row_stride is no multiple of 4"),
                     ({}, dict(frames=0x1000 + k), "frames pointer is no multiple of 4"))
            for dkw, ckw, word in calls:
                d = one(layout=lay, sample_bytes=2, box=EMPTY, **dkw)
                if k % 4:
                    assert tap_rc(fn16, d, **ckw) == VH_ERR_INVALID and word in last_error(), (k, lay, word, last_error())
                else:
                    assert reaches_the_box(fn16, d, **ckw), (k, lay, word, last_error())


def test_packed_calls_without_a_context_are_refused():
    L = vithip.lib()
    d = one()
    buf, out = np.zeros(41 * 61 * 8, np.uint8), np.zeros(8, np.float32)
    for fn in (L.vh_forward_frames_bgra, L.vh_forward_device_frames_bgra, L.vh_forward_frames_y410, L.vh_forward_device_frames_y410):
        assert fn(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1, out.ctypes.data) == VH_ERR_INVALID
    for fn in (L.vh_ring_submit_frames_bgra, L.vh_ring_submit_frames_y410):
        assert fn(None, buf.ctypes.data, buf.nbytes, C.addressof(d), 1) == VH_ERR_INVALID


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_frame_bgra_layout_is_the_header_s():
    """include/vithip.h: sizeof 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24."""
    F = vithip.FrameBGRA
    assert C.sizeof(F) == 40
    assert {n: getattr(F, n).offset for n, _ in F._fields_} == dict(offset=0, height=8, width=12, row_stride=16, layout=20, box=24)
    assert "sizeof(vh_frame_bgra) == 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24" in HDR
    body = re.search(r"typedef struct vh_frame_bgra \{(.*?)\} vh_frame_bgra;", HDR, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [n for n, _ in F._fields_]


# name -> (memory order of the samples, "x" unread; samples; yuv; value written out by hand)
NAMED = dict(RGB=("rgb", 36), BGR=("bgr", 6), RGBA=("rgbx", 100), BGRA=("bgrx", 70), ARGB=("xrgb", 121), ABGR=("xbgr", 91),
             YUV24=("yuv", 164), VUYA=("vuyx", 198), AYUV=("xyuv", 249), Y416=("uyvx", 225), AYUV64=("xyuv", 249))


def test_every_vh_444_value_is_the_header_s_macro_of_the_memory_order_in_its_name():
    macro = re.search(r"#define VH_444\(p0, p1, p2, four, yuv\) (.*)", HDR).group(1)
    assert macro.replace(" ", "") == "((p0)|(p1)<<2|(p2)<<4|((four)?64:0)|((yuv)?128:0))"
    values = {}
    for name, expr in re.findall(r"#define VH_444_(\w+) (.*?)\s*/\*", HDR):
        values[name] = eval(expr.replace("VH_444(", "f("), {"f": vithip.layout_444})
    assert sorted(values) == sorted(list(NAMED) + ["Y410", "V410"])
    for name, (order, by_hand) in NAMED.items():
        comps = "yuv" if "y" in order else "rgb"
        want = vithip.layout_444(*(order.index(c) for c in comps), len(order) == 4, comps == "yuv")
        assert values[name] == want == by_hand == getattr(vithip, "L444_" + name) == getattr(P, name), name
        assert P.samples(want) == len(order) and P.is_yuv(want) == (comps == "yuv")
    assert values["Y410"] == vithip.L444_Y410 == P.Y410 == 225 + 256 and values["V410"] == vithip.L444_V410 == P.V410 == 225 + 768


# ---- the layouts ----------------------------------------------------------------------------------------------------------------
def test_pixel_orders_by_hand():
    r, g, b = (np.array([[10 + k, 20 + k]], np.uint8) for k in (0, 1, 2))
    assert P.interleave(r, g, b, P.RGB).tolist() == [[10, 11, 12, 20, 21, 22]]
    assert P.interleave(r, g, b, P.BGR).tolist() == [[12, 11, 10, 22, 21, 20]]
    assert P.interleave(r, g, b, P.RGBA, 99).tolist() == [[10, 11, 12, 99, 20, 21, 22, 99]]
    assert P.interleave(r, g, b, P.BGRA, 99).tolist() == [[12, 11, 10, 99, 22, 21, 20, 99]]
    assert P.interleave(r, g, b, P.ARGB, 99).tolist() == [[99, 10, 11, 12, 99, 20, 21, 22]]
    assert P.interleave(r, g, b, P.ABGR, 99).tolist() == [[99, 12, 11, 10, 99, 22, 21, 20]]
    y, u, v = r, g, b
    assert P.interleave(y, u, v, P.YUV24).tolist() == [[10, 11, 12, 20, 21, 22]]
    assert P.interleave(y, u, v, P.VUYA, 99).tolist() == [[12, 11, 10, 99, 22, 21, 20, 99]]
    assert P.interleave(y, u, v, P.AYUV, 99).tolist() == [[99, 10, 11, 12, 99, 20, 21, 22]]
    assert P.interleave(y, u, v, P.Y416, 99).tolist() == [[11, 10, 12, 99, 21, 20, 22, 99]]


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)], ids=["u8", "u16"])
def test_interleave_round_trips_and_pack_frames_bgra_agrees(dtype, top):
    rng = np.random.default_rng(7)
    frames, layouts = [], []
    every = list(P.RGB_LAYOUTS.values()) + list(P.YUV_LAYOUTS.values()) if dtype == np.uint8 else list(P.WORD_LAYOUTS.values())
    for h, w in ((5, 1), (5, 2), (3, 3), (4, 53), (2, 54)):
        for lay in every:
            comps = tuple(rng.integers(0, top + 1, (h, w), dtype=dtype) for _ in range(3))
            back = P.deinterleave(P.interleave(*comps, lay), w, lay)
            assert all(np.array_equal(a, b) for a, b in zip(back, comps)), (h, w, lay)
            frames.append(comps); layouts.append(lay)
    buf, desc = vithip.pack_frames_bgra(frames, layouts)
    sb, off = np.dtype(dtype).itemsize, 0
    for d, comps, lay in zip(desc, frames, layouts):
        h, w = comps[0].shape
        assert (d.offset, d.height, d.width, d.row_stride, d.layout) == (off, h, w, P.samples(lay) * sb * w, lay)
        assert list(d.box) == [0.0, 0.0, float(w), float(h)]
        rows = buf[off:off + h * d.row_stride].view(np.dtype(dtype).newbyteorder("<")).reshape(h, -1)
        assert all(np.array_equal(a, b) for a, b in zip(P.deinterleave(rows, w, lay), comps))
        off += h * d.row_stride
    assert buf.dtype == np.uint8 and buf.size == off
    # [H, W, 3] pixels in output order are the same frames
    buf2, desc2 = vithip.pack_frames_bgra([np.stack(c, axis=-1) for c in frames], layouts)
    assert np.array_equal(buf, buf2) and bytes(desc) == bytes(desc2)
    with pytest.raises(ValueError):
        vithip.pack_frames_bgra(frames[:1], [vithip.layout_444(0, 1, 3, False, False)])
    with pytest.raises(ValueError):
        vithip.pack_frames_bgra(frames[:1], [every[0]], [None, None])
    if dtype == np.uint8:
        with pytest.raises(ValueError):
            vithip.pack_frames_bgra(frames[:1], P.Y410)                                  # 10-bit layouts take uint16 codes


def test_y410_and_v410_bit_layouts_are_each_pinned_by_one_hand_written_word():
    """Y410: U bits 0-9, Y 10-19, V 20-29.  V410: the same two bits higher.  Codes Y = 0x2A5, U = 0x13C, V = 0x3F1."""
    y, u, v = (np.array([[c]], np.uint16) for c in (0x2A5, 0x13C, 0x3F1))
    y410 = 0x13C | 0x2A5 << 10 | 0x3F1 << 20
    assert y410 == 0x3F1A953C and P.to_y410(y, u, v).tolist() == [[y410]]
    assert P.row_bytes((y, u, v), P.Y410).tobytes() == bytes([0x3C, 0x95, 0x1A, 0x3F])
    assert P.to_y410(y, u, v, ignored=3).tolist() == [[y410 | 0xC0000000]]
    v410 = 0x13C << 2 | 0x2A5 << 12 | 0x3F1 << 22
    assert v410 == 0xFC6A54F0 and P.to_v410(y, u, v).tolist() == [[v410]]
    assert P.row_bytes((y, u, v), P.V410).tobytes() == bytes([0xF0, 0x54, 0x6A, 0xFC])
    assert P.to_v410(y, u, v, ignored=3).tolist() == [[v410 | 3]]
    assert vithip.word10_rows(y, u, v, P.Y410).tolist() == [[y410]] and vithip.word10_rows(y, u, v, P.V410).tolist() == [[v410]]
    for lay, word in ((P.Y410, y410 | 0x80000000), (P.V410, v410 | 1)):
        assert [int(a[0, 0]) for a in P.from_word10(np.array([[word]], np.uint32), lay)] == [0x2A5, 0x13C, 0x3F1]
    buf, desc = vithip.pack_frames_bgra([(y, u, v), (y, u, v)], [P.Y410, P.V410])
    assert buf.tobytes() == bytes([0x3C, 0x95, 0x1A, 0x3F, 0xF0, 0x54, 0x6A, 0xFC]) and [d.row_stride for d in desc] == [4, 4]
    with pytest.raises(ValueError):
        vithip.word10_rows(np.full((1, 1), 1024, np.uint16), u, v, P.Y410)


def test_word10_round_trips():
    rng = np.random.default_rng(11)
    for w in (1, 2, 3, 53, 54):
        yuv = tuple(rng.integers(0, 1024, (3, w), dtype=np.uint16) for _ in range(3))
        yuv[0][0, 0], yuv[1][0, -1], yuv[2][-1, 0] = 1023, 0, 1023
        for lay, to in ((P.Y410, P.to_y410), (P.V410, P.to_v410)):
            words = to(*yuv, ignored=w % 4)
            assert words.shape == (3, w) and words.dtype == np.uint32
            assert all(np.array_equal(a, b) for a, b in zip(P.from_word10(words, lay), yuv)), (w, lay)
            assert np.array_equal(vithip.word10_rows(*yuv, lay), to(*yuv))


def test_lay_out_places_lead_padding_and_gaps():
    rng = np.random.default_rng(3)
    frames = [tuple(rng.integers(0, 256, (4, 5), dtype=np.uint8) for _ in range(3)), tuple(rng.integers(0, 256, (3, 6), dtype=np.uint8) for _ in range(3))]
    buf, desc = P.lay_out(frames, [None, (1.0, 0.0, 5.0, 3.0)], [P.BGR, P.ARGB], pad=3, lead=5, gap=2)
    assert (desc[0].offset, desc[0].row_stride, desc[1].offset, desc[1].row_stride) == (5, 18, 5 + 3 * 18 + 15 + 2, 27)
    assert buf.size == desc[1].offset + 2 * 27 + 24 + 2 and list(desc[1].box) == [1.0, 0.0, 5.0, 3.0]
    for d, comps in zip(desc, frames):
        n = d.width * P.samples(d.layout)
        rows = np.stack([buf[d.offset + r * d.row_stride:d.offset + r * d.row_stride + n] for r in range(d.height)])
        assert all(np.array_equal(a, b) for a, b in zip(P.deinterleave(rows, d.width, d.layout), comps))
    assert (buf[:5] == P.FILL).all() and (buf[-2:] == P.FILL).all()
    tight, _ = P.lay_out(frames, [None, None], [P.BGR, P.ARGB], pad=3, lead=5, gap=2, last_gap=False)
    assert tight.size == buf.size - 2 and np.array_equal(tight, buf[:-2])
