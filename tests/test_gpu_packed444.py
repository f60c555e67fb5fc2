"""GPU suite of the packed 4:4:4 entry points (include/vithip.h, "Packed 4:4:4 frames").  Every comparison is exact.

1. The taps vh_op_resize_bgra / vh_op_resize_y410 EQUAL vh_op_resize_yuv / vh_op_resize_yuv16 (sub (1, 1)) of the de-interleaved planes
   (YUV layouts) or vh_op_resize_u8 of the tight R G B frame (RGB layouts), AND yuv_ref.resize_yuv_f32, the fp32 emulation (RGB layouts:
   under the pass-through matrix, whose nested fmaf returns the resampled sample itself).
2. A Y410 and a V410 frame equal the Y416 frame holding code << 6.  3. Every alignment path gives the bytes of the aligned one, and a
   frame may end with its buffer.  4. Bands and batches, mixed layouts in one launch.  5. The logits of every entry point EQUAL those
   of forward_u8 given the tap's own output.  6. One resize launch, one frames ring for every kind of submit, refusals enqueue nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import nv12_ref as N
import packed444_ref as P
import vh_synth as S
import vithip
import yuv_ref as Y
from test_gpu_frames import PATCH14_MICRO, DTNAME, make_frame, same_bits
from test_gpu_frames import check_against_statement as check_rgb_statement
from test_gpu_frames import tap as tap_rgb
from test_gpu_yuv16 import colour16, device_logits, p010_set, run_tap, tap16
from test_gpu_yuv_planar import PASS_THROUGH, planner_boundary_444
from test_gpu_yuv_planar import tap as tap_yuv
from test_nv12 import make_nv12, make_rgb
from test_packed444 import PACKED_CASES
from test_yuv16 import make_yuv16
from test_yuv_planar import COLOURS, make_yuv

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE = 1, 3
P010 = "bt709_limited_10_msb_left"                                   # the default 16-bit colour state: Y410 under the code * 64 rule
COLOURS_Y410 = [P010, "bt709_full_16_msb_centre"]
CODES10 = "bt2020_limited_10_lsb_left"                               # make_yuv16 planes of 10-bit codes in the low bits
SITE = N.CHROMA_LEFT                                                 # nothing is sub-sampled: the siting is handed over and unread
UNREAD = np.full((3, 4), 12345.0, np.float32)                        # the matrix of a call whose layouts are all RGB


def tap_bgra(frames, boxes, s, m, layouts, site=SITE, **layout):
    return run_tap(vithip.op_resize_bgra, *P.lay_out(frames, boxes, layouts, **layout), s, m, site)


def tap_y410(frames, boxes, s, m, layouts, site=SITE, **layout):
    return run_tap(vithip.op_resize_y410, *P.lay_out(frames, boxes, layouts, **layout), s, m, site)


def rgb_planes(h, w, seed):
    rgb = make_rgb(h, w, seed)
    return tuple(np.ascontiguousarray(rgb[..., k]) for k in range(3))


def pixels(comps):
    return np.ascontiguousarray(np.stack(comps, axis=-1))


def shl6(yuv):
    """10-bit codes -> the Y416 / P010 words of the same codes."""
    return tuple((a << 6).astype(np.uint16) for a in yuv)


def with_extremes(yuv):
    """Codes 0 and 1023 in every component."""
    for a in yuv:
        a[0, 0], a[-1, -1] = 1023, 0
        if a.shape[1] > 2:
            a[0, 1], a[-1, -2] = 0, 1023
    return yuv


# ---- 1. the planar / RGB tap and the emulation ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_rgb(name):
    """(the RGB-ordered frame, vh_op_resize_u8's bytes, the emulation, the six packed taps) of one case; computed once."""
    h, w, box, s = PACKED_CASES[name]
    comps = rgb_planes(h, w, h + w)
    want = tap_rgb([pixels(comps)], [box], s)[0]
    ref = Y.resize_yuv_f32(*comps, box, s, PASS_THROUGH, SITE, P.SUB)
    return comps, want, ref, {key: tap_bgra([comps], [box], s, UNREAD, lay)[0] for key, lay in P.RGB_LAYOUTS.items()}


@functools.lru_cache(maxsize=None)
def case8(name, colour):
    h, w, box, s = PACKED_CASES[name]
    std, full, site = COLOURS[colour]
    m = vithip.yuv_matrix(std, full)
    yuv = make_yuv(h, w, P.SUB, seed=h + w)
    planar = tap_yuv([yuv], [box], s, m, site, subs=[P.SUB])[0]
    ref = Y.resize_yuv_f32(*yuv, box, s, m, site, P.SUB)
    return planar, ref, {key: tap_bgra([yuv], [box], s, m, lay, site)[0] for key, lay in P.YUV_LAYOUTS.items()}


@functools.lru_cache(maxsize=None)
def case16(name, colour):
    h, w, box, s = PACKED_CASES[name]
    m, site, _ = colour16(colour)
    yuv = make_yuv16(h, w, P.SUB, seed=h + w, colour=colour)
    planar = tap16([yuv], [box], s, m, site, subs=[P.SUB])[0]
    ref = Y.resize_yuv_f32(*yuv, box, s, m, site, P.SUB)
    return planar, ref, {key: tap_y410([yuv], [box], s, m, lay, site)[0] for key, lay in P.WORD_LAYOUTS.items()}


@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_rgb_layouts_equal_op_resize_u8_of_the_tight_rgb_frame(name):
    _, want, _, packed = case_rgb(name)
    for key in P.RGB_LAYOUTS:
        assert np.array_equal(packed[key], want), key


@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_rgb_layouts_match_the_emulation_and_the_statement(name):
    comps, _, ref, packed = case_rgb(name)
    h, w, box, s = PACKED_CASES[name]
    for key in P.RGB_LAYOUTS:
        assert np.array_equal(packed[key], ref), key
    check_rgb_statement(packed["bgra"][None], [pixels(comps)], [box], s)


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_yuv_layouts_equal_the_planar_444_tap_of_the_de_interleaved_planes(name, colour):
    planar, _, packed = case8(name, colour)
    for key in P.YUV_LAYOUTS:
        assert np.array_equal(packed[key], planar), key


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_yuv_layouts_match_the_emulation(name, colour):
    _, ref, packed = case8(name, colour)
    for key in P.YUV_LAYOUTS:
        assert np.array_equal(packed[key], ref), key


@pytest.mark.parametrize("colour", COLOURS_Y410)
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_y416_and_ayuv64_equal_the_planar_16_bit_tap_and_the_emulation(name, colour):
    planar, ref, packed = case16(name, colour)
    for key in P.WORD_LAYOUTS:
        assert np.array_equal(packed[key], planar), key
        assert np.array_equal(packed[key], ref), key


def test_an_unnamed_layout_word_is_taken_by_its_fields():
    """G B R X: no constant names it, the kernel reads positions."""
    h, w, box, s = PACKED_CASES["odd_37x53_16"]
    comps, want, _, _ = case_rgb("odd_37x53_16")
    assert np.array_equal(tap_bgra([comps], [box], s, UNREAD, vithip.layout_444(2, 0, 1, True, False))[0], want)
    assert np.array_equal(tap_bgra([comps], [box], s, UNREAD, vithip.layout_444(1, 2, 0, False, False))[0], want)


def test_an_rgb_layout_is_unaffected_by_the_colour_state_and_a_yuv_layout_by_the_siting():
    h, w, box, s = PACKED_CASES["fractional_box_98x132_28"]
    comps, want, _, _ = case_rgb("fractional_box_98x132_28")
    for m in (vithip.yuv_matrix(), vithip.yuv_matrix(vithip.YUV_BT601, True), np.zeros((3, 4), np.float32)):
        for site in (N.CHROMA_CENTER, N.CHROMA_LEFT):
            assert np.array_equal(tap_bgra([comps], [box], s, m, P.BGRA, site)[0], want)
            assert np.array_equal(tap_bgra([comps], [box], s, m, P.BGR, site)[0], want)
    planar, _, packed = case8("fractional_box_98x132_28", "bt709_limited_left")
    yuv = make_yuv(h, w, P.SUB, seed=h + w)
    for site in (N.CHROMA_CENTER, N.CHROMA_LEFT):
        assert np.array_equal(tap_bgra([yuv], [box], s, vithip.yuv_matrix(), P.VUYA, site)[0], planar)
    # ... through the context too: vh_set_frame_colour moves a VUYA frame and leaves a BGRA frame where it was
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=2)
    ctx.init_weights_seeded(17)
    try:
        rgb, yuv = [rgb_planes(s + 5, s + 9, 2)], [make_yuv(s + 5, s + 9, P.SUB, seed=2)]
        a_rgb, a_yuv = ctx.forward_frames_bgra(rgb, P.BGRA), ctx.forward_frames_bgra(yuv, P.VUYA)
        ctx.set_frame_colour(vithip.yuv_matrix(vithip.YUV_BT601, True), vithip.CHROMA_CENTER)
        assert same_bits(ctx.forward_frames_bgra(rgb, P.BGRA), a_rgb)
        moved = ctx.forward_frames_bgra(yuv, P.VUYA)
        assert not np.array_equal(moved, a_yuv)
        ctx.set_frame_colour(vithip.yuv_matrix(vithip.YUV_BT601, True), vithip.CHROMA_LEFT)
        assert same_bits(ctx.forward_frames_bgra(yuv, P.VUYA), moved)
        assert same_bits(ctx.forward_frames_bgra(rgb, P.BGRA), ctx.forward_frames([pixels(rgb[0])]))
    finally:
        ctx.close()


# ---- 2. Y410 and V410 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", COLOURS_Y410)
@pytest.mark.parametrize("w", [1, 2, 3, 53, 54])
def test_y410_and_v410_equal_the_y416_frame_of_the_same_codes(w, colour):
    """Codes 0 and 1023 in every component; the ignored bits (30-31 of Y410, 0-1 of V410) set."""
    h, s = 5, 16
    m, site, _ = colour16(colour)
    codes = with_extremes(make_yuv16(h, w, P.SUB, w, CODES10))
    assert all(int(a.min()) == 0 and int(a.max()) == 1023 for a in codes)
    want = tap_y410([shl6(codes)], [None], s, m, P.Y416)
    assert np.array_equal(want, tap16([shl6(codes)], [None], s, m, site, subs=[P.SUB]))
    assert np.array_equal(want[0], Y.resize_yuv_f32(*shl6(codes), None, s, m, site, P.SUB))
    for lay, mask, shift in ((P.Y410, 3, 30), (P.V410, 3, 0)):
        buf, desc = P.lay_out([codes], [None], lay, ignored=3)
        assert ((buf.view("<u4") >> shift) & mask == 3).all() and desc[0].row_stride == 4 * w
        assert np.array_equal(run_tap(vithip.op_resize_y410, buf, desc, s, m, site), want), lay
        assert np.array_equal(tap_y410([codes], [None], s, m, lay), want), lay            # the ignored bits clear


@pytest.mark.parametrize("colour", COLOURS_Y410)
def test_y410_and_v410_boxes_and_the_operator_cases(colour):
    m, site, _ = colour16(colour)
    for name, (h, w, box, s) in PACKED_CASES.items():
        codes = make_yuv16(h, w, P.SUB, h + w, CODES10)
        want = tap16([shl6(codes)], [box], s, m, site, subs=[P.SUB])
        assert np.array_equal(tap_y410([codes], [box], s, m, P.Y410, ignored=1), want), name
        assert np.array_equal(tap_y410([codes], [box], s, m, P.V410, ignored=2), want), name


# ---- 3. alignment ---------------------------------------------------------------------------------------------------------------
BOXES2 = [None, (0.5, 3.0, 29.5, 40.0)]


def test_8_bit_offsets_and_strides_of_any_alignment_give_the_same_bytes():
    m = vithip.yuv_matrix()
    frames = [rgb_planes(37, 53, 21), make_yuv(42, 30, P.SUB, seed=31)]
    for lays in ([P.BGRA, P.VUYA], [P.ARGB, P.AYUV], [P.BGR, P.YUV24]):
        buf, desc = P.lay_out(frames, BOXES2, lays)
        if lays[0] & 64:
            assert all(d.offset % 4 == 0 and d.row_stride % 4 == 0 for d in desc)                   # one 32-bit load per pixel
        want = tap_bgra(frames, BOXES2, 16, m, lays)
        assert np.array_equal(want[0], tap_rgb([pixels(frames[0])], BOXES2[:1], 16)[0])
        assert np.array_equal(want[1], tap_yuv(frames[1:], BOXES2[1:], 16, m, SITE, subs=[P.SUB])[0])
        for lead in (0, 1, 2, 3):
            for pad in (0, 1, 2, 3):
                assert np.array_equal(tap_bgra(frames, BOXES2, 16, m, lays, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def test_16_bit_offsets_and_strides_of_any_even_alignment_give_the_same_bytes():
    m, site, _ = colour16(P010)
    frames = [make_yuv16(37, 53, P.SUB, 21, P010), make_yuv16(42, 30, P.SUB, 31, P010)]
    lays = [P.Y416, P.AYUV64]
    buf, desc = P.lay_out(frames, BOXES2, lays)
    assert all(d.offset % 8 == 0 and d.row_stride % 8 == 0 for d in desc)                           # one 64-bit load per pixel
    want = tap_y410(frames, BOXES2, 16, m, lays)
    assert np.array_equal(want, tap16(frames, BOXES2, 16, m, site, subs=[P.SUB] * 2))
    for lead in (0, 2, 4, 6):
        for pad in (0, 2, 4, 6):
            assert np.array_equal(tap_y410(frames, BOXES2, 16, m, lays, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def test_10_bit_offsets_and_strides_of_any_multiple_of_4_give_the_same_bytes():
    m, site, _ = colour16(P010)
    frames = [make_yuv16(37, 53, P.SUB, 21, CODES10), make_yuv16(42, 30, P.SUB, 31, CODES10)]
    lays = [P.Y410, P.V410]
    want = tap_y410(frames, BOXES2, 16, m, lays)
    assert np.array_equal(want, tap16([shl6(p) for p in frames], BOXES2, 16, m, site, subs=[P.SUB] * 2))
    for lead in (0, 4, 8, 12):
        for pad in (0, 4):
            assert np.array_equal(tap_y410(frames, BOXES2, 16, m, lays, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def at_base(op, buf, desc, s, m, step, tail=0):
    """The tap on the frames `step` bytes into a device buffer that ends `tail` bytes behind them."""
    n = len(desc) * s * s * 3
    din = vithip.DeviceBuffer.from_numpy(np.concatenate([np.full(step, 0xEE, np.uint8), buf, np.full(tail, 0xEE, np.uint8)]))
    dout = vithip.DeviceBuffer.from_numpy(np.zeros(n, np.uint8))
    try:
        op(din.ptr + step, buf.nbytes, desc, s, m, SITE, dout.ptr)
        return dout.to_numpy(np.uint8, (n,)).reshape(len(desc), s, s, 3)
    finally:
        din.free(); dout.free()


def test_a_device_pointer_that_breaks_the_pixel_alignment_gives_the_same_bytes():
    """The base address enters the load choice like an offset: 4-byte pixels at bases 1, 2, 3 mod 4, 16-bit words at 2, 4, 6 mod 8,
    10-bit words at 4 mod 8."""
    s = 16
    for op, frames, lays, m, steps in (
            (vithip.op_resize_bgra, [rgb_planes(37, 53, 21)], P.BGRA, UNREAD, (1, 2, 3)),
            (vithip.op_resize_bgra, [make_yuv(37, 53, P.SUB, seed=21)], P.VUYA, vithip.yuv_matrix(), (1, 2, 3)),
            (vithip.op_resize_bgra, [rgb_planes(37, 53, 21)], P.BGR, UNREAD, (1, 2, 3)),
            (vithip.op_resize_y410, [make_yuv16(37, 53, P.SUB, 21, P010)], P.Y416, vithip.yuv_matrix16(), (2, 4, 6)),
            (vithip.op_resize_y410, [make_yuv16(37, 53, P.SUB, 21, CODES10)], P.V410, vithip.yuv_matrix16(), (4,))):
        buf, desc = P.lay_out(frames, [None], lays)
        want = run_tap(op, buf, desc, s, m, SITE)
        for step in steps:
            assert np.array_equal(at_base(op, buf, desc, s, m, step), want), (lays, step)


@pytest.mark.parametrize("key", ["bgr", "yuv24", "bgra", "argb"])
def test_a_frame_may_end_at_the_last_byte_of_an_exact_size_device_buffer(key):
    """3-byte and 4-byte pixels, the frame's span ending where the allocation ends, at every base residue mod 4; the bytes are those
    of the same frame with room behind it."""
    lay = dict(P.RGB_LAYOUTS, **P.YUV_LAYOUTS)[key]
    m = vithip.yuv_matrix()
    for h, w in ((5, 3), (7, 54)):
        comps = rgb_planes(h, w, 9)
        buf, desc = P.lay_out([comps], [None], lay)
        assert buf.nbytes == desc[0].offset + (h - 1) * desc[0].row_stride + w * P.samples(lay) == h * w * P.samples(lay)
        want = at_base(vithip.op_resize_bgra, buf, desc, 16, m, 0, tail=64)
        for step in (0, 1, 2, 3):
            assert np.array_equal(at_base(vithip.op_resize_bgra, buf, desc, 16, m, step), want), (h, w, step)


# ---- 4. bands and batches -------------------------------------------------------------------------------------------------------
def test_one_1080p_bgra_and_one_y410_frame_span_many_bands():
    s = S.CONFIGS["vit_micro"]["image_size"]
    box = [vithip.center_crop_box(1080, 1920)]
    comps = rgb_planes(1080, 1920, 3)
    assert np.array_equal(tap_bgra([comps], box, s, UNREAD, P.BGRA), tap_rgb([pixels(comps)], box, s))
    codes = make_yuv16(1080, 1920, P.SUB, 3, CODES10)
    m, site, _ = colour16(P010)
    assert np.array_equal(tap_y410([codes], box, s, m, P.Y410, ignored=2), tap16([shl6(codes)], box, s, m, site, subs=[P.SUB]))


SHAPES7 = [(37, 53), (64, 64), (20, 24), (98, 132), (270, 480), (1, 1), (33, 2)]
BOXES7 = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]


def test_mixed_batch_of_layouts_sizes_and_boxes_in_one_launch():
    """BGR, BGRA, ARGB and VUYA (and RGB, AYUV, YUV24) frames of different sizes in ONE launch: matrix and no matrix, one load and
    three per tap are workgroup-uniform branches."""
    m = vithip.yuv_matrix(vithip.YUV_BT601, True)
    lays = [P.BGR, P.BGRA, P.ARGB, P.VUYA, P.RGB, P.AYUV, P.YUV24]
    frames = [make_yuv(h, w, P.SUB, seed=40 + i) if P.is_yuv(lay) else rgb_planes(h, w, 40 + i) for i, ((h, w), lay) in enumerate(zip(SHAPES7, lays))]
    got = tap_bgra(frames, BOXES7, 32, m, lays, lead=1, gap=3, pad=1)
    for i, lay in enumerate(lays):
        alone = (tap_yuv([frames[i]], [BOXES7[i]], 32, m, SITE, subs=[P.SUB]) if P.is_yuv(lay) else tap_rgb([pixels(frames[i])], [BOXES7[i]], 32))[0]
        assert np.array_equal(got[i], alone), i
        assert np.array_equal(tap_bgra([frames[i]], [BOXES7[i]], 32, m, lay)[0], got[i]), i        # each frame alone: the same bytes
    # Y416, AYUV64, Y410 and V410 in one batch: the layout is the frame's, the kernel the batch's
    m, site, _ = colour16(P010)
    lays = [P.Y416, P.Y410, P.V410, P.AYUV64, P.V410, P.Y416, P.Y410]
    codes = [make_yuv16(h, w, P.SUB, 40 + i, CODES10) for i, (h, w) in enumerate(SHAPES7)]
    frames = [c if lay & 256 else shl6(c) for c, lay in zip(codes, lays)]
    got = tap_y410(frames, BOXES7, 32, m, lays, lead=4, gap=4)
    assert np.array_equal(got, tap16([shl6(c) for c in codes], BOXES7, 32, m, site, subs=[P.SUB] * 7))
    for i in range(7):
        assert np.array_equal(tap_y410([frames[i]], [BOXES7[i]], 32, m, lays[i])[0], got[i])


def test_large_batch_of_small_frames_runs_tall_bands():
    boxes = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    m = vithip.yuv_matrix()
    yuv = [make_yuv(41, 39, P.SUB, seed=100 + i) for i in range(40)]
    every = list(P.YUV_LAYOUTS.values())
    got = tap_bgra(yuv, boxes, 32, m, [every[i % 3] for i in range(40)])
    assert np.array_equal(got, tap_yuv(yuv, boxes, 32, m, SITE, subs=[P.SUB] * 40))
    for i in (0, 5, 18, 39):
        assert np.array_equal(got[i], Y.resize_yuv_f32(*yuv[i], boxes[i], 32, m, SITE, P.SUB))
    every = list(P.RGB_LAYOUTS.values())
    assert np.array_equal(tap_bgra(yuv, boxes, 32, UNREAD, [every[i % 6] for i in range(40)]), tap_rgb([pixels(c) for c in yuv], boxes, 32))
    m, site, _ = colour16(P010)
    codes = [make_yuv16(41, 39, P.SUB, 100 + i, CODES10) for i in range(40)]
    lays = [(P.Y410, P.V410, P.Y416)[i % 3] for i in range(40)]
    got = tap_y410([c if lay & 256 else shl6(c) for c, lay in zip(codes, lays)], boxes, 32, m, lays)
    assert np.array_equal(got, tap16([shl6(c) for c in codes], boxes, 32, m, site, subs=[P.SUB] * 40))


@pytest.mark.parametrize("which", ["largest_full_width", "smallest_narrowed"])
def test_the_two_frames_either_side_of_the_444_planner_boundary(which):
    """S = 130: an output row of t vertical taps costs 3 t floats per column, as the planar 4:4:4 frame does; 42 taps keep the full
    width, 43 narrow the column tiles (test_gpu_yuv_planar has the derivation)."""
    s = 130
    h_full, h_narrow = planner_boundary_444(s)
    h = h_full if which == "largest_full_width" else h_narrow
    yc = N.axis_table(h, 0.0, float(h), s)[1]
    assert (int(3 * yc.max()) > 16384 // s) == (which == "smallest_narrowed")
    m = vithip.yuv_matrix()
    yuv = make_yuv(h, 36, P.SUB, seed=7)
    want = tap_yuv([yuv], [None], s, m, SITE, subs=[P.SUB])
    assert np.array_equal(tap_bgra([yuv], [None], s, m, P.VUYA), want)
    assert np.array_equal(tap_bgra([yuv], [None], s, UNREAD, P.BGR), tap_rgb([pixels(yuv)], [None], s))
    m16, site, _ = colour16(P010)
    codes = make_yuv16(h, 36, P.SUB, 7, CODES10)
    assert np.array_equal(tap_y410([codes], [None], s, m16, P.V410), tap16([shl6(codes)], [None], s, m16, site, subs=[P.SUB]))


# ---- 5. the forward -------------------------------------------------------------------------------------------------------------
def bgra_set(s):
    """Three 8-bit frames: a BGRA one with a centre crop, an odd VUYA one, a small BGR one with a fractional box."""
    shapes = [(s + 16, s + 36), (s + 1, s + 3), (s // 2 + 6, s // 2 + 23)]
    lays = [P.BGRA, P.VUYA, P.BGR]
    frames = [make_yuv(h, w, P.SUB, seed=1 + i) if P.is_yuv(lay) else rgb_planes(h, w, 1 + i) for i, ((h, w), lay) in enumerate(zip(shapes, lays))]
    return frames, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)], lays


def y410_set(s):
    """The same shapes as a Y416 frame, a Y410 frame and a V410 frame."""
    shapes = [(s + 16, s + 36), (s + 1, s + 3), (s // 2 + 6, s // 2 + 23)]
    codes = [make_yuv16(h, w, P.SUB, 11 + i, CODES10) for i, (h, w) in enumerate(shapes)]
    lays = [P.Y416, P.Y410, P.V410]
    frames = [c if lay & 256 else shl6(c) for c, lay in zip(codes, lays)]
    return frames, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)], lays


FORWARD_CASES = [("vit_micro", S.CONFIGS["vit_micro"], vithip.DTYPE_BF16), ("patch14_micro", PATCH14_MICRO, vithip.DTYPE_BF16),
                 ("vit_micro", S.CONFIGS["vit_micro"], vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_every_packed_444_entry_point_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    m8, _ = ctx.get_frame_colour()
    m16, _ = ctx.get_frame_colour16()
    p8, b8, l8 = bgra_set(s)
    p16, b16, l16 = y410_set(s)
    want8 = ctx.forward_u8(tap_bgra(p8, b8, s, m8, l8))
    want16 = ctx.forward_u8(tap_y410(p16, b16, s, m16, l16))
    assert np.isfinite(want8).all() and np.isfinite(want16).all() and not np.array_equal(want8, want16)
    assert same_bits(ctx.forward_frames_bgra(p8, l8, b8), want8)
    assert same_bits(ctx.forward_frames_y410(p16, l16, b16), want16)
    buf8, desc8 = P.lay_out(p8, b8, l8, lead=3, pad=1, gap=2)
    assert same_bits(ctx.forward_frames_bgra_packed(buf8, desc8), want8)
    assert same_bits(device_logits(ctx.forward_device_frames_bgra, buf8, desc8, cfg["classes"]), want8)
    buf16, desc16 = P.lay_out(p16, b16, l16, lead=4, pad=4, gap=4, ignored=3)
    assert same_bits(ctx.forward_frames_y410_packed(buf16, desc16), want16)
    assert same_bits(device_logits(ctx.forward_device_frames_y410, buf16, desc16, cfg["classes"]), want16)
    ctx.ring_create_frames(2, 3, max(buf8.nbytes, buf16.nbytes))
    try:
        ctx.ring_submit_frames_bgra(p8, l8, b8)
        ctx.ring_submit_frames_y410_packed(buf16, buf16.nbytes, desc16)
        assert same_bits(ctx.ring_collect(), want8) and same_bits(ctx.ring_collect(), want16)
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)
    ctx.close()


@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
    ctx.init_weights_seeded(17)
    set8, set16 = bgra_set(s), y410_set(s)
    m8, _ = ctx.get_frame_colour()
    m16, _ = ctx.get_frame_colour16()
    ref8 = ctx.forward_u8(tap_bgra(set8[0], set8[1], s, m8, set8[2]))              # computed once; the tests below only read them
    ref16 = ctx.forward_u8(tap_y410(set16[0], set16[1], s, m16, set16[2]))
    ref8.setflags(write=False); ref16.setflags(write=False)
    yield ctx, cfg, set8, ref8, set16, ref16
    ctx.close()


def test_device_entry_points_with_streams_and_graphs(micro):
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    buf8, desc8 = P.lay_out(p8, b8, l8, lead=1, pad=2)
    buf16, desc16 = P.lay_out(p16, b16, l16, lead=4, gap=4)
    din8, din16 = vithip.DeviceBuffer.from_numpy(buf8), vithip.DeviceBuffer.from_numpy(buf16)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    logits = lambda: dout.to_numpy(np.float32, (3, cfg["classes"]))
    try:
        ctx.set_streams(2)                                                         # the resize runs once, before the fork
        ctx.set_graph(True)
        for _ in range(3):                                                         # eager, captured, replayed
            ctx.forward_device_frames_bgra(din8.ptr, buf8.nbytes, desc8, dout.ptr)
            assert same_bits(logits(), ref8)
        assert ctx.get_graph()[0] and ctx.get_graph()[1] >= 1
        # other frames, of the other depth, through the replayed graph: the resize in front of it is no part of the capture
        ctx.forward_device_frames_y410(din16.ptr, buf16.nbytes, desc16, dout.ptr)
        assert same_bits(logits(), ref16)
        assert same_bits(ctx.forward_frames_bgra(p8[::-1], l8[::-1], b8[::-1]), ref8[::-1])
        assert same_bits(ctx.forward_frames_y410(p16, l16, b16), ref16)
    finally:
        ctx.set_graph(False)
        ctx.set_streams(1)
        din8.free(); din16.free(); dout.free()


# ---- 6. state and ring ----------------------------------------------------------------------------------------------------------
def test_stage_timing_reports_one_resize_launch(micro):
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    try:
        ctx.set_stage_timing("resize")
        for call, args, want in ((ctx.forward_frames_bgra, (p8, l8, b8), ref8), (ctx.forward_frames_y410, (p16, l16, b16), ref16)):
            assert same_bits(call(*args), want)
            avg, mn, n = ctx.get_stage_timing()
            assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_frames_ring_takes_rgb_nv12_yuy2_bgra_vuya_p016_and_y410_alternately(micro):
    import packed422_ref as P422
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    s = cfg["image_size"]
    rgb = [make_frame(s + 7, s + 2, 3, seed=5), make_frame(s, s + 9, 3, seed=6)]
    ref_rgb = ctx.forward_frames(rgb)
    nv12 = [make_nv12(s + 4, s + 10, seed=12)]
    ref_nv12 = ctx.forward_frames_nv12(nv12)
    yuy2 = [make_yuv(s + 3, s + 5, P422.SUB, seed=8)]
    ref_yuy2 = ctx.forward_frames_yuy2(yuy2, P422.UYVY)
    pairs, pboxes = p010_set(s)
    ref_p016 = ctx.forward_frames_p016(pairs, pboxes)
    assert l8[0] == P.BGRA and l8[1] == P.VUYA
    bgra, vuya = ([p8[0], p8[2]], [l8[0], l8[2]], [b8[0], b8[2]]), ([p8[1]], [l8[1]], [b8[1]])
    ctx.ring_create_frames(7, 3, 1 << 17)
    try:
        ctx.ring_submit_frames(rgb)
        ctx.ring_submit_frames_nv12(nv12)
        ctx.ring_submit_frames_yuy2(yuy2, P422.UYVY)
        ctx.ring_submit_frames_bgra(*bgra)
        # slot 5: a VUYA frame filled in place, 3 bytes into the slot
        buf, desc = P.lay_out(vuya[0], vuya[2], vuya[1], lead=3)
        ctx.ring_input_frames()[:buf.size] = buf
        ctx.ring_submit_frames_bgra_packed(None, buf.size, desc)
        ctx.ring_submit_frames_p016(pairs, pboxes)
        ctx.ring_submit_frames_y410(p16, l16, b16)
        assert ctx.ring_free_slots() == 0
        assert same_bits(ctx.ring_collect(), ref_rgb)                              # FIFO
        ctx.ring_submit_frames_bgra(p8[::-1], l8[::-1], b8[::-1])
        assert same_bits(ctx.ring_collect(), ref_nv12)
        assert same_bits(ctx.ring_collect(), ref_yuy2)
        assert same_bits(ctx.ring_collect(), ref8[[0, 2]])
        assert same_bits(ctx.ring_collect(), ref8[[1]])
        assert same_bits(ctx.ring_collect(), ref_p016)
        assert same_bits(ctx.ring_collect(), ref16)
        assert same_bits(ctx.ring_collect(), ref8[::-1])
        assert ctx.ring_free_slots() == 7
        # a refused submit leaves the ring as it was and enqueues nothing
        buf, desc = P.lay_out(p8[:1], b8[:1], l8[:1])
        desc[0].row_stride -= 1
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_bgra_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "row_stride <" in str(e.value) and ctx.ring_free_slots() == 7
        desc[0].row_stride += 1
        desc[0].layout = P.Y410
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_bgra_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "10-bit layouts" in str(e.value) and ctx.ring_free_slots() == 7
        buf, desc = P.lay_out(p16[1:2], b16[1:2], l16[1:2])
        desc[0].offset += 2
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_y410_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "multiple of 4" in str(e.value) and ctx.ring_free_slots() == 7
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_collect()
        assert e.value.code == 7                                                   # VH_ERR_RING_EMPTY: nothing was enqueued
        ctx.ring_submit_frames_y410(p16[1:2], l16[1:2], b16[1:2])
        assert same_bits(ctx.ring_collect(), ref16[[1]])
        # packed submits on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            for call, args in ((ctx.ring_submit_frames_bgra, (p8[:1], l8[:1], b8[:1])), (ctx.ring_submit_frames_y410, (p16[:1], l16[:1], b16[:1]))):
                with pytest.raises(vithip.VhError) as e:
                    call(*args)
                assert e.value.code == VH_ERR_STATE and ctx.ring_free_slots() == 2
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


def test_refusals_enqueue_nothing(micro):
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    L = vithip.lib()
    buf8, desc8 = P.lay_out(p8, b8, l8)
    buf16, desc16 = P.lay_out(p16, b16, l16)
    out = np.zeros((3, cfg["classes"]), np.float32)

    def call8(n=3, nbytes=buf8.nbytes, d=desc8):
        return L.vh_forward_frames_bgra(ctx.h, buf8.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    def call16(n=3, nbytes=buf16.nbytes, d=desc16):
        return L.vh_forward_frames_y410(ctx.h, buf16.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    err = lambda: L.vh_last_error(ctx.h).decode()
    assert call8(n=4) == VH_ERR_INVALID and call16(n=4) == VH_ERR_INVALID          # batch > max_batch
    assert call8(nbytes=buf8.nbytes - 1) == VH_ERR_INVALID and "ends beyond nbytes" in err()
    assert call16(nbytes=buf16.nbytes - 1) == VH_ERR_INVALID and "ends beyond nbytes" in err()
    assert call8(d=None) == VH_ERR_INVALID and call16(d=None) == VH_ERR_INVALID
    desc8[1].layout = P.Y410
    assert call8() == VH_ERR_INVALID and "10-bit layouts" in err()
    desc8[1].layout = 1 << 12
    assert call8() == VH_ERR_INVALID and "bits outside" in err()
    desc8[1].layout = l8[1]
    desc8[2].layout = vithip.layout_444(0, 3, 1, False, False)
    assert call8() == VH_ERR_INVALID and "position 3" in err()
    desc8[2].layout = l8[2]
    desc16[0].layout = P.BGRA
    assert call16() == VH_ERR_INVALID and "RGB words" in err()
    desc16[0].layout = l16[0]
    desc16[0].offset += 1
    assert call16() == VH_ERR_INVALID and "offset is odd" in err()
    desc16[0].offset -= 1
    desc16[1].row_stride += 2
    assert call16() == VH_ERR_INVALID and "row_stride is no multiple of 4" in err()
    desc16[1].row_stride -= 2
    desc16[2].box[2] = desc16[2].width + 0.5
    assert call16() == VH_ERR_INVALID and "box outside" in err()
    desc16[2].box[2] = b16[2][2]
    assert not out.any()                                                           # nothing ran
    # a device frames pointer of the wrong alignment is refused before the device is asked anything
    dev = vithip.DeviceBuffer.from_numpy(np.concatenate([np.zeros(4, np.uint8), buf16]))
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    try:
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_frames_y410(dev.ptr + 1, buf16.nbytes, desc16, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "frames pointer is odd" in str(e.value)
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_frames_y410(dev.ptr + 2, buf16.nbytes, desc16, dout.ptr)     # the batch holds Y410 and V410 frames
        assert e.value.code == VH_ERR_INVALID and "frames pointer is no multiple of 4" in str(e.value)
        assert not dout.to_numpy(np.float32, (3, cfg["classes"])).any()
        ctx.forward_device_frames_y410(dev.ptr + 4, buf16.nbytes, desc16, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref16)
    finally:
        dev.free(); dout.free()
    assert same_bits(ctx.forward_frames_bgra(p8, l8, b8), ref8)
    # a context with one channel is refused, and goes on working
    c1 = vithip.VitContext(dict(cfg, channels=1), dtype=vithip.DTYPE_BF16, max_batch=3)
    c1.init_weights_seeded(5)
    grey = [make_frame(cfg["image_size"], cfg["image_size"], 1, seed=4)]
    before = c1.forward_frames(grey)
    for callc, args in ((c1.forward_frames_bgra, (p8, l8, b8)), (c1.forward_frames_y410, (p16, l16, b16))):
        with pytest.raises(vithip.VhError) as e:
            callc(*args)
        assert e.value.code == VH_ERR_INVALID and "3 channels" in str(e.value)
    assert same_bits(c1.forward_frames(grey), before)
    c1.close()
