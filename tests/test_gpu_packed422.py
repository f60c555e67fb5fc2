"""GPU suite of the packed 4:2:2 entry points (include/vithip.h, "Packed 4:2:2 frames").  Every comparison is exact.

1. The taps vh_op_resize_yuy2 / vh_op_resize_y210 EQUAL vh_op_resize_yuv / vh_op_resize_yuv16 (sub (2, 1)) of the de-interleaved planes,
   and yuv_ref.resize_yuv_f32 of them, for every layout, both sitings and two colour states per depth.
2. A v210 frame equals the Y210 frame holding code << 6.  3. Every alignment path gives the bytes of the aligned one.
4. Bands and batches.  5. The logits of every entry point EQUAL those of forward_u8 given the tap's own output.
6. One resize launch, two independent colour states, one frames ring for every kind of submit, refusals enqueue nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import nv12_ref as N
import packed422_ref as P
import vh_synth as S
import vithip
import yuv16_ref as W
import yuv_ref as Y
from test_gpu_frames import PATCH14_MICRO, DTNAME, make_frame, same_bits
from test_gpu_yuv16 import colour16, device_logits, p010_set, run_tap, tap16
from test_gpu_yuv_planar import tap as tap_yuv
from test_nv12 import make_nv12, make_rgb
from test_packed422 import PACKED_CASES, V210_WIDTHS
from test_yuv16 import make_yuv16
from test_yuv_planar import COLOURS, make_yuv

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE = 1, 3
P010 = "bt709_limited_10_msb_left"                                   # the default 16-bit colour state: Y210 as drivers write it
COLOURS_Y210 = [P010, "bt709_full_16_msb_centre"]                    # left-sited limited range, centre-sited full range
CODES10 = "bt2020_limited_10_lsb_left"                               # make_yuv16 planes of 10-bit codes in the low bits
LAYOUTS = (P.YUYV, P.UYVY, P.YVYU, P.VYUY)


def tap_yuy2(planes, boxes, s, m, site, layouts, **layout):
    return run_tap(vithip.op_resize_yuy2, *P.lay_out(planes, boxes, layouts, **layout), s, m, site)


def tap_y210(planes, boxes, s, m, site, layouts, **layout):
    return run_tap(vithip.op_resize_y210, *P.lay_out(planes, boxes, layouts, **layout), s, m, site)


def shl6(yuv):
    """10-bit codes -> the Y210 / P010 words of the same codes."""
    return tuple((a << 6).astype(np.uint16) for a in yuv)


def with_extremes(yuv):
    """Codes 0 and 1023 (8-bit: 255) in every plane."""
    top = 255 if yuv[0].dtype == np.uint8 else 1023
    for a in yuv:
        a[0, 0], a[-1, -1] = top, 0
        if a.shape[1] > 2:
            a[0, 1], a[-1, -2] = 0, top
    return yuv


# ---- 1. the planar tap and the statement ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case8(name, colour):
    """(planes, planar tap, emulation, the four packed taps) of one 8-bit case; computed once, read by two tests."""
    h, w, box, s = PACKED_CASES[name]
    std, full, site = COLOURS[colour]
    m = vithip.yuv_matrix(std, full)
    yuv = make_yuv(h, w, P.SUB, seed=h + w)
    planar = tap_yuv([yuv], [box], s, m, site, subs=[P.SUB])[0]
    ref = Y.resize_yuv_f32(*yuv, box, s, m, site, P.SUB)
    return planar, ref, {lay: tap_yuy2([yuv], [box], s, m, site, lay)[0] for lay in LAYOUTS}


@functools.lru_cache(maxsize=None)
def case16(name, colour):
    h, w, box, s = PACKED_CASES[name]
    m, site, _ = colour16(colour)
    yuv = make_yuv16(h, w, P.SUB, seed=h + w, colour=colour)
    planar = tap16([yuv], [box], s, m, site, subs=[P.SUB])[0]
    ref = Y.resize_yuv_f32(*yuv, box, s, m, site, P.SUB)
    return planar, ref, {lay: tap_y210([yuv], [box], s, m, site, lay)[0] for lay in LAYOUTS}


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_op_resize_yuy2_equals_the_planar_tap_of_the_de_interleaved_planes(name, colour):
    planar, _, packed = case8(name, colour)
    for lay in LAYOUTS:
        assert np.array_equal(packed[lay], planar), P.NAMES[lay]


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_op_resize_yuy2_matches_the_statement(name, colour):
    _, ref, packed = case8(name, colour)
    for lay in LAYOUTS:
        assert np.array_equal(packed[lay], ref), P.NAMES[lay]


@pytest.mark.parametrize("colour", COLOURS_Y210)
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_op_resize_y210_equals_the_planar_16_bit_tap_of_the_de_interleaved_planes(name, colour):
    planar, _, packed = case16(name, colour)
    for lay in LAYOUTS:
        assert np.array_equal(packed[lay], planar), P.NAMES[lay]


@pytest.mark.parametrize("colour", COLOURS_Y210)
@pytest.mark.parametrize("name", list(PACKED_CASES))
def test_op_resize_y210_matches_the_statement(name, colour):
    _, ref, packed = case16(name, colour)
    for lay in LAYOUTS:
        assert np.array_equal(packed[lay], ref), P.NAMES[lay]


# ---- 2. v210 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", COLOURS_Y210)
@pytest.mark.parametrize("w", V210_WIDTHS)
def test_v210_equals_the_y210_frame_of_the_same_codes(w, colour):
    """Every width mod 6 either side of one and of nine blocks, and 1918 x 4 (320 blocks a row; -> 64, because scale <= 32); codes 0
    and 1023 in every plane; bits 30-31 of every word set."""
    h, s = (4, 64) if w == 1918 else (5, 16)
    m, site, _ = colour16(colour)
    codes = with_extremes(make_yuv16(h, w, P.SUB, w, CODES10))
    assert all(int(a.min()) == 0 and int(a.max()) == 1023 for a in codes)
    want = tap_y210([shl6(codes)], [None], s, m, site, P.YUYV)
    buf, desc = P.lay_out([codes], [None], P.V210, high_bits=3)
    assert (buf.view("<u4") >> 30 == 3).all() and desc[0].row_stride == 16 * ((w + 5) // 6)
    assert np.array_equal(run_tap(vithip.op_resize_y210, buf, desc, s, m, site), want)
    assert np.array_equal(tap_y210([codes], [None], s, m, site, P.V210), want)                      # bits 30-31 clear
    assert np.array_equal(want[0], Y.resize_yuv_f32(*shl6(codes), None, s, m, site, P.SUB))
    assert np.array_equal(want, tap16([shl6(codes)], [None], s, m, site, subs=[P.SUB]))


@pytest.mark.parametrize("colour", COLOURS_Y210)
def test_v210_boxes_and_the_operator_cases(colour):
    m, site, _ = colour16(colour)
    for name, (h, w, box, s) in PACKED_CASES.items():
        codes = make_yuv16(h, w, P.SUB, h + w, CODES10)
        want = tap16([shl6(codes)], [box], s, m, site, subs=[P.SUB])
        assert np.array_equal(tap_y210([codes], [box], s, m, site, P.V210, high_bits=1), want), name


# ---- 3. alignment ---------------------------------------------------------------------------------------------------------------
BOXES2 = [None, (0.5, 3.0, 29.5, 40.0)]


def test_8_bit_offsets_and_strides_of_any_alignment_give_the_same_bytes():
    m, site = vithip.yuv_matrix(), N.CHROMA_LEFT
    planes = [make_yuv(37, 53, P.SUB, seed=21), make_yuv(42, 30, P.SUB, seed=31)]
    for lays in ([P.UYVY, P.YVYU], [P.YUYV, P.VYUY]):
        buf, desc = P.lay_out(planes, BOXES2, lays)
        assert all(d.offset % 4 == 0 and d.row_stride % 4 == 0 for d in desc)                       # one 32-bit load per macropixel
        want = tap_yuy2(planes, BOXES2, 16, m, site, lays)
        assert np.array_equal(want, tap_yuv(planes, BOXES2, 16, m, site, subs=[P.SUB] * 2))
        for lead in (0, 1, 2, 3):
            for pad in (0, 1, 2):
                assert np.array_equal(tap_yuy2(planes, BOXES2, 16, m, site, lays, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def test_16_bit_offsets_and_strides_of_any_even_alignment_give_the_same_bytes():
    m, site, _ = colour16(P010)
    planes = [make_yuv16(37, 53, P.SUB, 21, P010), make_yuv16(42, 30, P.SUB, 31, P010)]
    for lays in ([P.YUYV, P.VYUY], [P.UYVY, P.YVYU]):
        buf, desc = P.lay_out(planes, BOXES2, lays)
        assert all(d.offset % 8 == 0 and d.row_stride % 8 == 0 for d in desc)                       # one 64-bit load per macropixel
        want = tap_y210(planes, BOXES2, 16, m, site, lays)
        assert np.array_equal(want, tap16(planes, BOXES2, 16, m, site, subs=[P.SUB] * 2))
        for lead in (0, 2, 4, 6):
            for pad in (0, 2):
                assert np.array_equal(tap_y210(planes, BOXES2, 16, m, site, lays, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def test_v210_offsets_and_strides_of_any_multiple_of_4_give_the_same_bytes():
    m, site, _ = colour16(P010)
    planes = [make_yuv16(37, 53, P.SUB, 21, CODES10), make_yuv16(42, 30, P.SUB, 31, CODES10)]
    want = tap_y210(planes, BOXES2, 16, m, site, P.V210)
    assert np.array_equal(want, tap16([shl6(p) for p in planes], BOXES2, 16, m, site, subs=[P.SUB] * 2))
    for lead in (0, 4, 8, 12):
        for pad in (0, 4):
            assert np.array_equal(tap_y210(planes, BOXES2, 16, m, site, P.V210, lead=lead, pad=pad, gap=pad), want), (lead, pad)


def test_a_device_pointer_that_breaks_the_macropixel_alignment_gives_the_same_bytes():
    """The base address enters the load choice like an offset: the same frames 1 .. 3 bytes (2 .. 6 for 16-bit words) into a buffer."""
    s = 16
    for op, planes, lays, m, site, steps in (
            (vithip.op_resize_yuy2, [make_yuv(37, 53, P.SUB, seed=21)], P.UYVY, vithip.yuv_matrix(), N.CHROMA_LEFT, (1, 2, 3)),
            (vithip.op_resize_y210, [make_yuv16(37, 53, P.SUB, 21, P010)], P.YVYU, vithip.yuv_matrix16(), N.CHROMA_LEFT, (2, 4, 6))):
        buf, desc = P.lay_out(planes, [None], lays)
        want = run_tap(op, buf, desc, s, m, site)
        n = s * s * 3
        for step in steps:
            din = vithip.DeviceBuffer.from_numpy(np.concatenate([np.full(step, 0xEE, np.uint8), buf]))
            dout = vithip.DeviceBuffer.from_numpy(np.zeros(n, np.uint8))
            try:
                op(din.ptr + step, buf.nbytes, desc, s, m, site, dout.ptr)
                assert np.array_equal(dout.to_numpy(np.uint8, (n,)).reshape(1, s, s, 3), want), step
            finally:
                din.free(); dout.free()


# ---- 4. bands and batches -------------------------------------------------------------------------------------------------------
def test_one_1080p_uyvy_and_one_v210_frame_span_many_bands():
    s = S.CONFIGS["vit_micro"]["image_size"]
    rgb = make_rgb(1080, 1920, 3)
    box = [vithip.center_crop_box(1080, 1920)]
    yuv = Y.rgb_to_yuv_planes(rgb, *P.SUB)
    m, site = vithip.yuv_matrix(), N.CHROMA_LEFT
    assert np.array_equal(tap_yuy2([yuv], box, s, m, site, P.UYVY), tap_yuv([yuv], box, s, m, site, subs=[P.SUB]))
    codes = W.rgb_to_yuv16_planes(rgb, *P.SUB, 10, False)
    m, site, _ = colour16(P010)
    assert np.array_equal(tap_y210([codes], box, s, m, site, P.V210, high_bits=2), tap16([shl6(codes)], box, s, m, site, subs=[P.SUB]))


SHAPES7 = [(37, 53), (64, 64), (20, 24), (98, 132), (270, 480), (1, 1), (33, 2)]
BOXES7 = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]


def test_mixed_batch_of_sizes_layouts_and_boxes():
    m, site = vithip.yuv_matrix(vithip.YUV_BT601, True), N.CHROMA_CENTER
    planes = [make_yuv(h, w, P.SUB, seed=40 + i) for i, (h, w) in enumerate(SHAPES7)]
    lays = [i % 4 for i in range(7)]
    got = tap_yuy2(planes, BOXES7, 32, m, site, lays, lead=1, gap=3, pad=1)
    assert np.array_equal(got, tap_yuv(planes, BOXES7, 32, m, site, subs=[P.SUB] * 7))
    for i in range(7):                                                 # each frame alone gives the same bytes as in the batch
        assert np.array_equal(tap_yuy2([planes[i]], [BOXES7[i]], 32, m, site, lays[i])[0], got[i])
    # Y210 words and v210 blocks in one batch: the layout is the frame's, the kernel the batch's
    m, site, _ = colour16(P010)
    lays = [P.YUYV, P.V210, P.YVYU, P.V210, P.V210, P.UYVY, P.V210]
    codes = [make_yuv16(h, w, P.SUB, 40 + i, CODES10) for i, (h, w) in enumerate(SHAPES7)]
    planes = [c if lay == P.V210 else shl6(c) for c, lay in zip(codes, lays)]
    got = tap_y210(planes, BOXES7, 32, m, site, lays, lead=4, gap=4)
    assert np.array_equal(got, tap16([shl6(c) for c in codes], BOXES7, 32, m, site, subs=[P.SUB] * 7))
    for i in range(7):
        assert np.array_equal(tap_y210([planes[i]], [BOXES7[i]], 32, m, site, lays[i])[0], got[i])


def test_large_batch_of_small_frames_runs_tall_bands():
    boxes = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    m, site = vithip.yuv_matrix(), N.CHROMA_LEFT
    planes = [make_yuv(41, 39, P.SUB, seed=100 + i) for i in range(40)]
    got = tap_yuy2(planes, boxes, 32, m, site, [i % 4 for i in range(40)])
    assert np.array_equal(got, tap_yuv(planes, boxes, 32, m, site, subs=[P.SUB] * 40))
    for i in (0, 5, 18, 39):
        assert np.array_equal(got[i], Y.resize_yuv_f32(*planes[i], boxes[i], 32, m, site, P.SUB))
    m, site, _ = colour16(P010)
    codes = [make_yuv16(41, 39, P.SUB, 100 + i, CODES10) for i in range(40)]
    lays = [P.V210 if i % 3 else P.UYVY for i in range(40)]
    got = tap_y210([c if lay == P.V210 else shl6(c) for c, lay in zip(codes, lays)], boxes, 32, m, site, lays)
    assert np.array_equal(got, tap16([shl6(c) for c in codes], boxes, 32, m, site, subs=[P.SUB] * 40))


# ---- 5. the forward -------------------------------------------------------------------------------------------------------------
def yuy2_set(s):
    """Three 8-bit packed frames: an even one with a centre crop, an odd one, a small one with a fractional box; three layouts."""
    shapes = [(s + 16, s + 36), (s + 1, s + 3), (s // 2 + 6, s // 2 + 23)]
    planes = [make_yuv(h, w, P.SUB, seed=1 + i) for i, (h, w) in enumerate(shapes)]
    return planes, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)], [P.YUYV, P.UYVY, P.YVYU]


def y210_set(s):
    """The same shapes as a Y210 frame, a v210 frame and a Y216-style VYUY frame."""
    shapes = [(s + 16, s + 36), (s + 1, s + 3), (s // 2 + 6, s // 2 + 23)]
    codes = [make_yuv16(h, w, P.SUB, 11 + i, CODES10) for i, (h, w) in enumerate(shapes)]
    lays = [P.YUYV, P.V210, P.VYUY]
    planes = [c if lay == P.V210 else shl6(c) for c, lay in zip(codes, lays)]
    return planes, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)], lays


FORWARD_CASES = [("vit_micro", S.CONFIGS["vit_micro"], vithip.DTYPE_BF16), ("patch14_micro", PATCH14_MICRO, vithip.DTYPE_BF16),
                 ("vit_micro", S.CONFIGS["vit_micro"], vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_every_packed_entry_point_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    m8, site8 = ctx.get_frame_colour()
    m16, site16 = ctx.get_frame_colour16()
    p8, b8, l8 = yuy2_set(s)
    p16, b16, l16 = y210_set(s)
    want8 = ctx.forward_u8(tap_yuy2(p8, b8, s, m8, site8, l8))
    want16 = ctx.forward_u8(tap_y210(p16, b16, s, m16, site16, l16))
    assert np.isfinite(want8).all() and np.isfinite(want16).all() and not np.array_equal(want8, want16)
    assert same_bits(ctx.forward_frames_yuy2(p8, l8, b8), want8)
    assert same_bits(ctx.forward_frames_y210(p16, l16, b16), want16)
    buf8, desc8 = P.lay_out(p8, b8, l8, lead=3, pad=1, gap=2)
    assert same_bits(ctx.forward_frames_yuy2_packed(buf8, desc8), want8)
    assert same_bits(device_logits(ctx.forward_device_frames_yuy2, buf8, desc8, cfg["classes"]), want8)
    buf16, desc16 = P.lay_out(p16, b16, l16, lead=4, pad=4, gap=4, high_bits=3)
    assert same_bits(ctx.forward_frames_y210_packed(buf16, desc16), want16)
    assert same_bits(device_logits(ctx.forward_device_frames_y210, buf16, desc16, cfg["classes"]), want16)
    ctx.ring_create_frames(2, 3, max(buf8.nbytes, buf16.nbytes))
    try:
        ctx.ring_submit_frames_yuy2(p8, l8, b8)
        ctx.ring_submit_frames_y210_packed(buf16, buf16.nbytes, desc16)
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
    set8, set16 = yuy2_set(s), y210_set(s)
    m8, site8 = ctx.get_frame_colour()
    m16, site16 = ctx.get_frame_colour16()
    ref8 = ctx.forward_u8(tap_yuy2(set8[0], set8[1], s, m8, site8, set8[2]))       # computed once; the tests below only read them
    ref16 = ctx.forward_u8(tap_y210(set16[0], set16[1], s, m16, site16, set16[2]))
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
            ctx.forward_device_frames_yuy2(din8.ptr, buf8.nbytes, desc8, dout.ptr)
            assert same_bits(logits(), ref8)
        assert ctx.get_graph()[0] and ctx.get_graph()[1] >= 1
        # other frames, of the other depth, through the replayed graph: the resize in front of it is no part of the capture
        ctx.forward_device_frames_y210(din16.ptr, buf16.nbytes, desc16, dout.ptr)
        assert same_bits(logits(), ref16)
        assert same_bits(ctx.forward_frames_yuy2(p8[::-1], l8[::-1], b8[::-1]), ref8[::-1])
        assert same_bits(ctx.forward_frames_y210(p16, l16, b16), ref16)
    finally:
        ctx.set_graph(False)
        ctx.set_streams(1)
        din8.free(); din16.free(); dout.free()


# ---- 6. state and ring ----------------------------------------------------------------------------------------------------------
def test_stage_timing_reports_one_resize_launch(micro):
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    try:
        ctx.set_stage_timing("resize")
        for call, args, want in ((ctx.forward_frames_yuy2, (p8, l8, b8), ref8), (ctx.forward_frames_y210, (p16, l16, b16), ref16)):
            assert same_bits(call(*args), want)
            avg, mn, n = ctx.get_stage_timing()
            assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_the_two_colour_states_stay_independent(micro):
    """An 8-bit packed submit follows vh_set_frame_colour, a 16-bit one vh_set_frame_colour16, and neither the other's."""
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    s = cfg["image_size"]
    try:
        m16 = vithip.yuv_matrix16(vithip.YUV_BT2020, True, 10, True)
        ctx.set_frame_colour16(m16, vithip.CHROMA_CENTER)
        moved16 = ctx.forward_frames_y210(p16, l16, b16)
        assert same_bits(moved16, ctx.forward_u8(tap_y210(p16, b16, s, m16, vithip.CHROMA_CENTER, l16))) and not np.array_equal(moved16, ref16)
        assert same_bits(ctx.forward_frames_yuy2(p8, l8, b8), ref8)
        mj = vithip.yuv_matrix(vithip.YUV_BT601, True)
        ctx.set_frame_colour(mj, vithip.CHROMA_CENTER)
        moved8 = ctx.forward_frames_yuy2(p8, l8, b8)
        assert same_bits(moved8, ctx.forward_u8(tap_yuy2(p8, b8, s, mj, vithip.CHROMA_CENTER, l8))) and not np.array_equal(moved8, ref8)
        assert same_bits(ctx.forward_frames_y210(p16, l16, b16), moved16)
        ctx.ring_create_frames(2, 3, 1 << 17)
        try:                                                            # the ring's submits follow the same two states
            ctx.ring_submit_frames_yuy2(p8, l8, b8)
            ctx.ring_submit_frames_y210(p16, l16, b16)
            assert same_bits(ctx.ring_collect(), moved8) and same_bits(ctx.ring_collect(), moved16)
        finally:
            vithip.lib().vh_ring_destroy(ctx.h)
        ctx.set_frame_colour16(None)
        assert same_bits(ctx.forward_frames_y210(p16, l16, b16), ref16) and same_bits(ctx.forward_frames_yuy2(p8, l8, b8), moved8)
    finally:
        ctx.set_frame_colour(None)
        ctx.set_frame_colour16(None)
    assert same_bits(ctx.forward_frames_yuy2(p8, l8, b8), ref8)


def test_frames_ring_takes_nv12_yuy2_p016_y210_v210_and_rgb_alternately(micro):
    ctx, cfg, (p8, b8, l8), ref8, (p16, b16, l16), ref16 = micro
    s = cfg["image_size"]
    nv12 = [make_nv12(s + 4, s + 10, seed=12)]
    ref_nv12 = ctx.forward_frames_nv12(nv12)
    pairs, pboxes = p010_set(s)
    ref_p016 = ctx.forward_frames_p016(pairs, pboxes)
    rgb = [make_frame(s + 7, s + 2, 3, seed=5), make_frame(s, s + 9, 3, seed=6)]
    ref_rgb = ctx.forward_frames(rgb)
    # the Y210 frames and the v210 frame of the 16-bit set as two submits
    y210 = ([p16[0], p16[2]], [l16[0], l16[2]], [b16[0], b16[2]])
    v210 = ([p16[1]], [l16[1]], [b16[1]])
    assert l16[1] == P.V210
    ctx.ring_create_frames(6, 3, 1 << 17)
    try:
        ctx.ring_submit_frames_nv12(nv12)
        ctx.ring_submit_frames_yuy2(p8, l8, b8)
        ctx.ring_submit_frames_p016(pairs, pboxes)
        ctx.ring_submit_frames_y210(*y210)
        # slot 5: v210 blocks filled in place
        buf, desc = P.lay_out(v210[0], v210[2], v210[1], lead=4, high_bits=3)
        ctx.ring_input_frames()[:buf.size] = buf
        ctx.ring_submit_frames_y210_packed(None, buf.size, desc)
        ctx.ring_submit_frames(rgb)
        assert ctx.ring_free_slots() == 0
        assert same_bits(ctx.ring_collect(), ref_nv12)                             # FIFO
        ctx.ring_submit_frames_yuy2(p8[::-1], l8[::-1], b8[::-1])
        assert same_bits(ctx.ring_collect(), ref8)
        assert same_bits(ctx.ring_collect(), ref_p016)
        assert same_bits(ctx.ring_collect(), ref16[[0, 2]])
        assert same_bits(ctx.ring_collect(), ref16[[1]])
        assert same_bits(ctx.ring_collect(), ref_rgb)
        assert same_bits(ctx.ring_collect(), ref8[::-1])
        assert ctx.ring_free_slots() == 6
        # a refused submit leaves the ring as it was and enqueues nothing
        buf, desc = P.lay_out(p8[:1], b8[:1], l8[:1])
        desc[0].row_stride -= 1
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_yuy2_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "row_stride <" in str(e.value) and ctx.ring_free_slots() == 6
        desc[0].row_stride += 1
        desc[0].layout = P.V210
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_yuy2_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "VH_422_V210" in str(e.value) and ctx.ring_free_slots() == 6
        buf, desc = P.lay_out(v210[0], v210[2], v210[1])
        desc[0].offset += 2
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_y210_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "multiple of 4" in str(e.value) and ctx.ring_free_slots() == 6
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_collect()
        assert e.value.code == 7                                                   # VH_ERR_RING_EMPTY: nothing was enqueued
        ctx.ring_submit_frames_y210(*v210)
        assert same_bits(ctx.ring_collect(), ref16[[1]])
        # packed submits on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            for call, args in ((ctx.ring_submit_frames_yuy2, (p8[:1], l8[:1], b8[:1])), (ctx.ring_submit_frames_y210, v210)):
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
        return L.vh_forward_frames_yuy2(ctx.h, buf8.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    def call16(n=3, nbytes=buf16.nbytes, d=desc16):
        return L.vh_forward_frames_y210(ctx.h, buf16.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    err = lambda: L.vh_last_error(ctx.h).decode()
    assert call8(n=4) == VH_ERR_INVALID and call16(n=4) == VH_ERR_INVALID          # batch > max_batch
    assert call8(nbytes=buf8.nbytes - 1) == VH_ERR_INVALID and "ends beyond nbytes" in err()
    assert call16(nbytes=buf16.nbytes - 1) == VH_ERR_INVALID and "ends beyond nbytes" in err()
    assert call8(d=None) == VH_ERR_INVALID and call16(d=None) == VH_ERR_INVALID
    desc8[1].layout = 4
    assert call8() == VH_ERR_INVALID and "VH_422_V210" in err()
    desc8[1].layout = 9
    assert call8() == VH_ERR_INVALID and "layout must be" in err()
    desc8[1].layout = l8[1]
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
            ctx.forward_device_frames_y210(dev.ptr + 1, buf16.nbytes, desc16, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "frames pointer is odd" in str(e.value)
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_frames_y210(dev.ptr + 2, buf16.nbytes, desc16, dout.ptr)     # the batch holds a v210 frame
        assert e.value.code == VH_ERR_INVALID and "frames pointer is no multiple of 4" in str(e.value)
        assert not dout.to_numpy(np.float32, (3, cfg["classes"])).any()
        ctx.forward_device_frames_y210(dev.ptr + 4, buf16.nbytes, desc16, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref16)
    finally:
        dev.free(); dout.free()
    assert same_bits(ctx.forward_frames_yuy2(p8, l8, b8), ref8)
    # a context with one channel is refused, and goes on working
    c1 = vithip.VitContext(dict(cfg, channels=1), dtype=vithip.DTYPE_BF16, max_batch=3)
    c1.init_weights_seeded(5)
    grey = [make_frame(cfg["image_size"], cfg["image_size"], 1, seed=4)]
    before = c1.forward_frames(grey)
    for callc, args in ((c1.forward_frames_yuy2, (p8, l8, b8)), (c1.forward_frames_y210, (p16, l16, b16))):
        with pytest.raises(vithip.VhError) as e:
            callc(*args)
        assert e.value.code == VH_ERR_INVALID and "3 channels" in str(e.value)
    assert same_bits(c1.forward_frames(grey), before)
    c1.close()
