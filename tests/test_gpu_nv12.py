"""GPU suite of the NV12 entry points (include/vithip.h, "NV12 frames").

1. The operator tap vh_op_resize_nv12 tied EXACTLY to the merged kernel: with the pass-through matrix, channel 0 is vh_op_resize_u8 of
   the Y plane as a 1-channel frame, channels 1 and 2 are vh_op_resize_u8 of the UV plane as a 2-channel frame with the chroma box.
2. The tap against nv12_ref, the numpy float64 statement, with real matrices: every byte within 0.5 + margin of the (clamped)
   unrounded float64 value and at least 99.5 % of the bytes equal to rint(v64); margin = max(1e-3, 3.3 (taps_y + taps_c + 4) 255 2^-24),
   the fp32 accumulation bound of test_gpu_frames.check_against_statement scaled by the matrix's largest absolute row sum.
3. The forward: the logits of every NV12 entry point EQUAL those of forward_u8 given the tap's own output."""
import ctypes as C

import numpy as np
import pytest

import nv12_ref as N
import vh_synth as S
import vithip
from test_gpu_frames import GUARD, PATCH14_MICRO, DTNAME, make_frame, same_bits
from test_gpu_frames import tap as tap_rgb
from test_nv12 import make_nv12

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE = 1, 3
PASS_THROUGH = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
COLOURS = {"bt709_limited_left": (N.BT709, False, N.CHROMA_LEFT), "bt601_full_centre": (N.BT601, True, N.CHROMA_CENTER)}


def lay_out(planes, boxes, y_pad=0, uv_pad=0, lead=0, gap=0, uv_first=False):
    """Planes into one buffer: `lead` bytes in front, `gap` bytes between any two planes, rows padded by y_pad / uv_pad bytes;
    uv_first puts each frame's UV plane in front of its Y plane (the planes need not be adjacent or ordered)."""
    desc = (vithip.FrameNV12 * len(planes))()
    chunks, off = [np.full(lead, 0xEE, np.uint8)], lead
    for i, ((y, uv), box) in enumerate(zip(planes, boxes)):
        h, w = y.shape
        parts = {}
        for key, a, rows, pad in (("y", y, h, y_pad), ("uv", uv.reshape(h // 2, w), h // 2, uv_pad)):
            stride = w + pad
            buf = np.full((rows, stride), 0xEE, np.uint8)
            buf[:, :w] = a
            parts[key] = (buf.reshape(-1)[:(rows - 1) * stride + w], stride)       # the last row carries no padding
        for key in (("uv", "y") if uv_first else ("y", "uv")):
            flat, stride = parts[key]
            if key == "y":
                desc[i].y_offset, desc[i].y_stride = off, stride
            else:
                desc[i].uv_offset, desc[i].uv_stride = off, stride
            chunks += [flat, np.full(gap, 0xEE, np.uint8)]
            off += flat.size + gap
        desc[i].height, desc[i].width = h, w
        desc[i].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return np.concatenate(chunks), desc


def tap(planes, boxes, s, m, site, **layout):
    """vh_op_resize_nv12 -> [n, s, s, 3] bytes; checks that nothing but the output was written."""
    buf, desc = lay_out(planes, boxes, **layout)
    n = len(planes) * s * s * 3
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.full(n + GUARD, 0xA5, np.uint8))
    try:
        vithip.op_resize_nv12(din.ptr, buf.nbytes, desc, s, m, site, dout.ptr)
        raw = dout.to_numpy(np.uint8, (n + GUARD,))
    finally:
        din.free(); dout.free()
    assert (raw[n:] == 0xA5).all()                                   # the guard bytes behind the output
    return raw[:n].reshape(len(planes), s, s, 3)


def check_against_statement(got, planes, boxes, s, m, site, label=""):
    for g, (y, uv), box in zip(got, planes, boxes):
        v64 = np.clip(N.resize_nv12_f64(y, uv, box, s, m, site), 0.0, 255.0)   # the contract clamps before it rounds
        taps_y, taps_c = N.max_taps(y, box, s, site)
        margin = N.margin(taps_y, taps_c)
        err = float(np.abs(g.astype(np.float64) - v64).max())
        same = float((g == np.rint(v64).astype(np.uint8)).mean())
        print(f"nv12 {y.shape[0]}x{y.shape[1]} box {box} -> {s} {label}: max |got - v64| = {err:.6f} (bound {0.5 + margin:.6f}), {100 * same:.3f} % equal rint(v64)")
        assert err <= 0.5 + margin
        assert same >= 0.995


# (h, w, box, S): the smallest shapes that reach each path.  The boxes keep box / 2 + 0.25 inside the chroma plane, so the
# left-sited chroma table is one the merged kernel's table accepts too.
OP_CASES = {
    "down_38x54_16": (38, 54, (0.0, 0.0, 53.0, 38.0), 16),                        # non-integer down-scale; 16 x 16: one row per band
    "up_20x24_32": (20, 24, (0.0, 0.0, 23.5, 20.0), 32),                          # up-scale: two taps, one chroma row feeds four rows
    "fractional_box_98x132_28": (98, 132, (10.25, 5.5, 101.75, 95.125), 28),      # fractional box, S * 3 = 84: no aligned row of bytes
    "taps29_270x480_32": (270, 480, (0.0, 0.0, 479.0, 270.0), 32),               # 29 luma taps, 15 chroma taps
}


@pytest.mark.parametrize("site", [N.CHROMA_CENTER, N.CHROMA_LEFT], ids=["centre", "left"])
@pytest.mark.parametrize("name", list(OP_CASES))
def test_pass_through_matrix_equals_the_merged_kernel_per_plane(name, site):
    h, w, box, s = OP_CASES[name]
    y, uv = make_nv12(h, w, seed=h + w)
    got = tap([(y, uv)], [box], s, PASS_THROUGH, site)[0]
    x0, y0, x1, y1 = box
    dx = 0.25 if site == N.CHROMA_LEFT else 0.0
    cbox = (x0 / 2 + dx, y0 / 2, x1 / 2 + dx, y1 / 2)                             # exact in float32 for these boxes
    assert all(float(np.float32(v)) == v for v in cbox) and cbox[2] <= w // 2
    want_y = tap_rgb([y[:, :, None]], [box], s)[0]
    want_c = tap_rgb([uv], [cbox], s)[0]
    assert np.array_equal(got[..., :1], want_y)
    assert np.array_equal(got[..., 1:], want_c)


@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_op_resize_nv12_matches_the_statement(name, colour):
    h, w, box, s = OP_CASES[name]
    std, full, site = COLOURS[colour]
    planes = [make_nv12(h, w, seed=h + w)]
    m = vithip.yuv_matrix(std, full)
    for bx in (box, None):                                                         # None: the whole frame; left siting overhangs by 0.25
        check_against_statement(tap(planes, [bx], s, m, site), planes, [bx], s, m, site, colour)


def test_padded_strides_odd_offsets_and_planes_apart():
    planes = [make_nv12(38, 54, seed=21), make_nv12(42, 30, seed=31)]
    boxes = [None, (0.5, 3.0, 29.5, 40.0)]
    m = vithip.yuv_matrix()
    want = tap(planes, boxes, 16, m, N.CHROMA_LEFT)                                # even offsets and strides: 16-bit UV loads
    check_against_statement(want, planes, boxes, 16, m, N.CHROMA_LEFT)
    layouts = [dict(y_pad=6, uv_pad=10),                       # padded rows, still even: 16-bit UV loads
               dict(y_pad=5, uv_pad=0, lead=2),                # odd y_stride shifts the UV plane to an odd offset: byte loads
               dict(uv_pad=3),                                 # odd uv_stride: byte loads
               dict(lead=3, gap=7),                            # odd y_offset and even uv_offset, planes 7 bytes apart
               dict(lead=1, gap=2, y_pad=5, uv_pad=7),         # everything odd
               dict(gap=64, uv_first=True)]                    # UV in front of Y, planes not adjacent
    for lay in layouts:
        assert np.array_equal(tap(planes, boxes, 16, m, N.CHROMA_LEFT, **lay), want), lay


def test_one_1080p_frame_spans_many_bands():
    """224 output rows from 1080: the band cap of a one-frame call (S / 64 = 3 rows) gives 75 bands."""
    planes = [make_nv12(1080, 1920, seed=3)]
    box = vithip.center_crop_box(1080, 1920)
    m = vithip.yuv_matrix()
    check_against_statement(tap(planes, [box], 224, m, N.CHROMA_LEFT), planes, [box], 224, m, N.CHROMA_LEFT)


def test_large_batch_of_small_frames_runs_tall_bands():
    """With 40 frames in a call the cap is S / 2 = 16 rows, and 16 output rows of a 40 x 40 frame fit the LDS: tall bands."""
    planes = [make_nv12(40, 40, seed=100 + i) for i in range(40)]
    boxes = [None if i % 2 else (0.5, 1.0, 39.25, 38.0) for i in range(40)]
    m = vithip.yuv_matrix(vithip.YUV_BT601, True)
    got = tap(planes, boxes, 32, m, N.CHROMA_CENTER)
    check_against_statement(got[::9], planes[::9], boxes[::9], 32, m, N.CHROMA_CENTER)
    for i in (0, 7, 39):
        assert np.array_equal(tap([planes[i]], [boxes[i]], 32, m, N.CHROMA_CENTER)[0], got[i])


def test_mixed_batch_of_five_frames():
    shapes = [(38, 54), (64, 64), (20, 24), (98, 132), (270, 480)]
    planes = [make_nv12(h, w, seed=40 + i) for i, (h, w) in enumerate(shapes)]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480)]
    m = vithip.yuv_matrix()
    got = tap(planes, boxes, 32, m, N.CHROMA_LEFT, lead=1, gap=3)
    check_against_statement(got, planes, boxes, 32, m, N.CHROMA_LEFT)
    for i in range(5):                                                 # each frame alone gives the same bytes as in the batch
        assert np.array_equal(tap([planes[i]], [boxes[i]], 32, m, N.CHROMA_LEFT)[0], got[i])


@pytest.mark.parametrize("h", [4062, 4064])
def test_scale32_narrows_the_column_tiles(h):
    """S = 130 leaves 16384 / 130 = 126 floats per output column.  One output row of a 4062-row frame needs 64 luma rows and 31
    chroma rows, 64 + 2 x 31 = 126: full-width bands of one row.  4064 rows is the smallest even height whose worst row needs 127
    (65 + 2 x 31): the planner narrows the tile to 16384 / 127 = 129 columns, two column tiles per row, the second one column wide."""
    s = 130
    yc = N.axis_table(h, 0.0, float(h), s)[1]
    cc = N.axis_table(h // 2, 0.0, h / 2.0, s)[1]
    assert (int((yc + 2 * cc).max()) > 16384 // s) == (h == 4064)          # the planner's own criterion, from the statement's tables
    planes = [make_nv12(h, 36, seed=7)]
    m = vithip.yuv_matrix()
    check_against_statement(tap(planes, [None], s, m, N.CHROMA_LEFT), planes, [None], s, m, N.CHROMA_LEFT)


# ---- the forward ---------------------------------------------------------------------------------------------------------------
def forward_set(s):
    """Three NV12 frames of different sizes and boxes for a model of input size s."""
    planes = [make_nv12(s + 16, s + 36, seed=1), make_nv12(s, s, seed=2), make_nv12(s // 2 + 6, s // 2 + 22, seed=3)]
    boxes = [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)]
    return planes, boxes


FORWARD_CASES = [(n, c, d) for n, c in (("vit_micro", S.CONFIGS["vit_micro"]), ("patch14_micro", PATCH14_MICRO))
                 for d in (vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_forward_frames_nv12_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    planes, boxes = forward_set(s)
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    m, site = ctx.get_frame_colour()                       # the default: BT.709 limited range, left siting
    assert np.array_equal(m, vithip.yuv_matrix(vithip.YUV_BT709, False)) and site == vithip.CHROMA_LEFT
    resized = tap(planes, boxes, s, m, site)
    want = ctx.forward_u8(resized)
    got = ctx.forward_frames_nv12(planes, boxes)
    assert np.isfinite(want).all() and np.array_equal(got, want) and same_bits(got, want)
    # a second, different colour matrix: different, finite logits, again those of the tap
    m2 = vithip.yuv_matrix(vithip.YUV_BT601, True)
    ctx.set_frame_colour(m2, vithip.CHROMA_CENTER)
    m2b, site2 = ctx.get_frame_colour()
    assert np.array_equal(m2b, m2) and site2 == vithip.CHROMA_CENTER
    want2 = ctx.forward_u8(tap(planes, boxes, s, m2, vithip.CHROMA_CENTER))
    got2 = ctx.forward_frames_nv12(planes, boxes)
    assert np.isfinite(got2).all() and same_bits(got2, want2) and not np.array_equal(got2, got)
    ctx.set_frame_colour(None)                             # back to the default
    assert same_bits(ctx.forward_frames_nv12(planes, boxes), want)
    ctx.close()


@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
    ctx.init_weights_seeded(17)
    planes, boxes = forward_set(s)
    m, site = ctx.get_frame_colour()
    ref = ctx.forward_u8(tap(planes, boxes, s, m, site))   # computed once; the tests below only read it
    ref.setflags(write=False)
    yield ctx, cfg, planes, boxes, ref
    ctx.close()


def test_device_entry_point_streams_and_graphs(micro):
    ctx, cfg, planes, boxes, ref = micro
    buf, desc = lay_out(planes, boxes, y_pad=5, uv_pad=3, lead=3, gap=1)          # unaligned device planes
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    ctx.forward_device_frames_nv12(din.ptr, buf.nbytes, desc, dout.ptr)
    assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
    try:
        ctx.set_streams(2)                                                         # the resize runs once, before the fork
        ctx.set_graph(True)
        for _ in range(3):                                                         # eager, captured, replayed
            assert same_bits(ctx.forward_frames_nv12(planes, boxes), ref)
        assert ctx.get_graph()[0] and ctx.get_graph()[1] >= 1
        ctx.forward_device_frames_nv12(din.ptr, buf.nbytes, desc, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
        # other frames through the replayed graph: the resize in front of it is no part of the capture
        assert same_bits(ctx.forward_frames_nv12(planes[::-1], boxes[::-1]), ref[::-1])
    finally:
        ctx.set_graph(False)
        ctx.set_streams(1)
    din.free(); dout.free()


def test_stage_timing_times_the_nv12_resize(micro):
    ctx, cfg, planes, boxes, ref = micro
    try:
        ctx.set_stage_timing("resize")
        assert same_bits(ctx.forward_frames_nv12(planes, boxes), ref)
        avg, mn, n = ctx.get_stage_timing()
        assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_frames_ring_takes_rgb_and_nv12_alternately(micro):
    ctx, cfg, planes, boxes, ref = micro
    s = cfg["image_size"]
    rgb = [make_frame(s + 8, s + 20, 3, seed=9), make_frame(s, s, 3, seed=10)]
    ref_rgb = ctx.forward_frames(rgb)
    ctx.ring_create_frames(3, 3, 1 << 16)
    try:
        ctx.ring_submit_frames(rgb)
        ctx.ring_submit_frames_nv12(planes, boxes)
        # slot 2: NV12 planes filled in place
        buf, desc = lay_out(planes[1:], boxes[1:], lead=1)
        ctx.ring_input_frames()[:buf.size] = buf
        ctx.ring_submit_frames_nv12_packed(None, buf.size, desc)
        assert ctx.ring_free_slots() == 0
        assert same_bits(ctx.ring_collect(), ref_rgb)                              # FIFO
        ctx.ring_submit_frames(rgb[::-1])
        assert same_bits(ctx.ring_collect(), ref)
        assert same_bits(ctx.ring_collect(), ref[1:])
        assert same_bits(ctx.ring_collect(), ref_rgb[::-1])
        assert ctx.ring_free_slots() == 3
        # a refused NV12 submit (odd width) leaves the ring as it was
        buf, desc = lay_out(planes[:1], boxes[:1])
        desc[0].width -= 1
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_nv12_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and ctx.ring_free_slots() == 3
        ctx.ring_submit_frames_nv12(planes, boxes)
        assert same_bits(ctx.ring_collect(), ref)
        # an NV12 submit on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_submit_frames_nv12(planes[:1], boxes[:1])
            assert e.value.code == VH_ERR_STATE and ctx.ring_free_slots() == 2
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


def test_refusals_enqueue_nothing(micro):
    ctx, cfg, planes, boxes, ref = micro
    L = vithip.lib()
    buf, desc = lay_out(planes, boxes)
    out = np.zeros((3, cfg["classes"]), np.float32)

    def call(n=3, nbytes=buf.nbytes, d=desc):
        return L.vh_forward_frames_nv12(ctx.h, buf.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    assert call(n=4) == VH_ERR_INVALID                                             # batch > max_batch
    assert same_bits(ctx.forward_frames_nv12(planes, boxes), ref)
    assert call(nbytes=buf.nbytes - 1) == VH_ERR_INVALID                           # the last UV byte beyond nbytes
    assert call(d=None) == VH_ERR_INVALID
    desc[1].height += 1                                                            # odd height
    assert call() == VH_ERR_INVALID
    desc[1].height -= 1
    desc[2].box[2] = desc[2].width + 0.5
    assert call() == VH_ERR_INVALID
    assert not out.any()                                                           # nothing ran
    assert same_bits(ctx.forward_frames_nv12(planes, boxes), ref)
    # a context with one channel is refused, and goes on working
    cfg1 = dict(cfg, channels=1)
    c1 = vithip.VitContext(cfg1, dtype=vithip.DTYPE_BF16, max_batch=3)
    c1.init_weights_seeded(5)
    grey = [make_frame(cfg["image_size"], cfg["image_size"], 1, seed=4)]
    before = c1.forward_frames(grey)
    with pytest.raises(vithip.VhError) as e:
        c1.forward_frames_nv12(planes, boxes)
    assert e.value.code == VH_ERR_INVALID
    assert same_bits(c1.forward_frames(grey), before)
    c1.close()
