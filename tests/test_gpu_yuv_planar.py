"""GPU suite of the planar YUV entry points (include/vithip.h, "Planar YUV frames").

1. EXACT ties (np.array_equal) of the operator tap vh_op_resize_yuv to the merged kernels: I420 of even size to vh_op_resize_nv12 of the
   interleaved planes (and YV12 to both); with the pass-through matrix, channel k to vh_op_resize_u8 of plane k as a 1-channel frame
   with that plane's box, at all four sub-samplings and odd sizes; 4:4:4 to vh_op_resize_u8 of the three planes interleaved; every
   layout to the packed one; every frame of a batch to the frame alone.
2. The tap against yuv_ref, the numpy float64 statement, with real matrices: every byte within 0.5 + nv12_ref.margin(taps_y, taps_c)
   of the clamped unrounded float64 value, and at least 99.5 % of the bytes equal to rint of it.
3. The forward: the logits of every planar entry point EQUAL those of forward_u8 given the tap's own output."""
import ctypes as C
import functools

import numpy as np
import pytest

import nv12_ref as N
import vh_synth as S
import vithip
import yuv_ref as Y
from test_gpu_frames import GUARD, PATCH14_MICRO, DTNAME, make_frame, same_bits
from test_gpu_frames import tap as tap_rgb
from test_gpu_nv12 import tap as tap_nv12
from test_nv12 import make_nv12
from test_yuv_planar import COLOURS, OP_CASES, SUBS, make_yuv, statement_figures

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE = 1, 3
PASS_THROUGH = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
MATRICES = {"bt709_limited": (N.BT709, False), "bt601_full": (N.BT601, True)}


def lay_out(planes, boxes, subs=None, pads=(0, 0, 0), lead=0, gap=0, order="yuv"):
    """Planes into one buffer: `lead` bytes in front, `gap` bytes behind every plane, rows of Y / U / V padded by pads[0..2]
    bytes, each frame's planes in `order` (any permutation of "yuv").  subs: one (sub_x, sub_y) per frame, None = from the shapes."""
    desc = (vithip.FrameYUV * len(planes))()
    chunks, off = [np.full(lead, 0xEE, np.uint8)], lead
    for i, (yuv, box) in enumerate(zip(planes, boxes)):
        h, w = yuv[0].shape
        d = desc[i]
        d.sub_x, d.sub_y = Y.subsampling(yuv[0].shape, yuv[1].shape) if subs is None else subs[i]
        for key in order:
            k = "yuv".index(key)
            rows, cols = yuv[k].shape
            stride = cols + pads[k]
            buf = np.full((rows, stride), 0xEE, np.uint8)
            buf[:, :cols] = yuv[k]
            flat = buf.reshape(-1)[:(rows - 1) * stride + cols]                    # the last row carries no padding
            setattr(d, key + "_offset", off)
            setattr(d, key + "_stride", stride)
            chunks += [flat, np.full(gap, 0xEE, np.uint8)]
            off += flat.size + gap
        d.height, d.width = h, w
        d.box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return np.concatenate(chunks), desc


def tap(planes, boxes, s, m, site, subs=None, **layout):
    """vh_op_resize_yuv -> [n, s, s, 3] bytes; checks that nothing but the output was written."""
    buf, desc = lay_out(planes, boxes, subs, **layout)
    n = len(planes) * s * s * 3
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.full(n + GUARD, 0xA5, np.uint8))
    try:
        vithip.op_resize_yuv(din.ptr, buf.nbytes, desc, s, m, site, dout.ptr)
        raw = dout.to_numpy(np.uint8, (n + GUARD,))
    finally:
        din.free(); dout.free()
    assert (raw[n:] == 0xA5).all()                                   # the guard bytes behind the output
    return raw[:n].reshape(len(planes), s, s, 3)


def check_against_statement(got, planes, boxes, s, m, site, subs=None, label=""):
    for i, (g, yuv, box) in enumerate(zip(got, planes, boxes)):
        sub = Y.subsampling(yuv[0].shape, yuv[1].shape) if subs is None else subs[i]
        err, bound, same = statement_figures(g, yuv, box, s, m, site, sub)
        print(f"yuv sub {sub} {yuv[0].shape[0]}x{yuv[0].shape[1]} box {box} -> {s} {label}: max |got - v64| = {err:.6f} (bound {bound:.6f}), {100 * same:.3f} % equal rint(v64)")
        assert err <= bound
        assert same >= 0.995


# ---- exact ties -----------------------------------------------------------------------------------------------------------------
EVEN_CASES = [n for n, c in OP_CASES.items() if c[0] % 2 == 0 and c[1] % 2 == 0]


@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("site", [N.CHROMA_CENTER, N.CHROMA_LEFT], ids=["centre", "left"])
@pytest.mark.parametrize("name", EVEN_CASES)
def test_i420_and_yv12_equal_nv12_of_the_interleaved_planes(name, site, matrix):
    h, w, box, s = OP_CASES[name]
    y, uv = make_nv12(h, w, seed=h + w)
    u, v = np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])
    m = vithip.yuv_matrix(*MATRICES[matrix])
    want = tap_nv12([(y, uv)], [box], s, m, site)
    got = tap([(y, u, v)], [box], s, m, site, subs=[(2, 2)])
    assert np.array_equal(got, want)
    # YV12 as a decoder writes it: Y, V, U in memory, the descriptor's u_offset and v_offset exchanged accordingly
    assert np.array_equal(tap([(y, u, v)], [box], s, m, site, subs=[(2, 2)], order="yvu"), want)
    # and the planes named the wrong way round with the matrix's chroma columns exchanged to match (the G row then adds its two
    # chroma terms in the other order: the same bytes on these inputs, as test_yuv_planar's emulation shows, not by construction)
    assert np.array_equal(tap([(y, v, u)], [box], s, m[:, [0, 2, 1, 3]], site, subs=[(2, 2)]), want)


# boxes for which the chroma box (lo / sub + delta, hi / sub + delta) is exact in float32 and inside the chroma plane at both sitings,
# so that the merged 1-channel kernel accepts it too
TIE_CASES = dict(OP_CASES, down_38x54_16=(38, 54, (0.0, 0.0, 53.0, 38.0), 16), up_20x24_32=(20, 24, (0.0, 0.0, 23.5, 20.0), 32),
                 taps29_270x480_32=(270, 480, (0.0, 0.0, 479.0, 270.0), 32), two_by_two_4=(2, 2, (0.0, 0.0, 1.5, 2.0), 4))


@pytest.mark.parametrize("site", [N.CHROMA_CENTER, N.CHROMA_LEFT], ids=["centre", "left"])
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(TIE_CASES))
def test_pass_through_matrix_equals_the_merged_kernel_per_plane(name, sub, site):
    h, w, box, s = TIE_CASES[name]
    sx, sy = SUBS[sub]
    y, u, v = make_yuv(h, w, (sx, sy), seed=h + w)
    got = tap([(y, u, v)], [box], s, PASS_THROUGH, site, subs=[(sx, sy)])[0]
    cbox = Y.chroma_box(N.box_of(y, box), sx, sy, site)
    assert all(float(np.float32(t)) == t for t in cbox) and cbox[2] <= u.shape[1] and cbox[3] <= u.shape[0]
    assert np.array_equal(got[..., 0:1], tap_rgb([y[:, :, None]], [box], s)[0])
    assert np.array_equal(got[..., 1:2], tap_rgb([u[:, :, None]], [cbox], s)[0])
    assert np.array_equal(got[..., 2:3], tap_rgb([v[:, :, None]], [cbox], s)[0])


@pytest.mark.parametrize("name", list(OP_CASES))
def test_444_equals_the_rgb_kernel_on_the_interleaved_planes(name):
    h, w, box, s = OP_CASES[name]
    y, u, v = make_yuv(h, w, (1, 1), seed=h + w)
    for site in (N.CHROMA_CENTER, N.CHROMA_LEFT):                                  # no sub-sampled axis: the siting changes nothing
        got = tap([(y, u, v)], [box], s, PASS_THROUGH, site, subs=[(1, 1)])
        assert np.array_equal(got, tap_rgb([np.stack([y, u, v], axis=-1)], [box], s))


def test_padded_strides_odd_offsets_any_order_and_planes_apart():
    planes = [make_yuv(37, 53, (2, 2), seed=21), make_yuv(42, 31, (2, 1), seed=31), make_yuv(29, 30, (1, 1), seed=41)]
    boxes = [None, (0.5, 3.0, 29.5, 40.0), None]
    m = vithip.yuv_matrix(vithip.YUV_BT601, True)
    want = tap(planes, boxes, 16, m, N.CHROMA_CENTER)                              # packed: Y, U, V back to back
    check_against_statement(want, planes, boxes, 16, m, N.CHROMA_CENTER)
    layouts = [dict(pads=(6, 10, 2)),                          # padded rows, a different padding per plane
               dict(pads=(5, 0, 0), lead=2),                   # odd y_stride
               dict(pads=(0, 3, 0)),                           # odd u_stride alone: U and V rows no longer in step
               dict(pads=(0, 0, 7)),
               dict(lead=3, gap=7),                            # odd offsets, planes 7 bytes apart
               dict(lead=1, gap=2, pads=(5, 7, 3)),            # everything odd
               dict(order="yvu"),                              # YV12
               dict(gap=64, order="uvy"),                      # chroma in front of luma, planes not adjacent
               dict(lead=5, gap=1, order="vyu", pads=(1, 0, 2))]
    for lay in layouts:
        assert np.array_equal(tap(planes, boxes, 16, m, N.CHROMA_CENTER, **lay), want), lay


def test_mixed_batch_of_sizes_and_subsamplings():
    shapes = [(37, 53, "420"), (64, 64, "444"), (20, 24, "422"), (98, 132, "440"), (270, 480, "420"), (1, 1, "420"), (33, 2, "422")]
    planes = [make_yuv(h, w, SUBS[k], seed=40 + i) for i, (h, w, k) in enumerate(shapes)]
    subs = [SUBS[k] for _, _, k in shapes]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
    m = vithip.yuv_matrix()
    got = tap(planes, boxes, 32, m, N.CHROMA_LEFT, subs, lead=1, gap=3)
    check_against_statement(got, planes, boxes, 32, m, N.CHROMA_LEFT, subs)
    for i in range(len(planes)):                                       # each frame alone gives the same bytes as in the batch
        assert np.array_equal(tap([planes[i]], [boxes[i]], 32, m, N.CHROMA_LEFT, [subs[i]])[0], got[i])


def test_large_batch_of_small_frames_runs_tall_bands():
    """With 40 frames in a call the cap is S / 2 = 16 rows, and 16 output rows of a 41 x 39 frame fit the LDS: tall bands, at every
    sub-sampling in one call."""
    keys = list(SUBS)
    subs = [SUBS[keys[i % 4]] for i in range(40)]
    planes = [make_yuv(41, 39, subs[i], seed=100 + i) for i in range(40)]
    boxes = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    m = vithip.yuv_matrix(vithip.YUV_BT601, True)
    got = tap(planes, boxes, 32, m, N.CHROMA_CENTER, subs)
    check_against_statement(got[::9], planes[::9], boxes[::9], 32, m, N.CHROMA_CENTER, subs[::9])
    for i in (0, 5, 18, 39):
        assert np.array_equal(tap([planes[i]], [boxes[i]], 32, m, N.CHROMA_CENTER, [subs[i]])[0], got[i])


# ---- the statement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_op_resize_yuv_matches_the_statement(name, sub, colour):
    h, w, box, s = OP_CASES[name]
    std, full, site = COLOURS[colour]
    planes = [make_yuv(h, w, SUBS[sub], seed=h + w)]
    m = vithip.yuv_matrix(std, full)
    check_against_statement(tap(planes, [box], s, m, site, [SUBS[sub]]), planes, [box], s, m, site, [SUBS[sub]], f"{sub} {colour}")


def test_one_1080p_i420_frame_spans_many_bands():
    """224 output rows from 1080: the band cap of a one-frame call (S / 64 = 3 rows) gives 75 bands."""
    y, uv = make_nv12(1080, 1920, seed=3)
    planes = [(y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]))]
    box = vithip.center_crop_box(1080, 1920)
    m = vithip.yuv_matrix()
    check_against_statement(tap(planes, [box], 224, m, N.CHROMA_LEFT), planes, [box], 224, m, N.CHROMA_LEFT)


# ---- the planner's boundary at 4:4:4 --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planner_boundary_444(s=130):
    """(largest height whose every output row fits 16384 // s floats per column at 4:4:4, smallest height with a row that does
    not), found with the library's own host table over every height the scale limit admits."""
    fit = 16384 // s
    narrows = [int(3 * vithip.resize_table(h, 0.0, float(h), s)[1].max()) > fit for h in range(s, 32 * s + 1)]
    heights = np.arange(s, 32 * s + 1)
    return int(heights[~np.array(narrows)].max()), int(heights[np.array(narrows)].min())


@pytest.mark.parametrize("which", ["largest_full_width", "smallest_narrowed"])
def test_444_narrows_the_column_tiles_at_the_planner_s_boundary(which):
    """S = 130 leaves 16384 // 130 = 126 floats per output column, and at 4:4:4 an output row with t vertical taps costs 3 t of them:
    42 taps fit (126), 43 do not (129 -> tile_cols = 16384 // 129 = 127, two column tiles per row).  The two heights are the last
    and the first on either side of that, by the statement's own tables."""
    s = 130
    h_full, h_narrow = planner_boundary_444(s)
    h = h_full if which == "largest_full_width" else h_narrow
    yc = N.axis_table(h, 0.0, float(h), s)[1]                                      # at 4:4:4 the chroma table is the luma table
    print(f"4:4:4 planner boundary at S = {s}: full width up to {h_full} rows, narrowed from {h_narrow}; {h} rows -> {int(yc.max())} taps")
    assert (int((yc + 2 * yc).max()) > 16384 // s) == (which == "smallest_narrowed")
    planes = [make_yuv(h, 36, (1, 1), seed=7)]
    m = vithip.yuv_matrix()
    check_against_statement(tap(planes, [None], s, m, N.CHROMA_LEFT, [(1, 1)]), planes, [None], s, m, N.CHROMA_LEFT, [(1, 1)])


# ---- the forward ----------------------------------------------------------------------------------------------------------------
def video_set(s):
    """Three frames as a video decoder emits them: an even I420 frame with a centre crop, an odd 4:2:2 one, a 4:4:0 one with a box."""
    shapes = [(s + 16, s + 36, "420"), (s + 1, s + 3, "422"), (s // 2 + 6, s // 2 + 23, "440")]
    planes = [make_yuv(h, w, SUBS[k], seed=1 + i) for i, (h, w, k) in enumerate(shapes)]
    boxes = [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)]
    return planes, boxes


def jpeg_set(s):
    """Three pictures as a JPEG decoder emits them: odd sizes, 4:4:4 and 4:2:0 mixed."""
    shapes = [(s + 11, s + 37, "444"), (s + 29, s + 5, "420"), (s - 3, s - 7, "420")]
    planes = [make_yuv(h, w, SUBS[k], seed=11 + i) for i, (h, w, k) in enumerate(shapes)]
    boxes = [vithip.center_crop_box(s + 11, s + 37), vithip.center_crop_box(s + 29, s + 5), None]
    return planes, boxes


FORWARD_CASES = [(n, c, d) for n, c in (("vit_micro", S.CONFIGS["vit_micro"]), ("patch14_micro", PATCH14_MICRO))
                 for d in (vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_forward_frames_yuv_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    planes, boxes = video_set(s)
    m, site = ctx.get_frame_colour()                       # the default, the video one: BT.709 limited range, left siting
    assert np.array_equal(m, vithip.yuv_matrix(vithip.YUV_BT709, False)) and site == vithip.CHROMA_LEFT
    want = ctx.forward_u8(tap(planes, boxes, s, m, site))
    got = ctx.forward_frames_yuv(planes, boxes)
    assert np.isfinite(want).all() and np.array_equal(got, want) and same_bits(got, want)
    # what a JPEG caller sets: full-range BT.601, centre siting; odd sizes, 4:4:4 and 4:2:0 in one batch
    jplanes, jboxes = jpeg_set(s)
    mj = vithip.yuv_matrix(vithip.YUV_BT601, True)
    ctx.set_frame_colour(mj, vithip.CHROMA_CENTER)
    wantj = ctx.forward_u8(tap(jplanes, jboxes, s, mj, vithip.CHROMA_CENTER))
    gotj = ctx.forward_frames_yuv(jplanes, jboxes)
    assert np.isfinite(gotj).all() and same_bits(gotj, wantj) and not np.array_equal(gotj, got)
    # the one colour state serves both layouts: the video frames under the JPEG colour are the tap's under that colour
    assert same_bits(ctx.forward_frames_yuv(planes, boxes), ctx.forward_u8(tap(planes, boxes, s, mj, vithip.CHROMA_CENTER)))
    ctx.set_frame_colour(None)                             # back to the default
    assert same_bits(ctx.forward_frames_yuv(planes, boxes), want)
    ctx.close()


@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
    ctx.init_weights_seeded(17)
    planes, boxes = video_set(s)
    m, site = ctx.get_frame_colour()
    ref = ctx.forward_u8(tap(planes, boxes, s, m, site))   # computed once; the tests below only read it
    ref.setflags(write=False)
    yield ctx, cfg, planes, boxes, ref
    ctx.close()


def test_device_entry_point_streams_and_graphs(micro):
    ctx, cfg, planes, boxes, ref = micro
    buf, desc = lay_out(planes, boxes, pads=(5, 3, 1), lead=3, gap=1, order="vyu")   # unaligned device planes
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    ctx.forward_device_frames_yuv(din.ptr, buf.nbytes, desc, dout.ptr)
    assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
    try:
        ctx.set_streams(2)                                                         # the resize runs once, before the fork
        ctx.set_graph(True)
        for _ in range(3):                                                         # eager, captured, replayed
            assert same_bits(ctx.forward_frames_yuv(planes, boxes), ref)
        assert ctx.get_graph()[0] and ctx.get_graph()[1] >= 1
        ctx.forward_device_frames_yuv(din.ptr, buf.nbytes, desc, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
        # other frames through the replayed graph: the resize in front of it is no part of the capture
        assert same_bits(ctx.forward_frames_yuv(planes[::-1], boxes[::-1]), ref[::-1])
    finally:
        ctx.set_graph(False)
        ctx.set_streams(1)
    din.free(); dout.free()


def test_stage_timing_times_the_planar_resize(micro):
    ctx, cfg, planes, boxes, ref = micro
    try:
        ctx.set_stage_timing("resize")
        assert same_bits(ctx.forward_frames_yuv(planes, boxes), ref)
        avg, mn, n = ctx.get_stage_timing()
        assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_frames_ring_takes_rgb_nv12_and_planar_alternately(micro):
    ctx, cfg, planes, boxes, ref = micro
    s = cfg["image_size"]
    rgb = [make_frame(s + 8, s + 20, 3, seed=9), make_frame(s, s, 3, seed=10)]
    ref_rgb = ctx.forward_frames(rgb)
    nv12 = [make_nv12(s + 4, s + 10, seed=12)]
    ref_nv12 = ctx.forward_frames_nv12(nv12)
    ctx.ring_create_frames(4, 3, 1 << 16)
    try:
        ctx.ring_submit_frames(rgb)
        ctx.ring_submit_frames_yuv(planes, boxes)
        ctx.ring_submit_frames_nv12(nv12)
        # slot 3: planes filled in place
        buf, desc = lay_out(planes[1:], boxes[1:], lead=1)
        ctx.ring_input_frames()[:buf.size] = buf
        ctx.ring_submit_frames_yuv_packed(None, buf.size, desc)
        assert ctx.ring_free_slots() == 0
        assert same_bits(ctx.ring_collect(), ref_rgb)                              # FIFO
        ctx.ring_submit_frames_yuv(planes[::-1], boxes[::-1])
        assert same_bits(ctx.ring_collect(), ref)
        assert same_bits(ctx.ring_collect(), ref_nv12)
        assert same_bits(ctx.ring_collect(), ref[1:])
        assert same_bits(ctx.ring_collect(), ref[::-1])
        assert ctx.ring_free_slots() == 4
        # a refused planar submit (sub_x = 3) leaves the ring as it was
        buf, desc = lay_out(planes[:1], boxes[:1])
        desc[0].sub_x = 3
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_yuv_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "sub_x" in str(e.value) and ctx.ring_free_slots() == 4
        ctx.ring_submit_frames_yuv(planes, boxes)
        assert same_bits(ctx.ring_collect(), ref)
        # a planar submit on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_submit_frames_yuv(planes[:1], boxes[:1])
            assert e.value.code == VH_ERR_STATE and ctx.ring_free_slots() == 2
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


def test_refusals_enqueue_nothing(micro):
    ctx, cfg, planes, boxes, ref = micro
    L = vithip.lib()
    buf, desc = lay_out(planes, boxes)
    out = np.zeros((3, cfg["classes"]), np.float32)

    def call(n=3, nbytes=buf.nbytes, d=desc):
        return L.vh_forward_frames_yuv(ctx.h, buf.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    assert call(n=4) == VH_ERR_INVALID                                             # batch > max_batch
    assert same_bits(ctx.forward_frames_yuv(planes, boxes), ref)
    assert call(nbytes=buf.nbytes - 1) == VH_ERR_INVALID                           # the last V byte beyond nbytes
    assert call(d=None) == VH_ERR_INVALID
    desc[1].sub_y = 0
    assert call() == VH_ERR_INVALID
    desc[1].sub_y = 1
    desc[0].u_stride = desc[0].width // 2 - 1
    assert call() == VH_ERR_INVALID
    desc[0].u_stride = desc[0].width // 2
    desc[2].box[2] = desc[2].width + 0.5
    assert call() == VH_ERR_INVALID
    assert not out.any()                                                           # nothing ran
    assert same_bits(ctx.forward_frames_yuv(planes, boxes), ref)
    # a context with one channel is refused, and goes on working
    cfg1 = dict(cfg, channels=1)
    c1 = vithip.VitContext(cfg1, dtype=vithip.DTYPE_BF16, max_batch=3)
    c1.init_weights_seeded(5)
    grey = [make_frame(cfg["image_size"], cfg["image_size"], 1, seed=4)]
    before = c1.forward_frames(grey)
    with pytest.raises(vithip.VhError) as e:
        c1.forward_frames_yuv(planes, boxes)
    assert e.value.code == VH_ERR_INVALID and "3 channels" in str(e.value)
    assert same_bits(c1.forward_frames(grey), before)
    c1.close()
