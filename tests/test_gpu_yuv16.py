"""GPU suite of the 16-bit YUV entry points (include/vithip.h, "16-bit YUV frames").

1. EXACT ties (np.array_equal) of the taps vh_op_resize_yuv16 / vh_op_resize_p016 to the 8-bit kernels: 8-bit codes stored as 16-bit
   words under the 8-bit matrix, the same codes << 8 under the matrix with its first three columns x 2^-8 (a power of two commutes
   with every rounding of the chain), hence P010 of (byte << 8) under the default 16-bit state against NV12 under the default 8-bit
   state; P016 against the planar tap of the de-interleaved planes.
2. The taps against the numpy float64 statement with real 10 / 12 / 16-bit planes: every byte within 0.5 + yuv16_ref.margin of the
   clamped unrounded float64 value, and at least 99.5 % of the bytes equal to rint of it.
3. Words above 0x7fff are read as unsigned.  4. Layouts.  5. The planner's edges with 2-byte samples.
6. The forward: the logits of every 16-bit entry point EQUAL those of forward_u8 given the tap's own output.  7. One frames ring
   takes all kinds of submit.  8. Refusals enqueue nothing."""
import ctypes as C

import numpy as np
import pytest

import nv12_ref as N
import vh_synth as S
import vithip
import yuv16_ref as W
import yuv_ref as Y
from test_gpu_frames import GUARD, PATCH14_MICRO, DTNAME, same_bits
from test_gpu_nv12 import tap as tap_nv12
from test_gpu_yuv_planar import planner_boundary_444
from test_gpu_yuv_planar import tap as tap_yuv
from test_nv12 import make_nv12, make_rgb
from test_yuv16 import COLOURS16, make_yuv16
from test_yuv_planar import COLOURS, OP_CASES, SUBS, make_yuv

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE = 1, 3
P010 = "bt709_limited_10_msb_left"                                                 # the format of the default 16-bit colour state
EVEN_CASES = [n for n, c in OP_CASES.items() if c[0] % 2 == 0 and c[1] % 2 == 0]


def words(a):
    """[rows, cols] uint16 -> [rows, 2 cols] bytes, low byte first."""
    a = np.ascontiguousarray(a, "<u2")
    return a.view(np.uint8).reshape(a.shape[0], -1)


def lay_out16(planes, boxes, subs=None, pads=(0, 0, 0), lead=0, gap=0, order="yuv"):
    """test_gpu_yuv_planar.lay_out for uint16 planes: `lead` BYTES in front, `gap` bytes behind every plane, rows of Y / U / V padded
    by pads[0..2] bytes (all of them even), each frame's planes in `order`."""
    desc = (vithip.FrameYUV * len(planes))()
    chunks, off = [np.full(lead, 0xEE, np.uint8)], lead
    for i, (yuv, box) in enumerate(zip(planes, boxes)):
        h, w = yuv[0].shape
        d = desc[i]
        d.sub_x, d.sub_y = Y.subsampling(yuv[0].shape, yuv[1].shape) if subs is None else subs[i]
        for key in order:
            k = "yuv".index(key)
            rows, cols = yuv[k].shape
            stride = 2 * cols + pads[k]
            buf = np.full((rows, stride), 0xEE, np.uint8)
            buf[:, :2 * cols] = words(yuv[k])
            flat = buf.reshape(-1)[:(rows - 1) * stride + 2 * cols]                # the last row carries no padding
            setattr(d, key + "_offset", off)
            setattr(d, key + "_stride", stride)
            chunks += [flat, np.full(gap, 0xEE, np.uint8)]
            off += flat.size + gap
        d.height, d.width = h, w
        d.box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return np.concatenate(chunks), desc


def lay_out_p016(planes, boxes, y_pad=0, uv_pad=0, lead=0, gap=0, uv_first=False):
    """test_gpu_nv12.lay_out for (Y [H, W], UV [H/2, W/2, 2]) uint16 pairs; pads, lead and gap in bytes, all even."""
    desc = (vithip.FrameNV12 * len(planes))()
    chunks, off = [np.full(lead, 0xEE, np.uint8)], lead
    for i, ((y, uv), box) in enumerate(zip(planes, boxes)):
        h, w = y.shape
        parts = {}
        for key, a, rows, pad in (("y", y, h, y_pad), ("uv", uv.reshape(h // 2, w), h // 2, uv_pad)):
            stride = 2 * w + pad
            buf = np.full((rows, stride), 0xEE, np.uint8)
            buf[:, :2 * w] = words(a)
            parts[key] = (buf.reshape(-1)[:(rows - 1) * stride + 2 * w], stride)
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


def run_tap(op, buf, desc, s, m, site):
    """One of the two taps -> [n, s, s, 3] bytes; checks that nothing but the output was written."""
    n = len(desc) * s * s * 3
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.full(n + GUARD, 0xA5, np.uint8))
    try:
        op(din.ptr, buf.nbytes, desc, s, m, site, dout.ptr)
        raw = dout.to_numpy(np.uint8, (n + GUARD,))
    finally:
        din.free(); dout.free()
    assert (raw[n:] == 0xA5).all()                                   # the guard bytes behind the output
    return raw[:n].reshape(len(desc), s, s, 3)


def tap16(planes, boxes, s, m, site, subs=None, **layout):
    return run_tap(vithip.op_resize_yuv16, *lay_out16(planes, boxes, subs, **layout), s, m, site)


def tap_p016(planes, boxes, s, m, site, **layout):
    return run_tap(vithip.op_resize_p016, *lay_out_p016(planes, boxes, **layout), s, m, site)


def pairs_of(planes):
    """4:2:0 (Y, U, V) triples of even size -> P016 (Y, UV) pairs."""
    return [(y, Y.interleave(u, v)) for y, u, v in planes]


def check_against_statement(got, planes, boxes, s, m, site, vmax, subs=None, label=""):
    for i, (g, yuv, box) in enumerate(zip(got, planes, boxes)):
        sub = Y.subsampling(yuv[0].shape, yuv[1].shape) if subs is None else subs[i]
        err, bound, same = W.statement_figures(g, yuv, box, s, m, site, sub, vmax)
        print(f"yuv16 sub {sub} {yuv[0].shape[0]}x{yuv[0].shape[1]} box {box} -> {s} {label}: max |got - v64| = {err:.6f} (bound {bound:.6f}), {100 * same:.3f} % equal rint(v64)")
        assert err <= bound
        assert same >= 0.995


def colour16(name):
    """(matrix, chroma_site, largest word) of a COLOURS16 entry."""
    std, full, bits, msb, site = COLOURS16[name]
    return vithip.yuv_matrix16(std, full, bits, msb), site, W.largest_word(bits, msb)


# ---- 1. exact ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_8_bit_codes_in_16_bit_words_give_the_8_bit_kernel_s_bytes(name, sub, colour):
    h, w, box, s = OP_CASES[name]
    std, full, site = COLOURS[colour]
    planes = make_yuv(h, w, SUBS[sub], seed=h + w)
    m = vithip.yuv_matrix(std, full)
    want = tap_yuv([planes], [box], s, m, site, subs=[SUBS[sub]])
    wide = tuple(p.astype(np.uint16) for p in planes)
    assert np.array_equal(tap16([wide], [box], s, m, site, subs=[SUBS[sub]]), want)
    # the codes in the high byte, the first three columns of the matrix x 2^-8: every product, sum and rounding scales exactly
    m8 = m.copy()
    m8[:, :3] *= np.float32(2.0 ** -8)
    high = tuple((p << 8).astype(np.uint16) for p in wide)
    assert np.array_equal(tap16([high], [box], s, m8, site, subs=[SUBS[sub]]), want)


@pytest.mark.parametrize("name", EVEN_CASES)
def test_p010_of_byte_shl_8_under_the_default_16_bit_state_equals_nv12_under_the_default_8_bit_state(name):
    h, w, box, s = OP_CASES[name]
    y, uv = make_nv12(h, w, seed=h + w)
    want = tap_nv12([(y, uv)], [box], s, vithip.yuv_matrix(), N.CHROMA_LEFT)
    pair = ((y.astype(np.uint16) << 8).astype(np.uint16), (uv.astype(np.uint16) << 8).astype(np.uint16))
    assert np.array_equal(tap_p016([pair], [box], s, vithip.yuv_matrix16(), N.CHROMA_LEFT), want)


@pytest.mark.parametrize("colour", [P010, "bt709_full_16_msb_centre"])
@pytest.mark.parametrize("name", EVEN_CASES)
def test_p016_equals_the_planar_tap_of_the_de_interleaved_planes(name, colour):
    h, w, box, s = OP_CASES[name]
    m, site, _ = colour16(colour)
    y, u, v = make_yuv16(h, w, (2, 2), seed=h + w, colour=colour)
    want = tap_p016([(y, Y.interleave(u, v))], [box], s, m, site)
    assert np.array_equal(tap16([(y, u, v)], [box], s, m, site, subs=[(2, 2)]), want)
    # YV12-style: Y, V, U in memory, the descriptor's u_offset and v_offset exchanged accordingly
    assert np.array_equal(tap16([(y, u, v)], [box], s, m, site, subs=[(2, 2)], order="yvu"), want)


# ---- 2. the statement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", list(COLOURS16))
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("name", list(OP_CASES))
def test_op_resize_yuv16_matches_the_statement(name, sub, colour):
    h, w, box, s = OP_CASES[name]
    m, site, vmax = colour16(colour)
    planes = [make_yuv16(h, w, SUBS[sub], seed=h + w, colour=colour)]
    check_against_statement(tap16(planes, [box], s, m, site, [SUBS[sub]]), planes, [box], s, m, site, vmax, [SUBS[sub]], f"{sub} {colour}")


@pytest.mark.parametrize("colour", [P010, "bt709_full_16_msb_centre"])
@pytest.mark.parametrize("name", EVEN_CASES)
def test_op_resize_p016_matches_the_statement(name, colour):
    h, w, box, s = OP_CASES[name]
    m, site, vmax = colour16(colour)
    planes = [make_yuv16(h, w, (2, 2), seed=h + w, colour=colour)]
    check_against_statement(tap_p016(pairs_of(planes), [box], s, m, site), planes, [box], s, m, site, vmax, [(2, 2)], f"p016 {colour}")


# ---- 3. unsigned words ----------------------------------------------------------------------------------------------------------
UNIT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32) * np.float32(255.0 / 65535.0)


def test_all_ones_words_give_all_255_bytes():
    """A word of 0xFFFF read as int16 is -1, which the clamp turns into 0: any sign-extending load shows in every byte."""
    for h, w, s in ((38, 54, 16), (20, 24, 32)):
        full = lambda *shape: np.full(shape, 0xFFFF, np.uint16)
        for sub in SUBS.values():
            ch, cw = Y.chroma_size(h, w, *sub)
            assert (tap16([(full(h, w), full(ch, cw), full(ch, cw))], [None], s, UNIT, N.CHROMA_LEFT, [sub]) == 255).all()
        pair = [(full(h, w), full(h // 2, w // 2, 2))]
        assert (tap_p016(pair, [None], s, UNIT, N.CHROMA_LEFT) == 255).all()               # one 32-bit load per pair
        assert (tap_p016(pair, [None], s, UNIT, N.CHROMA_LEFT, lead=2) == 255).all()       # two 16-bit loads


def test_words_either_side_of_the_sign_bit_match_the_emulation_exactly():
    h, w, s = 38, 54, 16
    alt = lambda rows, cols, ph: np.where((np.add.outer(np.arange(rows), np.arange(cols)) + ph) % 2, 0x8000, 0x7FFF).astype(np.uint16)
    y, u, v = alt(h, w, 0), alt(h // 2, w // 2, 1), alt(h // 2, w // 2, 0)
    for m, site in ((UNIT, N.CHROMA_LEFT), (vithip.yuv_matrix16(vithip.YUV_BT709, True, 16, True), N.CHROMA_CENTER)):
        want = Y.resize_yuv_f32(y, u, v, None, s, m, site, (2, 2))
        assert want.min() > 0 and want.max() < 255                                         # nothing hides behind the clamp
        assert np.array_equal(tap16([(y, u, v)], [None], s, m, site, [(2, 2)])[0], want)
        assert np.array_equal(tap_p016([(y, Y.interleave(u, v))], [None], s, m, site)[0], want)
        assert np.array_equal(tap_p016([(y, Y.interleave(u, v))], [None], s, m, site, lead=2)[0], want)


# ---- 4. layout ------------------------------------------------------------------------------------------------------------------
def test_padded_even_strides_any_order_planes_apart_and_lead_bytes():
    colour = "bt601_full_12_lsb_centre"
    m, site, vmax = colour16(colour)
    planes = [make_yuv16(37, 53, (2, 2), 21, colour), make_yuv16(42, 31, (2, 1), 31, colour), make_yuv16(29, 30, (1, 1), 41, colour)]
    boxes = [None, (0.5, 3.0, 29.5, 40.0), None]
    want = tap16(planes, boxes, 16, m, site)                                       # packed: Y, U, V back to back
    check_against_statement(want, planes, boxes, 16, m, site, vmax)
    layouts = [dict(pads=(6, 10, 2)),                          # padded rows, a different padding per plane, none a multiple of 4
               dict(pads=(4, 0, 0), lead=2),
               dict(pads=(0, 2, 0)),                           # U and V rows no longer in step
               dict(pads=(0, 0, 14)),
               dict(lead=6, gap=2),                            # offsets that are even and no multiple of 4
               dict(order="yvu"),
               dict(gap=64, order="uvy"),                      # chroma in front of luma, planes not adjacent
               dict(lead=10, gap=6, order="vyu", pads=(2, 0, 4))]
    for lay in layouts:
        assert np.array_equal(tap16(planes, boxes, 16, m, site, **lay), want), lay


def test_p016_pair_loads_and_word_loads_give_the_same_bytes():
    """uv_offset, uv_stride = 0 (mod 4): one 32-bit load per (U, V) pair.  Either = 2 (mod 4): two 16-bit loads."""
    m, site, vmax = colour16(P010)
    planes = [make_yuv16(38, 54, (2, 2), 21, P010), make_yuv16(42, 30, (2, 2), 31, P010)]
    boxes = [None, (0.5, 3.0, 29.5, 40.0)]
    pairs = pairs_of(planes)
    buf, desc = lay_out_p016(pairs, boxes)
    assert all(d.uv_offset % 4 == 0 and d.uv_stride % 4 == 0 for d in desc)
    want = tap_p016(pairs, boxes, 16, m, site)
    check_against_statement(want, planes, boxes, 16, m, site, vmax)
    buf, desc = lay_out_p016(pairs, boxes, lead=2)
    assert all(d.uv_offset % 4 == 2 for d in desc)
    buf, desc = lay_out_p016(pairs, boxes, uv_pad=2)
    assert all(d.uv_stride % 4 == 2 for d in desc)
    for lay in (dict(lead=2), dict(uv_pad=2), dict(lead=4), dict(y_pad=6, uv_pad=12), dict(lead=2, gap=2, y_pad=2, uv_pad=6), dict(gap=64, uv_first=True),
                dict(gap=2, uv_first=True)):
        assert np.array_equal(tap_p016(pairs, boxes, 16, m, site, **lay), want), lay


def test_mixed_batch_of_sizes_subsamplings_and_boxes():
    colour = "bt2020_limited_10_lsb_left"
    m, site, vmax = colour16(colour)
    shapes = [(37, 53, "420"), (64, 64, "444"), (20, 24, "422"), (98, 132, "440"), (270, 480, "420"), (1, 1, "420"), (33, 2, "422")]
    planes = [make_yuv16(h, w, SUBS[k], 40 + i, colour) for i, (h, w, k) in enumerate(shapes)]
    subs = [SUBS[k] for _, _, k in shapes]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
    got = tap16(planes, boxes, 32, m, site, subs, lead=2, gap=6)
    check_against_statement(got, planes, boxes, 32, m, site, vmax, subs)
    for i in range(len(planes)):                                       # each frame alone gives the same bytes as in the batch
        assert np.array_equal(tap16([planes[i]], [boxes[i]], 32, m, site, [subs[i]])[0], got[i])
    # a P016 batch of three sizes and boxes
    pp = [make_yuv16(h, w, (2, 2), 60 + i, colour) for i, (h, w) in enumerate(((38, 54), (20, 24), (270, 480)))]
    pb = [None, (2.0, 1.0, 22.0, 19.5), vithip.center_crop_box(270, 480)]
    gp = tap_p016(pairs_of(pp), pb, 32, m, site, lead=2, gap=2)
    check_against_statement(gp, pp, pb, 32, m, site, vmax)
    for i in range(len(pp)):
        assert np.array_equal(tap_p016(pairs_of(pp[i:i + 1]), [pb[i]], 32, m, site)[0], gp[i])


# ---- 5. the planner's edges with 2-byte samples ---------------------------------------------------------------------------------
def test_one_1080p_p010_frame_spans_many_bands():
    """64 output rows from 1080: the band cap of a one-frame call (S / 64 = 1 row) gives 64 bands of about 34 luma rows."""
    s = S.CONFIGS["vit_micro"]["image_size"]
    m, site, vmax = colour16(P010)
    planes = [W.rgb_to_yuv16_planes(make_rgb(1080, 1920, 3), 2, 2, 10, True)]
    box = vithip.center_crop_box(1080, 1920)
    check_against_statement(tap_p016(pairs_of(planes), [box], s, m, site), planes, [box], s, m, site, vmax)


@pytest.mark.parametrize("which", ["largest_full_width", "smallest_narrowed"])
def test_444_narrows_the_column_tiles_at_the_planner_s_boundary_with_16_bit_samples(which):
    """The two shapes of test_gpu_yuv_planar's boundary test: the LDS holds fp32 whatever the sample, so the boundary is the same."""
    s = 130
    h_full, h_narrow = planner_boundary_444(s)
    h = h_full if which == "largest_full_width" else h_narrow
    colour = "bt601_full_12_lsb_centre"
    m, site, vmax = colour16(colour)
    planes = [make_yuv16(h, 36, (1, 1), 7, colour)]
    check_against_statement(tap16(planes, [None], s, m, site, [(1, 1)]), planes, [None], s, m, site, vmax, [(1, 1)])


def test_large_batch_of_small_frames_runs_tall_bands():
    m, site, vmax = colour16(P010)
    keys = list(SUBS)
    subs = [SUBS[keys[i % 4]] for i in range(40)]
    planes = [make_yuv16(41, 39, subs[i], 100 + i, P010) for i in range(40)]
    boxes = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    got = tap16(planes, boxes, 32, m, site, subs)
    check_against_statement(got[::9], planes[::9], boxes[::9], 32, m, site, vmax, subs[::9])
    for i in (0, 5, 18, 39):
        assert np.array_equal(tap16([planes[i]], [boxes[i]], 32, m, site, [subs[i]])[0], got[i])


# ---- 6. the forward -------------------------------------------------------------------------------------------------------------
def planar_set(s, colour=P010):
    """Three planar 16-bit frames: an even 4:2:0 one with a centre crop, an odd 4:2:2 one, a 4:4:0 one with a box."""
    shapes = [(s + 16, s + 36, "420"), (s + 1, s + 3, "422"), (s // 2 + 6, s // 2 + 23, "440")]
    planes = [make_yuv16(h, w, SUBS[k], 1 + i, colour) for i, (h, w, k) in enumerate(shapes)]
    return planes, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)]


def p010_set(s, colour=P010):
    """Three P010 frames as a hardware decoder emits them."""
    shapes = [(s + 16, s + 36), (s + 2, s + 4), (s // 2 + 6, s // 2 + 24)]
    pairs = pairs_of([make_yuv16(h, w, (2, 2), 11 + i, colour) for i, (h, w) in enumerate(shapes)])
    return pairs, [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)]


def device_logits(call, buf, desc, classes):
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((len(desc), classes), np.float32))
    try:
        call(din.ptr, buf.nbytes, desc, dout.ptr)
        return dout.to_numpy(np.float32, (len(desc), classes))
    finally:
        din.free(); dout.free()


FORWARD_CASES = [(n, c, d) for n, c in (("vit_micro", S.CONFIGS["vit_micro"]), ("patch14_micro", PATCH14_MICRO))
                 for d in (vithip.DTYPE_BF16, vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_every_16_bit_entry_point_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    m, site = ctx.get_frame_colour16()                     # the default: P010 as a hardware decoder writes it
    assert np.array_equal(m, vithip.yuv_matrix16(vithip.YUV_BT709, False, 10, True)) and site == vithip.CHROMA_LEFT
    planes, boxes = planar_set(s)
    pairs, pboxes = p010_set(s)
    want = ctx.forward_u8(tap16(planes, boxes, s, m, site))
    wantp = ctx.forward_u8(tap_p016(pairs, pboxes, s, m, site))
    assert np.isfinite(want).all() and np.isfinite(wantp).all() and not np.array_equal(want, wantp)
    assert same_bits(ctx.forward_frames_yuv16(planes, boxes), want)
    assert same_bits(ctx.forward_frames_p016(pairs, pboxes), wantp)
    buf, desc = lay_out16(planes, boxes, pads=(6, 2, 10), lead=2, gap=2, order="vyu")
    assert same_bits(device_logits(ctx.forward_device_frames_yuv16, buf, desc, cfg["classes"]), want)
    bufp, descp = lay_out_p016(pairs, pboxes, y_pad=2, uv_pad=6, lead=2)
    assert same_bits(device_logits(ctx.forward_device_frames_p016, bufp, descp, cfg["classes"]), wantp)
    ctx.ring_create_frames(2, 3, max(buf.nbytes, bufp.nbytes))
    try:
        ctx.ring_submit_frames_yuv16(planes, boxes)
        ctx.ring_submit_frames_p016_packed(bufp, bufp.nbytes, descp)
        assert same_bits(ctx.ring_collect(), want) and same_bits(ctx.ring_collect(), wantp)
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)
    ctx.close()


@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
    ctx.init_weights_seeded(17)
    planes, boxes = planar_set(s)
    pairs, pboxes = p010_set(s)
    m, site = ctx.get_frame_colour16()
    ref = ctx.forward_u8(tap16(planes, boxes, s, m, site))         # computed once; the tests below only read them
    refp = ctx.forward_u8(tap_p016(pairs, pboxes, s, m, site))
    ref.setflags(write=False); refp.setflags(write=False)
    yield ctx, cfg, planes, boxes, ref, pairs, pboxes, refp
    ctx.close()


def test_device_entry_points_with_streams_and_graphs(micro):
    ctx, cfg, planes, boxes, ref, pairs, pboxes, refp = micro
    buf, desc = lay_out16(planes, boxes, pads=(2, 6, 2), lead=6, gap=2, order="uvy")
    bufp, descp = lay_out_p016(pairs, pboxes, uv_pad=2, gap=2, uv_first=True)
    din, dinp = vithip.DeviceBuffer.from_numpy(buf), vithip.DeviceBuffer.from_numpy(bufp)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    logits = lambda: dout.to_numpy(np.float32, (3, cfg["classes"]))
    try:
        ctx.set_streams(2)                                                         # the resize runs once, before the fork
        ctx.set_graph(True)
        for _ in range(3):                                                         # eager, captured, replayed
            ctx.forward_device_frames_yuv16(din.ptr, buf.nbytes, desc, dout.ptr)
            assert same_bits(logits(), ref)
        assert ctx.get_graph()[0] and ctx.get_graph()[1] >= 1
        # other frames, of the other layout, through the replayed graph: the resize in front of it is no part of the capture
        ctx.forward_device_frames_p016(dinp.ptr, bufp.nbytes, descp, dout.ptr)
        assert same_bits(logits(), refp)
        assert same_bits(ctx.forward_frames_yuv16(planes[::-1], boxes[::-1]), ref[::-1])
        assert same_bits(ctx.forward_frames_p016(pairs, pboxes), refp)
    finally:
        ctx.set_graph(False)
        ctx.set_streams(1)
        din.free(); dinp.free(); dout.free()


def test_stage_timing_reports_one_resize_launch(micro):
    ctx, cfg, planes, boxes, ref, pairs, pboxes, refp = micro
    try:
        ctx.set_stage_timing("resize")
        for call, args, want in ((ctx.forward_frames_yuv16, (planes, boxes), ref), (ctx.forward_frames_p016, (pairs, pboxes), refp)):
            assert same_bits(call(*args), want)
            avg, mn, n = ctx.get_stage_timing()
            assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_the_two_colour_states_do_not_touch_each_other(micro):
    ctx, cfg, planes, boxes, ref, pairs, pboxes, refp = micro
    s = cfg["image_size"]
    nv12 = [make_nv12(s + 4, s + 10, seed=12)]
    m8, site8 = ctx.get_frame_colour()
    ref_nv12 = ctx.forward_frames_nv12(nv12)
    try:
        # the 16-bit state: changes the 16-bit result, not the NV12 one
        m16 = vithip.yuv_matrix16(vithip.YUV_BT2020, True, 10, True)
        ctx.set_frame_colour16(m16, vithip.CHROMA_CENTER)
        got_m, got_site = ctx.get_frame_colour16()
        assert np.array_equal(got_m, m16) and got_site == vithip.CHROMA_CENTER
        moved = ctx.forward_frames_p016(pairs, pboxes)
        assert same_bits(moved, ctx.forward_u8(tap_p016(pairs, pboxes, s, m16, vithip.CHROMA_CENTER))) and not np.array_equal(moved, refp)
        assert same_bits(ctx.forward_frames_yuv16(planes, boxes), ctx.forward_u8(tap16(planes, boxes, s, m16, vithip.CHROMA_CENTER)))
        assert np.array_equal(ctx.get_frame_colour()[0], m8) and ctx.get_frame_colour()[1] == site8
        assert same_bits(ctx.forward_frames_nv12(nv12), ref_nv12)
        # the 8-bit state: changes the NV12 result, not the 16-bit one
        mj = vithip.yuv_matrix(vithip.YUV_BT601, True)
        ctx.set_frame_colour(mj, vithip.CHROMA_CENTER)
        assert not np.array_equal(ctx.forward_frames_nv12(nv12), ref_nv12)
        assert np.array_equal(ctx.get_frame_colour16()[0], m16) and ctx.get_frame_colour16()[1] == vithip.CHROMA_CENTER
        assert same_bits(ctx.forward_frames_p016(pairs, pboxes), moved)
        # None restores each default on its own
        ctx.set_frame_colour16(None)
        assert same_bits(ctx.forward_frames_p016(pairs, pboxes), refp) and same_bits(ctx.forward_frames_yuv16(planes, boxes), ref)
        assert np.array_equal(ctx.get_frame_colour()[0], mj)
    finally:
        ctx.set_frame_colour(None)
        ctx.set_frame_colour16(None)
    assert same_bits(ctx.forward_frames_nv12(nv12), ref_nv12)
    with pytest.raises(vithip.VhError) as e:
        ctx.set_frame_colour16(np.full(12, np.nan, np.float32))
    assert e.value.code == VH_ERR_INVALID and "not finite" in str(e.value)
    with pytest.raises(vithip.VhError):
        ctx.set_frame_colour16(m8, 2)
    assert np.array_equal(ctx.get_frame_colour16()[0], vithip.yuv_matrix16())


# ---- 7. one frames ring for every kind ------------------------------------------------------------------------------------------
def test_frames_ring_takes_nv12_p016_planar_and_planar_16_bit_alternately(micro):
    ctx, cfg, planes, boxes, ref, pairs, pboxes, refp = micro
    s = cfg["image_size"]
    nv12 = [make_nv12(s + 4, s + 10, seed=12)]
    ref_nv12 = ctx.forward_frames_nv12(nv12)
    yuv8 = [make_yuv(s + 1, s + 3, (2, 1), seed=13), make_yuv(s + 5, s + 2, (2, 2), seed=14)]
    ref_yuv8 = ctx.forward_frames_yuv(yuv8)
    ctx.ring_create_frames(4, 3, 1 << 17)
    try:
        ctx.ring_submit_frames_nv12(nv12)
        ctx.ring_submit_frames_p016(pairs, pboxes)
        ctx.ring_submit_frames_yuv(yuv8)
        # slot 3: 16-bit planes filled in place
        buf, desc = lay_out16(planes[1:], boxes[1:], lead=2)
        ctx.ring_input_frames()[:buf.size] = buf
        ctx.ring_submit_frames_yuv16_packed(None, buf.size, desc)
        assert ctx.ring_free_slots() == 0
        assert same_bits(ctx.ring_collect(), ref_nv12)                             # FIFO
        ctx.ring_submit_frames_yuv16(planes[::-1], boxes[::-1])
        assert same_bits(ctx.ring_collect(), refp)
        assert same_bits(ctx.ring_collect(), ref_yuv8)
        assert same_bits(ctx.ring_collect(), ref[1:])
        assert same_bits(ctx.ring_collect(), ref[::-1])
        assert ctx.ring_free_slots() == 4
        # a refused 16-bit submit (odd stride) leaves the ring as it was, for both layouts
        buf, desc = lay_out16(planes[:1], boxes[:1])
        desc[0].y_stride += 1
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_yuv16_packed(buf, buf.size, desc)
        assert e.value.code == VH_ERR_INVALID and "stride is odd" in str(e.value) and ctx.ring_free_slots() == 4
        bufp, descp = lay_out_p016(pairs[:1], pboxes[:1])
        descp[0].uv_stride += 1
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames_p016_packed(bufp, bufp.size, descp)
        assert e.value.code == VH_ERR_INVALID and "stride is odd" in str(e.value) and ctx.ring_free_slots() == 4
        ctx.ring_submit_frames_p016(pairs, pboxes)
        assert same_bits(ctx.ring_collect(), refp)
        # 16-bit submits on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            for call, args in ((ctx.ring_submit_frames_yuv16, (planes[:1], boxes[:1])), (ctx.ring_submit_frames_p016, (pairs[:1], pboxes[:1]))):
                with pytest.raises(vithip.VhError) as e:
                    call(*args)
                assert e.value.code == VH_ERR_STATE and ctx.ring_free_slots() == 2
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(micro):
    ctx, cfg, planes, boxes, ref, pairs, pboxes, refp = micro
    L = vithip.lib()
    buf, desc = lay_out16(planes, boxes)
    bufp, descp = lay_out_p016(pairs, pboxes)
    out = np.zeros((3, cfg["classes"]), np.float32)

    def call(n=3, nbytes=buf.nbytes, d=desc):
        return L.vh_forward_frames_yuv16(ctx.h, buf.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    def callp(n=3, nbytes=bufp.nbytes, d=descp):
        return L.vh_forward_frames_p016(ctx.h, bufp.ctypes.data, nbytes, None if d is None else C.addressof(d), n, out.ctypes.data)

    assert call(n=4) == VH_ERR_INVALID and callp(n=4) == VH_ERR_INVALID            # batch > max_batch
    assert same_bits(ctx.forward_frames_yuv16(planes, boxes), ref)
    assert call(nbytes=buf.nbytes - 1) == VH_ERR_INVALID                           # the last V byte beyond nbytes
    assert callp(nbytes=bufp.nbytes - 1) == VH_ERR_INVALID
    assert call(d=None) == VH_ERR_INVALID and callp(d=None) == VH_ERR_INVALID
    desc[1].u_offset += 1
    assert call() == VH_ERR_INVALID and "offset is odd" in L.vh_last_error(ctx.h).decode()
    desc[1].u_offset -= 1
    desc[0].v_stride = desc[0].v_stride // 2                                        # the stride of the 8-bit layout
    assert call() == VH_ERR_INVALID
    desc[0].v_stride *= 2
    desc[2].sub_y = 0
    assert call() == VH_ERR_INVALID
    desc[2].sub_y = 2
    descp[1].y_stride -= 2
    assert callp() == VH_ERR_INVALID and "2 * width" in L.vh_last_error(ctx.h).decode()
    descp[1].y_stride += 2
    descp[2].box[2] = descp[2].width + 0.5
    assert callp() == VH_ERR_INVALID
    descp[2].box[2] = pboxes[2][2]
    assert not out.any()                                                           # nothing ran
    # an odd device frames pointer is refused before the device is asked anything; the same buffer one byte on is taken
    dev = vithip.DeviceBuffer.from_numpy(np.concatenate([np.zeros(2, np.uint8), buf]))
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    try:
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_frames_yuv16(dev.ptr + 1, buf.nbytes, desc, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "frames pointer is odd" in str(e.value)
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_frames_p016(dev.ptr + 1, bufp.nbytes, descp, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "frames pointer is odd" in str(e.value)
        assert not dout.to_numpy(np.float32, (3, cfg["classes"])).any()
        ctx.forward_device_frames_yuv16(dev.ptr + 2, buf.nbytes, desc, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
    finally:
        dev.free(); dout.free()
    assert same_bits(ctx.forward_frames_p016(pairs, pboxes), refp)
    # a context with one channel is refused, and goes on working
    cfg1 = dict(cfg, channels=1)
    c1 = vithip.VitContext(cfg1, dtype=vithip.DTYPE_BF16, max_batch=3)
    c1.init_weights_seeded(5)
    from test_gpu_frames import make_frame
    grey = [make_frame(cfg["image_size"], cfg["image_size"], 1, seed=4)]
    before = c1.forward_frames(grey)
    for callc, args in ((c1.forward_frames_yuv16, (planes, boxes)), (c1.forward_frames_p016, (pairs, pboxes))):
        with pytest.raises(vithip.VhError) as e:
            callc(*args)
        assert e.value.code == VH_ERR_INVALID and "3 channels" in str(e.value)
    assert same_bits(c1.forward_frames(grey), before)
    c1.close()
