"""GPU suite of the frames entry points (include/vithip.h, "8-bit frames").

1. The operator tap vh_op_resize_u8 against frames_ref, the numpy float64 statement of the contract, with two assertions:
   every byte within 0.5 + margin of the unrounded float64 value v64, and at least 99.5 % of the bytes equal to rint(v64) (the
   cap keeps the first criterion from hiding a systematically shifted image).  The margin is the worst-case error of the two fp32
   fmaf chains: (taps_x + taps_y) * 255 * 2^-24, which is below 1e-3 up to 2 * 29 taps -- every case but the scale-32 one uses 1e-3.
2. The forward: the logits of every frames entry point EQUAL those of forward_u8 given the tap's own output, on every path."""
import ctypes as C

import numpy as np
import pytest

import frames_ref as R
import vh_synth as S
import vithip
from tensor_ref import u8_reference
from test_u8_input import IMAGENET_MEAN, IMAGENET_STD
from vh_testlib import same_bits

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_RING_FULL = 1, 3, 6
GUARD = 4096
DTNAME = {vithip.DTYPE_BF16: "bf16", vithip.DTYPE_FP16: "fp16", vithip.DTYPE_FP8: "fp8"}
PATCH14_MICRO = dict(image_size=28, patch_size=14, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=8)


def make_frame(h, w, ch, seed):
    """Smooth structure plus noise: neighbouring taps differ, and a shifted or transposed result is far from the reference."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 96.0 + 80.0 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0) + 0.11 * x - 0.07 * y
    img = base[:, :, None] + 13.0 * np.arange(ch)[None, None, :] + rng.normal(0.0, 40.0, (h, w, ch))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def lay_out(frames, boxes, pad=0, lead=0, gap=0):
    """Frames into one buffer with `lead` bytes in front, `gap` bytes between them and rows padded by `pad` bytes."""
    desc = (vithip.Frame * len(frames))()
    chunks, off = [np.full(lead, 0xEE, np.uint8)], lead
    for i, (f, box) in enumerate(zip(frames, boxes)):
        h, w, ch = f.shape
        stride = w * ch + pad
        rows = np.full((h, stride), 0xEE, np.uint8)
        rows[:, :w * ch] = f.reshape(h, w * ch)
        flat = rows.reshape(-1)[:(h - 1) * stride + w * ch]          # the last row carries no padding
        desc[i].offset, desc[i].height, desc[i].width, desc[i].row_stride = off, h, w, stride
        desc[i].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
        chunks += [flat, np.full(gap, 0xEE, np.uint8)]
        off += flat.size + gap
    return np.concatenate(chunks), desc


def tap(frames, boxes, s, pad=0, lead=0, gap=0):
    """vh_op_resize_u8 -> [n, s, s, ch] bytes; checks that nothing but the output was written."""
    ch = frames[0].shape[2]
    buf, desc = lay_out(frames, boxes, pad, lead, gap)
    n = len(frames) * s * s * ch
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.full(n + GUARD, 0xA5, np.uint8))
    try:
        vithip.op_resize_u8(din.ptr, buf.nbytes, desc, ch, s, dout.ptr)
        raw = dout.to_numpy(np.uint8, (n + GUARD,))
    finally:
        din.free(); dout.free()
    assert (raw[n:] == 0xA5).all()                                   # the guard bytes behind the output
    return raw[:n].reshape(len(frames), s, s, ch)


def check_against_statement(got, frames, boxes, s):
    for g, f, box in zip(got, frames, boxes):
        v64 = R.resize_f64(f, box, s)
        h, w, _ = f.shape
        x0, y0, x1, y1 = (0.0, 0.0, w, h) if box is None else box
        taps = int(R.axis_table(w, np.float32(x0), np.float32(x1), s)[1].max()) + int(R.axis_table(h, np.float32(y0), np.float32(y1), s)[1].max())
        margin = max(1e-3, taps * 255 * 2.0 ** -24)
        err = float(np.abs(g.astype(np.float64) - v64).max())
        same = float((g == R.to_bytes(v64)).mean())
        print(f"resize {h}x{w}x{f.shape[2]} box {box} -> {s}: max |got - v64| = {err:.6f} (bound {0.5 + margin:.6f}), {100 * same:.3f} % equal rint(v64)")
        assert err <= 0.5 + margin
        assert same >= 0.995


# (h, w, channels, box, S): the smallest shapes that reach each code path
OP_CASES = {
    "down_37x53_16": (37, 53, 3, None, 16),                          # non-integer down-scale
    "up_20x24_32": (20, 24, 3, None, 32),                            # up-scale, two taps, exact ties; 16-byte stores
    "box_97x131_28": (97, 131, 3, (10.0, 5.0, 101.0, 96.0), 28),     # off-centre box; S * C = 84 is no multiple of 16: byte stores
    "fractional_box": (97, 131, 3, (10.25, 5.5, 101.75, 95.125), 28),
    "taps29_270x480_32": (270, 480, 3, None, 32),
    "one_channel": (37, 53, 1, None, 16),
    "four_channels": (37, 53, 4, (1.5, 0.0, 50.0, 37.0), 16),        # 32-bit loads (offset 0, stride 212)
    "four_channels_up": (20, 24, 4, None, 32),
    "scale32_column_tiles": (2304, 80, 4, None, 72),                 # 64 source rows x 72 x 4 floats exceed the LDS: two column tiles
}


@pytest.mark.parametrize("name", list(OP_CASES))
def test_op_resize_matches_the_statement(name):
    h, w, ch, box, s = OP_CASES[name]
    frames = [make_frame(h, w, ch, seed=h + w + ch)]
    got = tap(frames, [box], s)
    check_against_statement(got, frames, [box], s)


def test_identity_returns_the_input_bytes():
    for ch in (1, 3, 4):
        f = make_frame(64, 64, ch, seed=ch)
        assert np.array_equal(tap([f], [None], 64)[0], f)
    # and the 0.875 centre box of a larger frame at scale exactly 1 is that crop
    f = make_frame(32, 40, 3, seed=11)
    assert np.array_equal(tap([f], [(8.0, 2.0, 36.0, 30.0)], 28)[0], f[2:30, 8:36])


def test_one_1080p_frame_spans_many_bands():
    f = make_frame(1080, 1920, 3, seed=3)
    box = vithip.center_crop_box(1080, 1920)
    got = tap([f], [box], 224)
    check_against_statement(got, [f], [box], 224)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_padded_rows_and_odd_offsets(ch):
    frames = [make_frame(37, 53, ch, seed=20 + ch), make_frame(41, 30, ch, seed=30 + ch)]
    boxes = [None, (0.5, 3.0, 29.5, 40.0)]
    want = tap(frames, boxes, 16)
    check_against_statement(want, frames, boxes, 16)
    # the same frames behind padded rows (stride = width * C + 5), at odd byte offsets, or both: the same bytes
    for pad, lead, gap in ((5, 0, 0), (0, 3, 7), (5, 1, 2)):
        assert np.array_equal(tap(frames, boxes, 16, pad=pad, lead=lead, gap=gap), want), (pad, lead, gap)


def test_mixed_batch_of_five_frames():
    shapes = [(37, 53), (64, 64), (20, 24), (97, 131), (270, 480)]
    frames = [make_frame(h, w, 3, seed=40 + i) for i, (h, w) in enumerate(shapes)]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480)]
    got = tap(frames, boxes, 32, lead=1, gap=3)
    check_against_statement(got, frames, boxes, 32)
    for i in range(5):                                                 # each frame alone gives the same bytes as in the batch
        assert np.array_equal(tap([frames[i]], [boxes[i]], 32)[0], got[i])


def test_large_batch_of_small_frames_runs_tall_bands():
    """With 64 frames in a call nothing caps the band height: a workgroup owns as many output rows as the LDS holds."""
    frames = [make_frame(20 + i % 5, 24 + i % 7, 3, seed=100 + i) for i in range(64)]
    boxes = [None if i % 2 else (0.5, 1.0, 23.25, 19.0) for i in range(64)]
    got = tap(frames, boxes, 32)
    check_against_statement(got[::9], frames[::9], boxes[::9], 32)
    for i in (0, 7, 63):
        assert np.array_equal(tap([frames[i]], [boxes[i]], 32)[0], got[i])


# ---- the forward ---------------------------------------------------------------------------------------------------------------


def forward_frames_set(s):
    """Three frames of different sizes and boxes for a model of input size s."""
    frames = [make_frame(s + 16, s + 36, 3, seed=1), make_frame(s, s, 3, seed=2), make_frame(s // 2 + 5, s // 2 + 21, 3, seed=3)]
    boxes = [vithip.center_crop_box(s + 16, s + 36), None, (1.5, 0.0, s // 2 + 20.25, s // 2 + 5.0)]
    return frames, boxes


FORWARD_CASES = [(n, c, d) for n, c in (("vit_micro", S.CONFIGS["vit_micro"]), ("patch14_micro", PATCH14_MICRO))
                 for d in (vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8)]


@pytest.mark.parametrize("name,cfg,dtype", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d in FORWARD_CASES])
def test_forward_frames_equals_forward_u8_of_the_tap(name, cfg, dtype):
    s = cfg["image_size"]
    frames, boxes = forward_frames_set(s)
    resized = tap(frames, boxes, s)
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3)
    ctx.init_weights_seeded(17)
    want = ctx.forward_u8(resized)                       # the default norm
    got = ctx.forward_frames(frames, boxes)
    assert np.isfinite(want).all() and np.array_equal(got, want) and same_bits(got, want)
    ctx.set_input_norm(*vithip.input_norm_from_mean_std(IMAGENET_MEAN, IMAGENET_STD))
    want2 = ctx.forward_u8(resized)
    got2 = ctx.forward_frames(frames, boxes)
    assert np.isfinite(want2).all() and np.array_equal(got2, want2) and not np.array_equal(want2, want)
    # the default box is the whole frame
    assert np.array_equal(ctx.forward_frames(frames[1:2]), ctx.forward_u8(frames[1][None]))
    ctx.close()


@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    s = cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
    ctx.init_weights_seeded(17)
    ctx.set_input_norm(*vithip.input_norm_from_mean_std(IMAGENET_MEAN, IMAGENET_STD))
    frames, boxes = forward_frames_set(s)
    resized = tap(frames, boxes, s)
    ref = ctx.forward_u8(resized)                        # computed once; the tests below only read it
    for a in (resized, ref):
        a.setflags(write=False)
    yield ctx, cfg, frames, boxes, resized, ref
    ctx.close()


def test_device_entry_point_streams_and_graphs(micro):
    ctx, cfg, frames, boxes, resized, ref = micro
    buf, desc = lay_out(frames, boxes, pad=5, lead=3, gap=1)          # unaligned device frames
    din = vithip.DeviceBuffer.from_numpy(buf)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((3, cfg["classes"]), np.float32))
    ctx.forward_device_frames_u8(din.ptr, buf.nbytes, desc, dout.ptr)
    assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
    try:
        ctx.set_streams(2)                                             # the resize runs once, before the fork
        assert same_bits(ctx.forward_frames(frames, boxes), ref)
        ctx.forward_device_frames_u8(din.ptr, buf.nbytes, desc, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, (3, cfg["classes"])), ref)
    finally:
        ctx.set_streams(1)
    try:
        ctx.set_graph(True)
        for cached in (0, 1, 1):                                       # eager, captured, replayed
            assert same_bits(ctx.forward_frames(frames, boxes), ref)
            assert ctx.get_graph() == (True, cached)
        # other frames through the replayed graph: the resize in front of it is no part of the capture
        assert same_bits(ctx.forward_frames(frames[::-1], boxes[::-1]), ref[::-1])
        assert ctx.get_graph() == (True, 1)
    finally:
        ctx.set_graph(False)
    din.free(); dout.free()


def test_stage_timing_times_the_resize(micro):
    ctx, cfg, frames, boxes, resized, ref = micro
    try:
        ctx.set_stage_timing("resize")
        assert same_bits(ctx.forward_frames(frames, boxes), ref)
        avg, mn, n = ctx.get_stage_timing()
        assert n == 1 and avg > 0.0
    finally:
        ctx.set_stage_timing(None)


def test_frames_ring(micro):
    ctx, cfg, frames, boxes, resized, ref = micro
    picks = [[0, 1], [2], [1, 2, 0]]                                   # three submits with different batches
    slot_bytes = 1 << 16
    ctx.ring_create_frames(3, 3, slot_bytes)
    try:
        assert ctx.ring_free_slots() == 3
        # slot 0: filled in place
        buf, desc = lay_out([frames[i] for i in picks[0]], [boxes[i] for i in picks[0]], lead=1)
        view = ctx.ring_input_frames()
        assert view.dtype == np.uint8 and view.shape == (slot_bytes,)
        view[:buf.size] = buf
        ctx.ring_submit_frames_packed(None, buf.size, desc)
        desc[0].height = 0                                             # the descriptors were copied at the call
        ctx.ring_submit_frames([frames[i] for i in picks[1]], [boxes[i] for i in picks[1]])
        for call in (lambda: ctx.ring_submit(np.zeros((1, 64, 64, 3), np.float32)), lambda: ctx.ring_input(1),
                     lambda: ctx.ring_submit_u8(resized[:1]), lambda: ctx.ring_input_u8(1)):   # the other kinds' calls
            with pytest.raises(vithip.VhError) as e:
                call()
            assert e.value.code == VH_ERR_STATE
        ctx.ring_submit_frames([frames[i] for i in picks[2]], [boxes[i] for i in picks[2]])
        assert ctx.ring_free_slots() == 0
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames(frames[:1], boxes[:1])
        assert e.value.code == VH_ERR_RING_FULL
        for p in picks:                                                # FIFO
            assert same_bits(ctx.ring_collect(), ref[p])
        assert ctx.ring_free_slots() == 3
        # refusals leave the ring as it was: a bad box, more bytes than a slot holds, more frames than a slot's batch
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames(frames[:1], [(0.0, 0.0, 1000.0, 10.0)])
        assert e.value.code == VH_ERR_INVALID
        big = make_frame(200, 200, 3, seed=5)
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames([big])
        assert e.value.code == VH_ERR_INVALID
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_frames([frames[1]] * 4)
        assert e.value.code == VH_ERR_INVALID
        assert ctx.ring_free_slots() == 3
        ctx.ring_submit_frames(frames, boxes)
        assert same_bits(ctx.ring_collect(), ref)
        # the frames calls on the other two kinds of ring
        for u8 in (True, False):
            ctx.ring_create(2, 2, u8=u8)
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_submit_frames(frames[:1], boxes[:1])
            assert e.value.code == VH_ERR_STATE
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_input_frames()
            assert e.value.code == VH_ERR_STATE
        vithip.lib().vh_ring_destroy(ctx.h)
        # after vh_ring_destroy an fp32 ring on the same context still works
        ctx.ring_create(2, 2)
        scale, shift = ctx.get_input_norm()
        ctx.ring_submit(u8_reference(resized[:2], scale, shift))
        assert same_bits(ctx.ring_collect(), ref[:2])
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


def test_refusals_enqueue_nothing(micro):
    ctx, cfg, frames, boxes, resized, ref = micro
    f = frames[1]
    h, w, _ = f.shape
    bad_boxes = [(-1.0, 0.0, w, h), (0.0, 0.0, w + 0.5, h), (5.0, 0.0, 5.0, h), (0.0, 9.0, w, 3.0), (float("nan"), 0.0, w, h)]
    for box in bad_boxes:
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_frames([f], [box])
        assert e.value.code == VH_ERR_INVALID
    with pytest.raises(vithip.VhError) as e:                          # scale > 32: 64 * 32 = 2048 source rows at the most
        ctx.forward_frames([make_frame(2049, 64, 3, seed=6)])
    assert e.value.code == VH_ERR_INVALID
    buf, desc = lay_out(frames, boxes)
    out = np.zeros((3, cfg["classes"]), np.float32)
    L = vithip.lib()
    assert L.vh_forward_frames_u8(ctx.h, buf.ctypes.data, buf.nbytes - 1, C.addressof(desc), 3, out.ctypes.data) == VH_ERR_INVALID   # last byte beyond nbytes
    desc[2].row_stride -= 1
    assert L.vh_forward_frames_u8(ctx.h, buf.ctypes.data, buf.nbytes, C.addressof(desc), 3, out.ctypes.data) == VH_ERR_INVALID
    desc[2].row_stride += 1
    desc[0].width = 8193
    assert L.vh_forward_frames_u8(ctx.h, buf.ctypes.data, buf.nbytes, C.addressof(desc), 3, out.ctypes.data) == VH_ERR_INVALID
    assert L.vh_forward_frames_u8(ctx.h, buf.ctypes.data, buf.nbytes, C.addressof(desc), 4, out.ctypes.data) == VH_ERR_INVALID       # batch > max_batch
    assert L.vh_forward_frames_u8(ctx.h, buf.ctypes.data, buf.nbytes, None, 3, out.ctypes.data) == VH_ERR_INVALID
    assert not out.any()                                               # nothing ran
    assert same_bits(ctx.forward_frames(frames, boxes), ref)           # and a following valid forward is right
