"""CPU suite of the frames entry points (include/vithip.h, "8-bit frames"): the host half of the contract.

vh_resize_table returns the table the kernel gets; frames_ref states the same table in numpy float64, and torch's antialiased
bilinear on the CPU is the filter both claim to be.  Every refusal of the contract is decided on the host before any device call,
so it is checked here through the operator tap with a pointer that is never dereferenced.  The VH_ERR_STATE answers across ring
kinds need a context, and a context needs a device: they are in test_gpu_frames.py."""
import ctypes as C

import numpy as np
import pytest

import frames_ref as R
import vithip

VH_ERR_INVALID = 1

# (n_in, lo, hi, n_out)
TABLE_CASES = [
    (53, 0.0, 53.0, 16),          # non-integer down-scale
    (37, 0.0, 37.0, 16),
    (480, 0.0, 480.0, 32),        # scale 15: 29 or 30 taps a row
    (20, 0.0, 20.0, 32),          # up-scale: two taps
    (24, 0.0, 24.0, 32),          # up-scale with exact ties
    (64, 0.0, 64.0, 64),          # identity: one tap of weight 1
    (131, 10.25, 101.75, 28),     # fractional box
    (97, 5.5, 96.0, 28),
    (100, 0.0, 37.5, 16),         # boxes that touch the frame's edges
    (100, 37.5, 100.0, 16),
    (256, 16.0, 240.0, 224),      # the 0.875 centre box of a 256 frame: scale exactly 1
    (2048, 0.0, 2048.0, 64),      # scale = 32: 64 or 65 taps
    (8192, 0.0, 8192.0, 256),
    (1080, 0.0, 1080.0, 224),
]


@pytest.mark.parametrize("n,lo,hi,s", TABLE_CASES, ids=lambda v: str(v))
def test_resize_table_equals_the_numpy_statement(n, lo, hi, s):
    first, count, weights = vithip.resize_table(n, lo, hi, s, R.MAX_TAPS)
    rf, rc, rw = R.axis_table(n, lo, hi, s)
    assert np.array_equal(first, rf) and np.array_equal(count, rc)
    assert np.array_equal(weights.view(np.uint32), rw.view(np.uint32))   # equal after the one fp32 rounding
    assert (count >= 1).all() and (first >= 0).all() and (first + count <= n).all() and count.max() <= R.MAX_TAPS
    for i in range(s):
        assert (weights[i, :count[i]] > 0).all() and not weights[i, count[i]:].any()
    # a row of at most 65 weights, each within half an fp32 ulp (<= 2^-25) of its double: the sum is within 65 * 2^-24 of 1
    assert np.abs(weights.astype(np.float64).sum(axis=1) - 1.0).max() <= 65 * 2.0 ** -24
    if (n, lo, hi) == (64, 0.0, 64.0) or (n, lo, hi) == (256, 16.0, 240.0):
        assert (count == 1).all() and (weights[:, 0] == 1.0).all() and np.array_equal(first, np.arange(s) + int(lo))
    # a narrower row stride holds the same table, as long as every row fits
    k = int(count.max())
    f2, c2, w2 = vithip.resize_table(n, lo, hi, s, k)
    assert np.array_equal(f2, first) and np.array_equal(c2, count) and np.array_equal(w2, weights[:, :k])


def test_tap_counts_at_the_limits():
    _, count, _ = vithip.resize_table(2048, 0.0, 2048.0, 64)
    assert count.max() <= 65 and count.min() >= 33      # interior rows 64 or 65 taps; the two edge rows lose half
    _, count, _ = vithip.resize_table(480, 0.0, 480.0, 32)
    assert count.max() in (29, 30)
    _, count, _ = vithip.resize_table(20, 0.0, 20.0, 32)
    assert count.max() == 2


@pytest.mark.parametrize("h,w,s", [(37, 53, 16), (270, 480, 32), (64, 64, 64), (20, 24, 32)], ids=lambda v: str(v))
def test_statement_is_torch_antialiased_bilinear(h, w, s):
    import torch
    rng = np.random.default_rng(h * 1000 + w)
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = R.resize_f64(frame, None, s)
    t = torch.from_numpy(frame.astype(np.float32)).permute(2, 0, 1)[None]
    want = torch.nn.functional.interpolate(t, size=(s, s), mode="bilinear", antialias=True, align_corners=False)
    want = want[0].permute(1, 2, 0).numpy().astype(np.float64)
    diff = float(np.abs(got - want).max())
    print(f"frames_ref vs torch {h}x{w}->{s}: max |d| = {diff:.3e}")
    assert diff <= 1e-4
    if (h, w, s) == (64, 64, 64):
        assert np.array_equal(got, frame.astype(np.float64))


def test_resize_table_refusals():
    L = vithip.lib()
    first, count = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    weights = (C.c_float * (64 * 65))()

    def rc(n, lo, hi, s, taps=65, f=first, c=count, w=weights):
        return L.vh_resize_table(n, lo, hi, s, f, c, w, taps)

    assert rc(53, 0.0, 53.0, 16) == 0
    for bad in ((53, -0.5, 53.0, 16), (53, 0.0, 53.5, 16), (53, 20.0, 20.0, 16), (53, 30.0, 20.0, 16),
                (53, float("nan"), 53.0, 16), (53, 0.0, float("nan"), 16), (53, 0.0, float("inf"), 16),
                (0, 0.0, 1.0, 16), (8193, 0.0, 8193.0, 64), (53, 0.0, 53.0, 0),
                (2049, 0.0, 2049.0, 64)):                # scale 32.02
        assert rc(*bad) == VH_ERR_INVALID, bad
    assert rc(2048, 0.0, 2048.0, 64) == 0                # scale exactly 32
    assert rc(480, 0.0, 480.0, 32, taps=28) == VH_ERR_INVALID   # a row needs 29 taps or more
    assert rc(53, 0.0, 53.0, 16, f=None) == VH_ERR_INVALID
    assert rc(53, 0.0, 53.0, 16, w=None) == VH_ERR_INVALID
    assert rc(53, 0.0, 53.0, 16, taps=0) == VH_ERR_INVALID


def one_frame(h=40, w=60, stride=None, offset=0, box=None, ch=3):
    d = (vithip.Frame * 1)()
    d[0].offset, d[0].height, d[0].width = offset, h, w
    d[0].row_stride = w * ch if stride is None else stride
    d[0].box[:] = (0.0, 0.0, float(w), float(h)) if box is None else box
    return d


def test_every_refusal_of_the_contract_is_decided_on_the_host():
    """vh_op_resize_u8 checks and plans before its first device call: with a bad descriptor it returns VH_ERR_INVALID whether or
    not a device exists, and never reads the pointers (0x1000 here)."""
    L = vithip.lib()
    fake, big = C.c_void_p(0x1000), 1 << 30

    def rc(d, nbytes=big, ch=3, s=16, batch=1):
        return L.vh_op_resize_u8(fake, nbytes, C.addressof(d), batch, ch, s, fake, None)

    bad = [one_frame(h=0), one_frame(w=0), one_frame(h=8193), one_frame(w=8193), one_frame(h=-3),
           one_frame(stride=60 * 3 - 1), one_frame(stride=0), one_frame(stride=-180),
           one_frame(box=(-0.25, 0.0, 60.0, 40.0)), one_frame(box=(0.0, -1.0, 60.0, 40.0)),       # outside the frame
           one_frame(box=(0.0, 0.0, 60.5, 40.0)), one_frame(box=(0.0, 0.0, 60.0, 40.25)),
           one_frame(box=(30.0, 0.0, 30.0, 40.0)), one_frame(box=(0.0, 25.0, 60.0, 20.0)),       # empty
           one_frame(box=(float("nan"), 0.0, 60.0, 40.0)), one_frame(box=(0.0, 0.0, 60.0, float("nan"))),
           one_frame(h=513, w=60), one_frame(h=40, w=520)]                                       # scale > 32 in y, in x
    for d in bad:
        assert rc(d) == VH_ERR_INVALID, (d[0].height, d[0].width, d[0].row_stride, list(d[0].box))
        assert b"resize" in L.vh_last_error(None)
    # a frame whose last byte lies beyond nbytes: 40 rows of 180 bytes at offset 7 end at byte 7207
    assert rc(one_frame(offset=7), nbytes=7206) == VH_ERR_INVALID
    assert rc(one_frame(offset=7300), nbytes=7250) == VH_ERR_INVALID
    assert rc(one_frame(offset=2 ** 64 - 8), nbytes=big) == VH_ERR_INVALID           # no wrap-around
    assert rc(one_frame(stride=185), nbytes=39 * 185 + 179) == VH_ERR_INVALID        # the last row is not padded: 39 * 185 + 180
    # the second frame of a batch is checked like the first
    two = (vithip.Frame * 2)()
    for i, f in enumerate((one_frame(), one_frame(box=(0.0, 0.0, 61.0, 40.0)))):
        C.memmove(C.addressof(two[i]), C.addressof(f[0]), C.sizeof(vithip.Frame))
    assert rc(two, batch=2) == VH_ERR_INVALID
    # arguments of the tap itself
    ok = one_frame()
    assert rc(ok, batch=0) == VH_ERR_INVALID and rc(ok, ch=0) == VH_ERR_INVALID and rc(ok, ch=65) == VH_ERR_INVALID
    assert rc(ok, s=0) == VH_ERR_INVALID and rc(ok, s=4097) == VH_ERR_INVALID
    assert L.vh_op_resize_u8(None, big, C.addressof(ok), 1, 3, 16, fake, None) == VH_ERR_INVALID
    assert L.vh_op_resize_u8(fake, big, None, 1, 3, 16, fake, None) == VH_ERR_INVALID
    assert L.vh_op_resize_u8(fake, big, C.addressof(ok), 1, 3, 16, None, None) == VH_ERR_INVALID


def test_frames_calls_without_a_context_are_refused():
    L = vithip.lib()
    d, buf, out = one_frame(), (C.c_uint8 * 16)(), (C.c_float * 16)()
    p, cap = C.POINTER(C.c_uint8)(), C.c_size_t(0)
    assert L.vh_forward_frames_u8(None, buf, 16, C.addressof(d), 1, out) == VH_ERR_INVALID
    assert L.vh_forward_device_frames_u8(None, buf, 16, C.addressof(d), 1, out) == VH_ERR_INVALID
    assert L.vh_ring_create_frames(None, 2, 1, 1024) == VH_ERR_INVALID
    assert L.vh_ring_input_frames(None, C.byref(p), C.byref(cap)) == VH_ERR_INVALID
    assert L.vh_ring_submit_frames(None, buf, 16, C.addressof(d), 1) == VH_ERR_INVALID


def test_stage_names_keep_their_indices():
    L = vithip.lib()
    for i, name in enumerate(vithip.STAGES):
        assert L.vh_stage_name(i) == name.encode()
    assert L.vh_stage_name(len(vithip.STAGES)) == b"resize" and vithip.TIMED_STAGES[-1] == vithip.STAGE_RESIZE == "resize"
    assert L.vh_stage_name(len(vithip.TIMED_STAGES)) == b""


def test_center_crop_box():
    assert vithip.center_crop_box(256, 256) == (16.0, 16.0, 240.0, 240.0)
    assert vithip.center_crop_box(360, 480) == (82.5, 22.5, 397.5, 337.5)
    assert vithip.center_crop_box(480, 360) == (22.5, 82.5, 337.5, 397.5)
    assert vithip.center_crop_box(100, 300, 1.0) == (100.0, 0.0, 200.0, 100.0)
    x0, y0, x1, y1 = vithip.center_crop_box(1080, 1920)
    assert x1 - x0 == y1 - y0 == 945.0 and x0 + x1 == 1920.0 and y0 + y1 == 1080.0
    for bad in ((0, 5, 0.875), (5, 5, 0.0), (5, 5, 1.5)):
        with pytest.raises(ValueError):
            vithip.center_crop_box(*bad)


def test_pack_frames():
    a = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    b = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)[:, ::-1]      # not contiguous
    buf, desc = vithip.pack_frames([a, b], [None, (0.5, 1.0, 4.0, 3.5)], channels=3)
    assert buf.dtype == np.uint8 and buf.size == a.size + b.size and len(desc) == 2
    assert (desc[0].offset, desc[0].height, desc[0].width, desc[0].row_stride, list(desc[0].box)) == (0, 2, 3, 9, [0.0, 0.0, 3.0, 2.0])
    assert (desc[1].offset, desc[1].height, desc[1].width, desc[1].row_stride, list(desc[1].box)) == (18, 4, 5, 15, [0.5, 1.0, 4.0, 3.5])
    assert np.array_equal(buf[18:].reshape(4, 5, 3), b)
    with pytest.raises(ValueError):
        vithip.pack_frames([a], channels=1)
    with pytest.raises(TypeError):
        vithip.pack_frames([a.astype(np.float32)])
