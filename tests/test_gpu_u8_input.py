"""GPU suite of the 8-bit input path.  The contract (include/vithip.h, "8-bit images"): pixel p of channel c enters the
model as fmaf((float)p, scale[c], shift[c]) with one rounding and is then rounded to the MFMA operand type as an fp32 input
is.  So the patch matrix, and with it every logit, has the BITS the fp32 entry point gives for that host-computed array
(test_u8_input.u8_reference): every comparison below is equality, no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import vh_synth as S
import vithip
from tensor_ref import make_u8_images, u8_reference
from test_u8_input import DEFAULT_SCALE, IMAGENET_MEAN, IMAGENET_STD, gather_patches
from vh_testlib import same_bits

pytestmark = pytest.mark.gpu

BATCH = 3
SENTINEL = 0xA5C3
DTYPES16 = [vithip.DTYPE_BF16, vithip.DTYPE_FP16]
DTNAME = {vithip.DTYPE_BF16: "bf16", vithip.DTYPE_FP16: "fp16", vithip.DTYPE_FP8: "fp8"}

PATCH14_MICRO = dict(image_size=28, patch_size=14, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=8)
# dim and mlp_dim multiples of 256: the one shape here whose LayerNorms fold (split residual, PATCH_SPLIT epilogue, class-token tail)
FOLD_MICRO = dict(image_size=32, patch_size=16, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=8)


def norm_for(channels):
    """Per-channel constants inside u8_reference's precondition: ImageNet for 3 channels, distinct values otherwise."""
    if channels == 3:
        return vithip.input_norm_from_mean_std(IMAGENET_MEAN, IMAGENET_STD)
    mean = [0.45 + 0.02 * c for c in range(channels)]
    std = [0.225 + 0.01 * c for c in range(channels)]
    return vithip.input_norm_from_mean_std(mean, std)


# ---- 1. the operator, bit for bit ---------------------------------------------------------------------------------------
OP_SHAPES = [(32, 16, 3, 768),    # aligned 8-byte loads, no padding
             (28, 14, 3, 640),    # byte loads (28 * 28 * 3 = 2352 B rows of 84 B; 14 * 3 = 42 is no multiple of 8), zero padding
             (64, 32, 1, 1024),   # one channel, 8-byte loads
             (12, 4, 5, 128)]     # an 8-element chunk straddles patch rows and the channel order; 80 real columns of 128


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: DTNAME[d])
@pytest.mark.parametrize("image,patch,ch,kpad", OP_SHAPES, ids=lambda v: str(v))
def test_op_im2col_u8_is_bit_exact(image, patch, ch, kpad, dtype):
    u8 = make_u8_images(BATCH, image, ch, seed=image + ch)
    scale, shift = norm_for(ch)
    want = vithip.to16(gather_patches(u8_reference(u8, scale, shift), patch, kpad), dtype)
    rows, kp, tail = want.shape[0], patch * patch * ch, 512
    din = vithip.DeviceBuffer.from_numpy(u8)
    dout = vithip.DeviceBuffer.from_numpy(np.full(rows * kpad + tail, SENTINEL, dtype=np.uint16))
    vithip.op_im2col_u8(din.ptr, BATCH, image, patch, ch, kpad, scale, shift, dout.ptr, dtype)
    raw = dout.to_numpy(np.uint16, (rows * kpad + tail,))
    got = raw[:rows * kpad].reshape(rows, kpad)
    assert np.array_equal(got[:, :kp], want[:, :kp])
    assert not got[:, kp:].any()                         # the padding columns are written, as zeros
    assert (raw[rows * kpad:] == SENTINEL).all()         # and nothing behind the matrix is
    # the same matrix from the fp32 kernel fed the reference array: the statement the forward tests rest on
    dref = vithip.DeviceBuffer.from_numpy(u8_reference(u8, scale, shift))
    dout2 = vithip.DeviceBuffer(rows * kpad * 2)
    vithip.op_im2col_padded(dref.ptr, BATCH, image, patch, ch, kpad, dout2.ptr, dtype)
    assert np.array_equal(dout2.to_numpy(np.uint16, (rows, kpad)), got)
    for b in (din, dout, dref, dout2):
        b.free()


# ---- 2. forward_u8 == forward(reference array), bitwise -------------------------------------------------------------------
ALL3 = [vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8]
FORWARD_CASES = (
    [("vit_micro", S.CONFIGS["vit_micro"], d, 0) for d in ALL3]
    # vit_gray's mlp_dim (320) is no multiple of 128, which VH_DTYPE_FP8 needs: that context cannot be created
    + [("vit_gray", S.CONFIGS["vit_gray"], d, 0) for d in DTYPES16]
    + [("patch14_micro", PATCH14_MICRO, d, 0) for d in ALL3]
    + [("vit_micro_clip", S.CONFIGS["vit_micro"], d, vithip.FLAG_PRE_LN | vithip.FLAG_QUICK_GELU) for d in ALL3]
    + [("vit_micro_fold_off", S.CONFIGS["vit_micro"], d, vithip.FLAG_LN_FOLD_OFF) for d in ALL3]
    + [("fold_micro_on", FOLD_MICRO, d, vithip.FLAG_LN_FOLD_ON) for d in ALL3]
    + [("fold_micro_cls_tail", FOLD_MICRO, d, vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL) for d in DTYPES16])


@pytest.mark.parametrize("name,cfg,dtype,flags", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d, _ in FORWARD_CASES])
def test_forward_u8_equals_fp32_forward_bitwise(name, cfg, dtype, flags):
    ch = cfg["channels"]
    u8 = make_u8_images(BATCH, cfg["image_size"], ch, seed=5)
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=BATCH, flags=flags)
    ctx.init_weights_seeded(17)
    if name.startswith("fold_micro"):
        assert ctx.ln_fold()
    # the default norm, no set_input_norm call: x = p * float32(1 / 255)
    sc, sh = ctx.get_input_norm()
    assert np.array_equal(sc, np.full(ch, DEFAULT_SCALE)) and not sh.any()
    ref = ctx.forward(u8_reference(u8, np.full(ch, DEFAULT_SCALE), np.zeros(ch, np.float32)))
    got = ctx.forward_u8(u8)
    assert np.isfinite(ref).all() and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # per-channel mean / std
    scale, shift = norm_for(ch)
    ctx.set_input_norm(scale, shift)
    sc, sh = ctx.get_input_norm()
    assert np.array_equal(sc, scale) and np.array_equal(sh, shift)
    ref2 = ctx.forward(u8_reference(u8, scale, shift))
    got2 = ctx.forward_u8(u8)
    assert np.isfinite(ref2).all() and np.array_equal(got2.view(np.uint32), ref2.view(np.uint32))
    assert not np.array_equal(ref, ref2)   # the constants reach the model
    # NULL, NULL restores the default
    ctx.set_input_norm()
    assert np.array_equal(ctx.forward_u8(u8).view(np.uint32), ref.view(np.uint32))
    ctx.close()


# ---- shared: vit_micro bf16 with the ImageNet constants, its images and its fp32-path logits --------------------------------
@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=BATCH)
    ctx.init_weights_seeded(17)
    scale, shift = norm_for(3)
    ctx.set_input_norm(scale, shift)
    u8 = make_u8_images(BATCH, cfg["image_size"], 3, seed=9)
    ref = ctx.forward(u8_reference(u8, scale, shift))   # computed once; the tests below only read it
    ref.setflags(write=False)
    yield ctx, cfg, u8, ref
    ctx.close()


# ---- 3. device entry points and streams -------------------------------------------------------------------------------------
def test_device_entry_points_and_streams(micro):
    ctx, cfg, u8, ref = micro
    din = vithip.DeviceBuffer.from_numpy(u8)
    dout = vithip.DeviceBuffer.from_numpy(np.zeros((BATCH, cfg["classes"]), np.float32))
    shape = (BATCH, cfg["classes"])
    ctx.forward_device_u8(din.ptr, BATCH, dout.ptr)
    assert same_bits(dout.to_numpy(np.float32, shape), ref)
    vithip.lib().vh_memcpy_h2d(0, dout.ptr, np.zeros(shape, np.float32).ctypes.data, BATCH * cfg["classes"] * 4)
    ctx.forward_device_u8_async(din.ptr, BATCH, dout.ptr, steps=2)
    ctx.synchronize()
    assert same_bits(dout.to_numpy(np.float32, shape), ref)
    try:
        ctx.set_streams(2)   # parts of 2 and 1 images: the second part's pointer advances by BYTES
        vithip.lib().vh_memcpy_h2d(0, dout.ptr, np.zeros(shape, np.float32).ctypes.data, BATCH * cfg["classes"] * 4)
        ctx.forward_device_u8(din.ptr, BATCH, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, shape), ref)
        assert same_bits(ctx.forward_u8(u8), ref)
    finally:
        ctx.set_streams(1)
    din.free(); dout.free()


# ---- 4. graphs ---------------------------------------------------------------------------------------------------------------
def test_graph_cache_keys_on_the_input_kind_and_drops_on_a_norm_change():
    cfg = S.CONFIGS["vit_micro"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=BATCH)
    ctx.init_weights_seeded(17)
    scale, shift = norm_for(3)
    ctx.set_input_norm(scale, shift)
    u8 = make_u8_images(BATCH, cfg["image_size"], 3, seed=9)
    x = u8_reference(u8, scale, shift)
    ref = ctx.forward(x)                      # eager, before graphs are on
    ctx.set_graph(True)
    assert same_bits(ctx.forward_u8(u8), ref)   # first forward at this batch: eager
    assert ctx.get_graph() == (True, 0)
    assert same_bits(ctx.forward_u8(u8), ref)   # captured and launched
    assert ctx.get_graph() == (True, 1)
    assert same_bits(ctx.forward_u8(u8), ref)   # replayed
    assert ctx.get_graph() == (True, 1)
    # the fp32 forward stages into the same device buffer and writes the same logits buffer at the same batch: only the input
    # kind tells the two launch sequences apart
    assert same_bits(ctx.forward(x), ref)
    assert ctx.get_graph() == (True, 2)
    assert same_bits(ctx.forward_u8(u8), ref) and ctx.get_graph() == (True, 2)
    # other constants: the cached graphs hold the old ones by value and must go
    scale2, shift2 = np.float32([0.0078125, 0.0068359375, 0.0087890625]), np.float32([-1.0, -0.875, -1.125])
    ctx.set_input_norm(scale2, shift2)
    assert ctx.get_graph() == (True, 0)
    ref2 = u8_reference(u8, scale2, shift2)
    got2 = ctx.forward_u8(u8)
    assert ctx.get_graph() == (True, 1)
    ctx.set_graph(False)
    want2 = ctx.forward(ref2)
    assert same_bits(got2, want2) and not same_bits(want2, ref)
    ctx.close()


# ---- 5. the ring ---------------------------------------------------------------------------------------------------------------
def test_u8_ring(micro):
    ctx, cfg, u8, ref = micro
    VH_ERR_STATE, VH_ERR_RING_FULL = 3, 6
    batches = [u8[0:2], u8[2:3], u8[1:3]]
    want = [ref[0:2], ref[2:3], ref[1:3]]
    ctx.ring_create_u8(3, 2)
    try:
        assert ctx.ring_free_slots() == 3
        view = ctx.ring_input_u8(2)
        assert view.dtype == np.uint8 and view.shape == (2, 64, 64, 3)
        view[...] = batches[0]
        ctx.ring_submit_u8(batch=2)            # filled in place
        ctx.ring_submit_u8(batches[1])         # by pointer
        with pytest.raises(vithip.VhError) as e:   # the fp32 calls on a u8 ring
            ctx.ring_submit(np.zeros((1, 64, 64, 3), np.float32))
        assert e.value.code == VH_ERR_STATE
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_input(1)
        assert e.value.code == VH_ERR_STATE
        ctx.ring_submit_u8(batches[2])
        assert ctx.ring_free_slots() == 0
        with pytest.raises(vithip.VhError) as e:   # a fourth submit before any collect
            ctx.ring_submit_u8(batches[1])
        assert e.value.code == VH_ERR_RING_FULL
        for w in want:                             # FIFO
            assert same_bits(ctx.ring_collect(), w)
        assert ctx.ring_free_slots() == 3
        for b, w in zip(batches, want):            # and each equals forward_u8 of the same images
            assert same_bits(ctx.forward_u8(b), w)
        # the u8 calls on an fp32 ring
        ctx.ring_create(2, 2)
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_submit_u8(batches[1])
        assert e.value.code == VH_ERR_STATE
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_input_u8(1)
        assert e.value.code == VH_ERR_STATE
        scale, shift = ctx.get_input_norm()
        ctx.ring_submit(u8_reference(batches[1], scale, shift))
        assert same_bits(ctx.ring_collect(), want[1])
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


# ---- 6. argument checks --------------------------------------------------------------------------------------------------------
def test_argument_checks(micro):
    ctx, cfg, u8, ref = micro
    VH_ERR_INVALID = 1
    L = vithip.lib()
    din = vithip.DeviceBuffer(u8.nbytes + 64)
    dout = vithip.DeviceBuffer(BATCH * cfg["classes"] * 4)
    col = vithip.DeviceBuffer(BATCH * 16 * 768 * 2)
    scale, shift = ctx.get_input_norm()
    for off in (1, 8):   # a device input pointer that is not 16-byte aligned
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_u8(din.ptr + off, BATCH, dout.ptr)
        assert e.value.code == VH_ERR_INVALID
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_u8_async(din.ptr + off, BATCH, dout.ptr, steps=1)
        assert e.value.code == VH_ERR_INVALID
        with pytest.raises(vithip.VhError) as e:
            vithip.op_im2col_u8(din.ptr + off, BATCH, 64, 16, 3, 768, scale, shift, col.ptr, vithip.DTYPE_BF16)
        assert e.value.code == VH_ERR_INVALID
    for bad in (np.nan, np.inf):   # a non-finite constant
        s2 = scale.copy(); s2[1] = bad
        with pytest.raises(vithip.VhError) as e:
            ctx.set_input_norm(s2, shift)
        assert e.value.code == VH_ERR_INVALID
        with pytest.raises(vithip.VhError) as e:
            ctx.set_input_norm(scale, s2)
        assert e.value.code == VH_ERR_INVALID
        with pytest.raises(vithip.VhError) as e:
            vithip.op_im2col_u8(din.ptr, BATCH, 64, 16, 3, 768, s2, shift, col.ptr, vithip.DTYPE_BF16)
        assert e.value.code == VH_ERR_INVALID
    three = (C.c_float * 3)(0.5, 0.5, 0.5)   # only one of the two given
    assert L.vh_set_input_norm(ctx.h, three, None) == VH_ERR_INVALID
    assert L.vh_set_input_norm(ctx.h, None, three) == VH_ERR_INVALID
    with pytest.raises(vithip.VhError) as e:
        ctx.set_input_norm(scale, None)
    assert e.value.code == VH_ERR_INVALID
    with pytest.raises(vithip.VhError) as e:   # fp8 is no patch-matrix type
        vithip.op_im2col_u8(din.ptr, BATCH, 64, 16, 3, 768, scale, shift, col.ptr, vithip.DTYPE_FP8)
    assert e.value.code == VH_ERR_INVALID
    # none of the refused calls changed the constants or the results
    sc, sh = ctx.get_input_norm()
    assert np.array_equal(sc, scale) and np.array_equal(sh, shift)
    assert same_bits(ctx.forward_u8(u8), ref)
    for b in (din, dout, col):
        b.free()
