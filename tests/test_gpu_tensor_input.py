"""GPU suite of the image-tensor input path.  The contract (include/vithip.h, "Image tensors"): element (b, y, x, c) of a dense
tensor of one element type in one layout enters the model as the fp32 value v (itself, exactly widened, or the u8 fma) and is then
rounded to the MFMA operand type as an fp32 input is.  So the patch matrix, and with it every logit, has the BITS the fp32 entry
point gives for the NHWC fp32 array of v (tensor_ref.tensor_reference): every comparison below is equality, no tolerance anywhere."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import tensor_ref as R
import vh_synth as S
import vithip
from test_gpu_u8_input import FORWARD_CASES, OP_SHAPES, norm_for
from test_u8_input import DEFAULT_SCALE, gather_patches
from vh_testlib import same_bits

pytestmark = pytest.mark.gpu

BATCH = 3
SENTINEL = 0xA5C3
DTYPES16 = [vithip.DTYPE_BF16, vithip.DTYPE_FP16]
DTNAME = {vithip.DTYPE_BF16: "bf16", vithip.DTYPE_FP16: "fp16", vithip.DTYPE_FP8: "fp8"}
KINDS = [(e, l) for l in R.LAYOUTS for e in R.ELEMS]                      # all 8 (elem, layout) pairs
KIND_ID = [f"{R.ELEM_NAME[e]}-{R.LAYOUT_NAME[l]}" for e, l in KINDS]
VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_RING_FULL, VH_ERR_RING_EMPTY = 1, 3, 6, 7


# ---- 1. the operator, bit for bit -------------------------------------------------------------------------------------------------
# OP_SHAPES (the u8 suite's): (32, 16, 3, 768) vector path, no padding | (28, 14, 3, 640) unaligned plane rows, padding |
# (64, 32, 1, 1024) one channel | (12, 4, 5, 128) a chunk straddles patch rows and channels
@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: DTNAME[d])
@pytest.mark.parametrize("image,patch,ch,kpad", OP_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("elem,layout", KINDS, ids=KIND_ID)
def test_op_im2col_tensor_is_bit_exact(elem, layout, image, patch, ch, kpad, dtype):
    nhwc = R.make_tensor(elem, BATCH, image, ch, seed=image + ch)           # float kinds: with the infinities and the largest finite value
    scale, shift = norm_for(ch)
    ref = R.tensor_reference(nhwc, elem, vithip.LAYOUT_NHWC, scale, shift)
    with np.errstate(over="ignore"):                                       # the fp16 operand type overflows to inf, as the kernel does
        want = vithip.to16(gather_patches(ref, patch, kpad), dtype)
    rows, kp, tail = want.shape[0], patch * patch * ch, 512
    din = vithip.DeviceBuffer.from_numpy(R.to_layout(nhwc, layout))
    dout = vithip.DeviceBuffer.from_numpy(np.full(rows * kpad + tail, SENTINEL, dtype=np.uint16))
    vithip.op_im2col_tensor(din.ptr, elem, layout, BATCH, image, patch, ch, kpad, dout.ptr, dtype, scale, shift)
    raw = dout.to_numpy(np.uint16, (rows * kpad + tail,))
    got = raw[:rows * kpad].reshape(rows, kpad)
    assert np.array_equal(got[:, :kp], want[:, :kp])
    assert not got[:, kp:].any()                         # the padding columns are written, as zeros
    assert (raw[rows * kpad:] == SENTINEL).all()         # and nothing behind the matrix is
    # the same matrix from the fp32 kernel fed the reference array: the statement the forward tests rest on
    dref = vithip.DeviceBuffer.from_numpy(ref)
    dout2 = vithip.DeviceBuffer(rows * kpad * 2)
    vithip.op_im2col_padded(dref.ptr, BATCH, image, patch, ch, kpad, dout2.ptr, dtype)
    assert np.array_equal(dout2.to_numpy(np.uint16, (rows, kpad)), got)
    for b in (din, dout, dref, dout2):
        b.free()


@pytest.mark.parametrize("elem,layout", [k for k in KINDS if k[0] != vithip.ELEM_U8], ids=[i for i, k in zip(KIND_ID, KINDS) if k[0] != vithip.ELEM_U8])
def test_nan_positions_survive(elem, layout):
    """A NaN's payload is no part of the contract; that a NaN element gives a NaN operand, and no other element does, is."""
    image, patch, ch, kpad = 28, 14, 3, 640
    nhwc = R.make_tensor(elem, BATCH, image, ch, seed=2, extremes=False)
    nan_bits = {vithip.ELEM_F32: 0x7FC00001, vithip.ELEM_F16: 0x7E01, vithip.ELEM_BF16: 0x7FC1}[elem]
    bits = nhwc.view({4: np.uint32, 2: np.uint16}[nhwc.dtype.itemsize]).reshape(-1)
    where = np.array([0, 5, 1000, bits.size - 1])
    bits[where] = nan_bits
    ref = R.widen(nhwc, elem)
    assert np.isnan(ref).sum() == len(where)
    want_nan = np.isnan(gather_patches(ref, patch, kpad))
    din = vithip.DeviceBuffer.from_numpy(R.to_layout(nhwc, layout))
    rows = want_nan.shape[0]
    dout = vithip.DeviceBuffer(rows * kpad * 2)
    vithip.op_im2col_tensor(din.ptr, elem, layout, BATCH, image, patch, ch, kpad, dout.ptr, vithip.DTYPE_BF16)
    got = vithip.from16(dout.to_numpy(np.uint16, (rows, kpad)), vithip.DTYPE_BF16)
    assert np.array_equal(np.isnan(got), want_nan)
    din.free(); dout.free()


# ---- 2. forward_tensor == forward(reference array), bitwise ------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,dtype,flags", FORWARD_CASES, ids=[f"{n}-{DTNAME[d]}" for n, _, d, _ in FORWARD_CASES])
def test_forward_tensor_equals_fp32_forward_bitwise(name, cfg, dtype, flags):
    ch, image = cfg["channels"], cfg["image_size"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=BATCH, flags=flags)
    ctx.init_weights_seeded(17)
    if name.startswith("fold_micro"):
        assert ctx.ln_fold()
    default = (np.full(ch, DEFAULT_SCALE), np.zeros(ch, np.float32))
    refs = {}
    for elem in R.ELEMS:
        nhwc = R.make_tensor(elem, BATCH, image, ch, seed=5 + elem, extremes=False)
        norms = [default, norm_for(ch)] if elem == vithip.ELEM_U8 else [default]   # u8: the default and an ImageNet-style norm
        for i, (scale, shift) in enumerate(norms):
            if i:
                ctx.set_input_norm(scale, shift)
            ref = ctx.forward(R.tensor_reference(nhwc, elem, vithip.LAYOUT_NHWC, scale, shift))   # one reference for both layouts
            assert np.isfinite(ref).all()
            refs[(elem, i)] = ref
            for layout in R.LAYOUTS:
                got = ctx.forward_tensor(R.to_layout(nhwc, layout), layout, elem)
                assert same_bits(got, ref), (R.ELEM_NAME[elem], R.LAYOUT_NAME[layout], i)
        ctx.set_input_norm()
    assert not same_bits(refs[(vithip.ELEM_U8, 0)], refs[(vithip.ELEM_U8, 1)])   # the constants reach the model
    assert not same_bits(refs[(vithip.ELEM_F32, 0)], refs[(vithip.ELEM_F16, 0)])  # and the inputs differ per element type
    ctx.close()


# ---- shared: vit_micro bf16 with the ImageNet constants; per element type its images and fp32-path logits ---------------------------
@pytest.fixture(scope="module")
def micro():
    cfg = S.CONFIGS["vit_micro"]
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=BATCH)
    ctx.init_weights_seeded(17)
    scale, shift = norm_for(3)
    ctx.set_input_norm(scale, shift)
    data = {}
    for elem in R.ELEMS:
        nhwc = R.make_tensor(elem, BATCH, cfg["image_size"], 3, seed=9 + elem, extremes=False)
        ref = ctx.forward(R.tensor_reference(nhwc, elem, vithip.LAYOUT_NHWC, scale, shift))   # computed once; the tests only read it
        assert np.isfinite(ref).all()
        ref.setflags(write=False)
        data[elem] = (nhwc, ref)
    yield ctx, cfg, data
    ctx.close()


# ---- 3. device entry points, streams, graphs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,layout", KINDS, ids=KIND_ID)
def test_device_entry_points_and_streams(micro, elem, layout):
    ctx, cfg, data = micro
    nhwc, ref = data[elem]
    shape = (BATCH, cfg["classes"])
    din = vithip.DeviceBuffer.from_numpy(R.to_layout(nhwc, layout))
    dout = vithip.DeviceBuffer.from_numpy(np.zeros(shape, np.float32))

    def clear():
        vithip.lib().vh_memcpy_h2d(0, dout.ptr, np.zeros(shape, np.float32).ctypes.data, BATCH * cfg["classes"] * 4)

    ctx.forward_device_tensor(din.ptr, elem, layout, BATCH, dout.ptr)
    assert same_bits(dout.to_numpy(np.float32, shape), ref)
    clear()
    ctx.forward_device_tensor_async(din.ptr, elem, layout, BATCH, dout.ptr, steps=3)
    ctx.synchronize()
    assert same_bits(dout.to_numpy(np.float32, shape), ref)
    try:
        ctx.set_streams(2)   # parts of 2 and 1 images: the second part's pointer advances by the ELEMENT size
        clear()
        ctx.forward_device_tensor(din.ptr, elem, layout, BATCH, dout.ptr)
        assert same_bits(dout.to_numpy(np.float32, shape), ref)
        assert same_bits(ctx.forward_tensor(R.to_layout(nhwc, layout), layout, elem), ref)
    finally:
        ctx.set_streams(1)
    for off in (2, 8):       # a device input pointer that is not 16-byte aligned
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_tensor(din.ptr + off, elem, layout, BATCH, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "aligned" in str(e.value)
    for batch in (0, BATCH + 1):
        with pytest.raises(vithip.VhError) as e:
            ctx.forward_device_tensor(din.ptr, elem, layout, batch, dout.ptr)
        assert e.value.code == VH_ERR_INVALID and "batch" in str(e.value)
    din.free(); dout.free()


def test_graphs_eager_captured_replayed(micro):
    _, cfg, data = micro
    nhwc, ref = data[vithip.ELEM_F16]
    x = R.to_layout(nhwc, vithip.LAYOUT_NCHW)
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=BATCH)   # its own context: no batch size has run yet
    ctx.init_weights_seeded(17)
    ctx.set_graph(True)
    try:
        assert same_bits(ctx.forward_tensor(x, vithip.LAYOUT_NCHW), ref)   # first forward at this batch: eager
        assert ctx.get_graph() == (True, 0)
        assert same_bits(ctx.forward_tensor(x, vithip.LAYOUT_NCHW), ref)   # captured and launched
        assert ctx.get_graph() == (True, 1)
        assert same_bits(ctx.forward_tensor(x, vithip.LAYOUT_NCHW), ref)   # replayed
        assert ctx.get_graph() == (True, 1)
    finally:
        ctx.close()


def test_graph_cache_keys_on_element_type_and_layout(micro):
    """One device buffer, one logits buffer, one batch: only the kind tells the three launch sequences apart."""
    ctx, cfg, data = micro
    scale, shift = ctx.get_input_norm()
    shape = (BATCH, cfg["classes"])
    rng = np.random.default_rng(4)
    # bit patterns that are tame values both as fp16 and as bf16: sign 0, fp16 exponent field 13..15 = bf16 exponent 104..127
    bits = (rng.integers(0x3400, 0x3C00, size=(BATCH, 3, 64, 64)) | (rng.integers(0, 2, size=(BATCH, 3, 64, 64)) << 15)).astype(np.uint16)
    kinds = [(vithip.ELEM_F16, vithip.LAYOUT_NCHW), (vithip.ELEM_BF16, vithip.LAYOUT_NCHW), (vithip.ELEM_F16, vithip.LAYOUT_NHWC)]
    views = [bits.view(np.float16), bits, bits.view(np.float16).reshape(BATCH, 64, 64, 3)]   # the same memory read three ways
    refs = [ctx.forward(R.tensor_reference(v, e, l, scale, shift)) for v, (e, l) in zip(views, kinds)]
    assert all(np.isfinite(r).all() for r in refs)
    assert not same_bits(refs[0], refs[1]) and not same_bits(refs[0], refs[2]) and not same_bits(refs[1], refs[2])
    din = vithip.DeviceBuffer.from_numpy(bits)
    dout = vithip.DeviceBuffer(BATCH * cfg["classes"] * 4)
    ctx.set_graph(True)
    try:
        ctx.forward_device_tensor(din.ptr, *kinds[0], BATCH, dout.ptr)      # eager (unless an earlier test warmed this batch size)
        ctx.forward_device_tensor(din.ptr, *kinds[0], BATCH, dout.ptr)      # captured
        n0 = ctx.get_graph()[1]
        assert n0 >= 1
        for i, kind in enumerate(kinds):
            ctx.forward_device_tensor(din.ptr, *kind, BATCH, dout.ptr)
            assert same_bits(dout.to_numpy(np.float32, shape), refs[i]), i
            assert ctx.get_graph() == (True, n0 + i)                        # a new graph per kind, none replayed for another
        for i, kind in enumerate(kinds):                                    # and each replays its own
            ctx.forward_device_tensor(din.ptr, *kind, BATCH, dout.ptr)
            assert same_bits(dout.to_numpy(np.float32, shape), refs[i]), i
        assert ctx.get_graph() == (True, n0 + 2)
    finally:
        ctx.set_graph(False)
        din.free(); dout.free()


# ---- 4. the ring -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", R.ELEMS, ids=lambda e: R.ELEM_NAME[e])
def test_tensor_ring(micro, elem):
    ctx, cfg, data = micro
    nhwc, ref = data[elem]
    x = R.to_layout(nhwc, vithip.LAYOUT_NCHW)
    batches, want = [x[0:2], x[2:3], x[1:3]], [ref[0:2], ref[2:3], ref[1:3]]
    ctx.ring_create_tensor(3, 2, elem, vithip.LAYOUT_NCHW)
    try:
        assert ctx.ring_free_slots() == 3
        with pytest.raises(vithip.VhError) as e:
            ctx.ring_collect()
        assert e.value.code == VH_ERR_RING_EMPTY
        view = ctx.ring_input_tensor()
        assert view.dtype == np.uint8 and view.size == 2 * 64 * 64 * 3 * vithip.ELEM_BYTES[elem]   # capacity: by the element type
        view.view(x.dtype).reshape(2, 3, 64, 64)[...] = batches[0]
        ctx.ring_submit_tensor(batch=2)            # filled in place
        ctx.ring_input_tensor().view(x.dtype)[:batches[1].size] = batches[1].reshape(-1)
        ctx.ring_submit_tensor(batch=1)            # filled in place, a partial batch
        for wrong in (lambda: ctx.ring_submit(np.zeros((1, 64, 64, 3), np.float32)), lambda: ctx.ring_input(1),
                      lambda: ctx.ring_submit_u8(np.zeros((1, 64, 64, 3), np.uint8)), lambda: ctx.ring_input_u8(1),
                      lambda: ctx.ring_input_frames()):                     # the other kinds' calls on a tensor ring
            with pytest.raises(vithip.VhError) as e:
                wrong()
            assert e.value.code == VH_ERR_STATE
        ctx.ring_submit_tensor(batches[2])         # from a pointer
        assert ctx.ring_free_slots() == 0
        with pytest.raises(vithip.VhError) as e:   # a fourth submit before any collect
            ctx.ring_submit_tensor(batches[1])
        assert e.value.code == VH_ERR_RING_FULL
        for w in want:                             # FIFO
            assert same_bits(ctx.ring_collect(), w)
        assert ctx.ring_free_slots() == 3
        # the tensor calls on the other kinds of ring
        for create in (lambda: ctx.ring_create(2, 2), lambda: ctx.ring_create_u8(2, 2), lambda: ctx.ring_create_frames(2, 2, 4096)):
            create()
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_submit_tensor(batches[1])
            assert e.value.code == VH_ERR_STATE
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_input_tensor()
            assert e.value.code == VH_ERR_STATE
        for bad_elem, bad_layout in ((4, 1), (-1, 0), (0, 2)):
            with pytest.raises(vithip.VhError) as e:
                ctx.ring_create_tensor(2, 2, bad_elem, bad_layout)
            assert e.value.code == VH_ERR_INVALID
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)


# ---- 5. torch tensors ------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r"""
import torch                      # before libvithip.so is loaded: one HIP runtime in the process (INTEGRATION.md)
import numpy as np
import tensor_ref as R, vh_synth as S, vithip
from test_gpu_u8_input import norm_for
cfg = S.CONFIGS["vit_micro"]
ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=3)
ctx.init_weights_seeded(17)
scale, shift = norm_for(3)
ctx.set_input_norm(scale, shift)
data = {}
for elem in R.ELEMS:
    nhwc = R.make_tensor(elem, 3, cfg["image_size"], 3, seed=9 + elem, extremes=False)
    data[elem] = (nhwc, ctx.forward(R.tensor_reference(nhwc, elem, vithip.LAYOUT_NHWC, scale, shift)))
    assert np.isfinite(data[elem][1]).all()
dev = torch.device("cuda", 0)

def check(x, ref, device_type):
    got = ctx.forward_torch(x)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == device_type, (got.dtype, got.device)
    assert got.shape == ref.shape and np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))

f16, ref16 = data[vithip.ELEM_F16]
f32, ref32 = data[vithip.ELEM_F32]
b16, refb = data[vithip.ELEM_BF16]
u8, refu = data[vithip.ELEM_U8]
nchw = lambda a: torch.from_numpy(R.to_layout(a, vithip.LAYOUT_NCHW))
check(nchw(f16).to(dev), ref16, "cuda")                                                    # CUDA fp16, NCHW
x = nchw(f32).to(dev).contiguous(memory_format=torch.channels_last)                        # CUDA fp32, channels_last: NHWC in place
assert not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
check(x, ref32, "cuda")
check(nchw(b16.view(np.int16)).view(torch.bfloat16).to(dev), refb, "cuda")                 # CUDA bf16
check(nchw(u8).to(dev), refu, "cuda")                                                      # CUDA uint8
x = nchw(f16).to(dev).transpose(2, 3).contiguous()[:, :, ::1, :].transpose(2, 3)           # a view that is neither: .contiguous() first
assert not x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
assert torch.equal(x, nchw(f16).to(dev))
check(x, ref16, "cuda")
check(nchw(f16), ref16, "cpu")                                                             # CPU fp16: the host entry point
try:
    ctx.forward_torch(nchw(f32).double())
    raise SystemExit("float64 was not refused")
except TypeError:
    pass
if torch.cuda.device_count() > 1:
    try:
        ctx.forward_torch(nchw(f16).to(torch.device("cuda", 1)))
        raise SystemExit("a tensor on another GPU was not refused")
    except ValueError:
        pass
print("forward_torch ok")
"""


def run_script(script):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.pathsep.join([os.path.join(root, "tests"), os.path.join(root, "vit-fpga_amd", "python")])
    env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_forward_torch():
    """In a process of its own: torch brings a HIP runtime of its own and has to be imported before libvithip.so is loaded (one
    runtime per process), and this process loaded the library long ago.  For the same reason the test only LOOKS
    for torch here (what pytest.importorskip would do by importing it): a second runtime loaded into this process ends it with a
    double free when the interpreter exits."""
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    assert "forward_torch ok" in run_script(TORCH_SCRIPT)
