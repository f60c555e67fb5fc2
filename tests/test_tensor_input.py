"""CPU suite of the image-tensor input path (include/vithip.h, "Image tensors"): the constants, the reference's own checks
(tensor_ref.py, which the GPU suite test_gpu_tensor_input.py imports), the binding's new names, and every refusal that needs no
device -- each VH_ERR_INVALID with a message that names the argument."""
import ctypes as C
import os
import py_compile
import re

import numpy as np
import pytest

import tensor_ref as R
import vithip
from vh_testlib import last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VH_ERR_INVALID = 1


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "vithip.h")).read()
    want = {"VH_ELEM_F32": vithip.ELEM_F32, "VH_ELEM_F16": vithip.ELEM_F16, "VH_ELEM_BF16": vithip.ELEM_BF16, "VH_ELEM_U8": vithip.ELEM_U8,
            "VH_LAYOUT_NHWC": vithip.LAYOUT_NHWC, "VH_LAYOUT_NCHW": vithip.LAYOUT_NCHW}
    for name, value in want.items():
        m = re.search(rf"^#define {name} (\d+)\s*$", text, flags=re.M)
        assert m and int(m.group(1)) == value, name
    assert (vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16, vithip.ELEM_U8) == (0, 1, 2, 3)
    assert (vithip.LAYOUT_NHWC, vithip.LAYOUT_NCHW) == (0, 1)
    assert vithip.ELEM_BYTES == {0: 4, 1: 2, 2: 2, 3: 1}
    # nothing existing moved (the issue's constraints): stage names, ABI version
    assert vithip.STAGES[0] == "im2col" and vithip.lib().vh_abi_version() == 1


def test_new_names_are_bound():
    for name in ("vh_forward_tensor", "vh_forward_device_tensor", "vh_forward_device_tensor_async", "vh_ring_create_tensor",
                 "vh_ring_input_tensor", "vh_ring_submit_tensor", "vh_op_im2col_tensor"):
        assert name in vithip.SYMBOLS and hasattr(vithip.lib(), name)
    for name in ("forward_tensor", "forward_device_tensor", "forward_device_tensor_async", "forward_torch", "ring_create_tensor",
                 "ring_input_tensor", "ring_submit_tensor"):
        assert callable(getattr(vithip.VitContext, name))
    assert callable(vithip.op_im2col_tensor)


# ---- the reference checks itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", R.ELEMS, ids=lambda e: R.ELEM_NAME[e])
def test_layout_round_trip(elem):
    a = R.make_tensor(elem, 2, 12, 5, seed=3)
    assert a.dtype == R.NUMPY_DTYPE[elem] and a.shape == (2, 12, 12, 5)
    nchw = R.to_layout(a, vithip.LAYOUT_NCHW)
    assert nchw.shape == (2, 5, 12, 12) and nchw.flags["C_CONTIGUOUS"]
    assert nchw[1, 3, 7, 2].tobytes() == a[1, 7, 2, 3].tobytes()
    assert R.same_bits(R.from_layout(nchw, vithip.LAYOUT_NCHW), a)
    assert R.same_bits(R.to_layout(a, vithip.LAYOUT_NHWC), a)
    scale, shift = np.full(5, np.float32(1.0 / 255.0)), np.zeros(5, np.float32)
    r_nhwc = R.tensor_reference(a, elem, vithip.LAYOUT_NHWC, scale, shift)
    r_nchw = R.tensor_reference(nchw, elem, vithip.LAYOUT_NCHW, scale, shift)
    assert r_nhwc.dtype == np.float32 and r_nhwc.shape == a.shape and R.same_bits(r_nhwc, r_nchw)


def test_bf16_widening_is_exact():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)          # every bf16 pattern
    wide = R.widen(bits, vithip.ELEM_BF16)
    assert np.array_equal(wide.view(np.uint32), bits.astype(np.uint32) << 16)
    finite = ~np.isnan(wide)
    # rounding the widened value back to bf16 gives the pattern again: nothing was added and nothing lost
    assert np.array_equal(vithip.to_bf16_bits(wide[finite]), bits[finite])
    assert np.array_equal(vithip.from_bf16_bits(bits).view(np.uint32), wide.view(np.uint32))
    # the planted specials are what their comment says
    v = R.widen(np.array(R.SPECIAL_BITS[vithip.ELEM_BF16], dtype=np.uint16), vithip.ELEM_BF16)
    assert np.signbit(v[1]) and v[1] == 0 and v[2] == np.float32(2.0) ** -133 and v[3] == np.float32(2.0) ** -126
    assert np.isposinf(v[5]) and np.isneginf(v[6]) and v[7] == 65536.0 and v[9] == 1.0078125


def test_fp16_widening_is_exact():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)          # every fp16 pattern
    half = bits.view(np.float16)
    wide = R.widen(half, vithip.ELEM_F16)
    finite = ~np.isnan(wide)
    with np.errstate(over="ignore"):
        assert np.array_equal(wide[finite].astype(np.float16).view(np.uint16), bits[finite])   # exact: it converts back to itself
    assert np.array_equal(wide[finite].astype(np.float64), half[finite].astype(np.float64))
    assert wide[1] == np.float32(2.0) ** -24 and wide[0x0400] == np.float32(2.0) ** -14 and wide[0x7BFF] == 65504.0
    assert np.signbit(wide[0x8000]) and np.isposinf(wide[0x7C00]) and np.isneginf(wide[0xFC00])


def test_specials_round_differently_to_the_two_operand_types():
    for elem in (vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16):
        a = np.array(R.SPECIAL_BITS[elem], dtype={4: np.uint32, 2: np.uint16}[vithip.ELEM_BYTES[elem]]).view(R.NUMPY_DTYPE[elem])
        v = R.widen(a, elem)
        with np.errstate(over="ignore"):
            as_bf16, as_fp16 = vithip.from16(vithip.to16(v, vithip.DTYPE_BF16), vithip.DTYPE_BF16), vithip.from16(vithip.to16(v, vithip.DTYPE_FP16), vithip.DTYPE_FP16)
        assert (as_bf16 != as_fp16).any(), R.ELEM_NAME[elem]
    # and the generator plants every special, extremes or not
    for elem in (vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16):
        full = R.widen(R.make_tensor(elem, 3, 12, 5, seed=1), elem)
        tame = R.widen(R.make_tensor(elem, 3, 12, 5, seed=1, extremes=False), elem)
        assert np.isinf(full).sum() == 4 and np.isfinite(tame).all() and np.abs(tame).max() < R.EXTREME
        assert not np.isnan(full).any()


# ---- refusals that need no device -------------------------------------------------------------------------------------------------


GOOD = dict(in_dev=4096, elem=vithip.ELEM_F16, layout=vithip.LAYOUT_NCHW, batch=1, image=32, patch=16, channels=3, kpad=768,
            scale=None, shift=None, out=8192, dtype=vithip.DTYPE_BF16)


def op(**kw):
    a = dict(GOOD, **kw)
    return vithip.lib().vh_op_im2col_tensor(a["in_dev"], a["elem"], a["layout"], a["batch"], a["image"], a["patch"], a["channels"], a["kpad"],
                                            a["scale"], a["shift"], a["out"], a["dtype"], None)


@pytest.mark.parametrize("bad", [-1, 4, 100])
def test_unknown_elem_and_layout_are_refused(bad):
    L = vithip.lib()
    out = (C.c_float * 8)()
    img = (C.c_float * 64)()
    assert op(elem=bad) == VH_ERR_INVALID and "elem" in last_error()
    assert op(layout=bad) == VH_ERR_INVALID and "layout" in last_error()
    for call in (lambda e, l: L.vh_forward_tensor(None, img, e, l, 1, out), lambda e, l: L.vh_forward_device_tensor(None, 4096, e, l, 1, 8192),
                 lambda e, l: L.vh_forward_device_tensor_async(None, 4096, e, l, 1, 8192, 1)):
        assert call(bad, vithip.LAYOUT_NCHW) == VH_ERR_INVALID and "elem" in last_error()
        assert call(vithip.ELEM_F16, bad) == VH_ERR_INVALID and "layout" in last_error()


def test_null_pointers_are_refused():
    L = vithip.lib()
    assert op(in_dev=None) == VH_ERR_INVALID and "null" in last_error()
    assert op(out=None) == VH_ERR_INVALID and "null" in last_error()
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert op(elem=vithip.ELEM_U8, scale=one, shift=None) == VH_ERR_INVALID and "null" in last_error()   # u8 needs both arrays
    assert op(elem=vithip.ELEM_U8, scale=None, shift=one) == VH_ERR_INVALID and "null" in last_error()
    # the forward and ring entry points: a null context
    assert L.vh_forward_tensor(None, None, 0, 0, 1, None) == VH_ERR_INVALID and "null" in last_error()
    assert L.vh_forward_device_tensor(None, None, 0, 0, 1, None) == VH_ERR_INVALID and "null" in last_error()
    assert L.vh_forward_device_tensor_async(None, None, 0, 0, 1, None, 1) == VH_ERR_INVALID and "null" in last_error()
    assert L.vh_ring_create_tensor(None, 2, 1, 0, 1) == VH_ERR_INVALID and "null" in last_error()
    assert L.vh_ring_input_tensor(None, None, None) == VH_ERR_INVALID and "null" in last_error()
    assert L.vh_ring_submit_tensor(None, None, 1) == VH_ERR_INVALID and "null" in last_error()


def test_bad_shapes_and_dtypes_are_refused():
    assert op(image=30) == VH_ERR_INVALID and "patch" in last_error()                 # image % patch != 0
    assert op(patch=0) == VH_ERR_INVALID and "patch" in last_error()
    assert op(kpad=760) == VH_ERR_INVALID and "kpad" in last_error()                  # kpad < kp
    assert op(kpad=772) == VH_ERR_INVALID and "kpad" in last_error()                  # kpad % 8
    for ch in (0, -3, 65):
        assert op(channels=ch, kpad=16 * 16 * 65 + 8 - (16 * 16 * 65) % 8) == VH_ERR_INVALID and "channels" in last_error()
    for dt in (3, 7, vithip.DTYPE_FP8):
        assert op(dtype=dt) == VH_ERR_INVALID and "dtype" in last_error()
    assert op(batch=0) == VH_ERR_INVALID and "batch" in last_error()


@pytest.mark.parametrize("off", [1, 2, 8])
def test_a_misaligned_device_pointer_is_refused(off):
    L = vithip.lib()
    assert op(in_dev=4096 + off) == VH_ERR_INVALID and "aligned" in last_error()
    assert L.vh_forward_device_tensor(None, 4096 + off, vithip.ELEM_F16, vithip.LAYOUT_NCHW, 1, 8192) == VH_ERR_INVALID and "aligned" in last_error()
    assert L.vh_forward_device_tensor_async(None, 4096 + off, vithip.ELEM_F16, vithip.LAYOUT_NCHW, 1, 8192, 1) == VH_ERR_INVALID and "aligned" in last_error()


def test_wrappers_raise_python_errors_for_the_wrong_array():
    import vh_synth as S
    ctx = object.__new__(vithip.VitContext)   # what is left of a context whose vh_create failed
    ctx.h, ctx.cfg, ctx._ring_batch, ctx.device = None, dict(S.CONFIGS["vit_micro"]), 0, 0
    with pytest.raises(TypeError):
        ctx.forward_tensor(np.zeros((1, 3, 64, 64), np.float64), vithip.LAYOUT_NCHW)
    with pytest.raises(TypeError):    # uint16 says nothing: bf16 must be named
        ctx.forward_tensor(np.zeros((1, 3, 64, 64), np.uint16), vithip.LAYOUT_NCHW)
    with pytest.raises(TypeError):    # two bytes per element, not four
        ctx.forward_tensor(np.zeros((1, 3, 64, 64), np.float32), vithip.LAYOUT_NCHW, elem=vithip.ELEM_BF16)
    for call in (lambda: ctx.forward_tensor(np.zeros((1, 3, 64, 64), np.uint16), vithip.LAYOUT_NCHW, elem=vithip.ELEM_BF16),
                 lambda: ctx.forward_tensor(np.zeros((1, 3, 64, 64), np.float16), vithip.LAYOUT_NCHW),
                 lambda: ctx.forward_device_tensor(4096, vithip.ELEM_F16, vithip.LAYOUT_NCHW, 1, 8192),
                 lambda: ctx.forward_device_tensor_async(4096, vithip.ELEM_F16, vithip.LAYOUT_NCHW, 1, 8192),
                 lambda: ctx.ring_create_tensor(2, 1, vithip.ELEM_F16, vithip.LAYOUT_NCHW), lambda: ctx.ring_input_tensor(),
                 lambda: ctx.ring_submit_tensor(batch=1),
                 lambda: vithip.op_im2col_tensor(None, vithip.ELEM_F16, vithip.LAYOUT_NCHW, 1, 32, 16, 3, 768, None, vithip.DTYPE_BF16)):
        with pytest.raises(vithip.VhError) as e:
            call()
        assert e.value.code == VH_ERR_INVALID
    with pytest.raises(ValueError):
        vithip.op_im2col_tensor(4096, vithip.ELEM_U8, vithip.LAYOUT_NCHW, 1, 32, 16, 3, 768, 8192, vithip.DTYPE_BF16, np.ones(2), np.zeros(2))


def test_the_module_imports_without_torch():
    src = open(os.path.join(ROOT, "vit-fpga_amd", "python", "vithip.py")).read()
    top_level = [ln for ln in src.splitlines() if re.match(r"(import|from)\s+torch\b", ln)]
    assert not top_level          # torch is imported inside forward_torch only
    assert re.search(r"def forward_torch\(self, x\):.*?\n        import torch\n", src, flags=re.S)


def test_the_bench_tools_compile():
    for rel in ("tools/tensor_input_bench.py", "tools/gather_lds_banks.py"):
        py_compile.compile(os.path.join(ROOT, rel), doraise=True)
