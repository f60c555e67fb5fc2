"""CPU suite of the 8-bit input path: the host helper, the binding's new names, the argument checks that need no device,
and a numpy statement of the contract

    x = fmaf((float)p, scale[c], shift[c])            one rounding

(tensor_ref.u8_reference) which the GPU suite (test_gpu_u8_input.py) imports as its reference array.

Why float64 numpy states it exactly: p has 8 significant bits and a float32 scale 24, so the float64 product p * scale is
exact (32 bits).  Adding the float32 shift is exact in float64 when every bit of both terms lies inside one 53-bit window:
  - 2^-12 <= |scale| < 8: the product is below 2^11 and its lowest bit is at least ulp(2^-12) = 2^-35;
  - |shift| <= 8, and shift == 0 or |shift| >= 2^-12: the shift is below 2^4 and its lowest bit is at least 2^-35 too.
2^11 down to 2^-35 is 46 bits.  The one rounding to float32 at the end is then the fma's.  Every test asserts these bounds
on the constants it uses (assert_norm_in_precondition), so the reference never leaves its precondition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vh_synth as S
import vithip
from tensor_ref import assert_norm_in_precondition, make_u8_images, u8_reference

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
DEFAULT_SCALE = np.float32(1.0 / 255.0)


def gather_patches(x, patch, kpad):
    """[B, I, I, C] -> the patch matrix [B * (I / patch)^2, kpad] in (ky, kx, c) column order, zero padded."""
    b, i, _, c = x.shape
    g = i // patch
    rows = x.reshape(b, g, patch, g, patch, c).transpose(0, 1, 3, 2, 4, 5).reshape(b * g * g, patch * patch * c)
    out = np.zeros((rows.shape[0], kpad), dtype=x.dtype)
    out[:, :rows.shape[1]] = rows
    return out


@pytest.mark.parametrize("mean,std", [(IMAGENET_MEAN, IMAGENET_STD), (CLIP_MEAN, CLIP_STD)], ids=["imagenet", "clip"])
def test_input_norm_from_mean_std(mean, std):
    scale, shift = vithip.input_norm_from_mean_std(mean, std)
    assert scale.dtype == np.float32 and shift.dtype == np.float32 and scale.shape == shift.shape == (3,)
    for c in range(3):
        assert scale[c] == np.float32(1.0 / (255.0 * float(std[c])))
        assert shift[c] == np.float32(-float(mean[c]) / float(std[c]))
    assert_norm_in_precondition(scale, shift)
    # and it is the usual normalisation, to float32 rounding: (p / 255 - mean) / std
    p = np.arange(256, dtype=np.float64)[:, None]
    want = (p / 255.0 - np.asarray(mean)) / np.asarray(std)
    got = u8_reference(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1), scale, shift)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    with pytest.raises(ValueError):
        vithip.input_norm_from_mean_std((0.5, 0.5), (0.2, 0.0))
    with pytest.raises(ValueError):
        vithip.input_norm_from_mean_std((0.5, 0.5, 0.5), (0.2, 0.2))


def test_reference_is_the_single_rounding_fma():
    """u8_reference against exact rational arithmetic, for every byte and the constants the GPU tests use."""
    from fractions import Fraction
    consts = [vithip.input_norm_from_mean_std(IMAGENET_MEAN, IMAGENET_STD), vithip.input_norm_from_mean_std(CLIP_MEAN, CLIP_STD),
              (np.full(3, DEFAULT_SCALE), np.zeros(3, np.float32)), (np.float32([0.0078125, 0.5, 0.003]), np.float32([-1.0, 0.25, 0.001]))]
    p = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for scale, shift in consts:
        got = u8_reference(p, scale, shift)
        for c in range(3):
            for v in range(0, 256, 5):
                exact = Fraction(v) * Fraction(float(scale[c])) + Fraction(float(shift[c]))
                assert Fraction(float(exact)) == exact          # the precondition at work: the sum is a double
                assert got[v, c] == np.float32(float(exact))    # and the float32 beside it is its one rounding
    assert DEFAULT_SCALE == np.float32(1.0) / np.float32(255.0)   # the library's default constant, 1.0f / 255.0f


def test_gather_patches_matches_the_k_order():
    x = np.arange(2 * 4 * 4 * 3, dtype=np.float32).reshape(2, 4, 4, 3)
    m = gather_patches(x, 2, 16)
    assert m.shape == (8, 16)
    # patch (py=1, px=0) of image 1: rows 2..3, columns 0..1
    want = np.concatenate([x[1, 2, 0], x[1, 2, 1], x[1, 3, 0], x[1, 3, 1]])
    assert np.array_equal(m[4 + 2, :12], want) and not m[:, 12:].any()


def test_make_u8_images_covers_every_byte():
    a = make_u8_images(3, 12, 5, 7)
    assert len(np.unique(a)) == 256
    assert (a[:, 0, 0] == 0).all() and (a[:, -1, -1] == 255).all()


def test_new_names_are_bound():
    for name in ("vh_set_input_norm", "vh_get_input_norm", "vh_forward_u8", "vh_forward_device_u8", "vh_forward_device_u8_async",
                 "vh_ring_create_u8", "vh_ring_input_u8", "vh_ring_submit_u8", "vh_op_im2col_u8"):
        assert name in vithip.SYMBOLS and hasattr(vithip.lib(), name)
    for name in ("set_input_norm", "get_input_norm", "forward_u8", "forward_device_u8", "forward_device_u8_async", "ring_create_u8",
                 "ring_input_u8", "ring_submit_u8"):
        assert callable(getattr(vithip.VitContext, name))
    assert callable(vithip.op_im2col_u8) and callable(vithip.input_norm_from_mean_std)


def test_argument_checks_without_a_device():
    L = vithip.lib()
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.vh_set_input_norm(None, None, None) == 1            # VH_ERR_INVALID: null context
    assert L.vh_set_input_norm(None, one, one) == 1
    assert L.vh_get_input_norm(None, one, one) == 1
    assert L.vh_forward_u8(None, None, 1, None) == 1
    assert L.vh_forward_device_u8(None, None, 1, None) == 1
    assert L.vh_forward_device_u8_async(None, None, 1, None, 1) == 1
    assert L.vh_ring_create_u8(None, 2, 1) == 1
    assert L.vh_ring_submit_u8(None, None, 1) == 1
    assert L.vh_ring_input_u8(None, None) == 1
    assert b"null" in L.vh_last_error(None)


def test_wrappers_raise_without_a_context_or_device():
    """A wrapper never crashes: with no context (and, on this suite's machine, no device) every call is a VhError."""
    ctx = object.__new__(vithip.VitContext)   # what is left of a context whose vh_create failed
    ctx.h, ctx.cfg, ctx._ring_batch = None, dict(S.CONFIGS["vit_micro"]), 0
    u8 = np.zeros((1, 64, 64, 3), dtype=np.uint8)
    calls = [lambda: ctx.set_input_norm(), lambda: ctx.set_input_norm(np.ones(3), np.zeros(3)), lambda: ctx.get_input_norm(),
             lambda: ctx.forward_u8(u8), lambda: ctx.forward_device_u8(None, 1, None), lambda: ctx.forward_device_u8_async(None, 1, None),
             lambda: ctx.ring_create_u8(2, 1), lambda: ctx.ring_create(2, 1, u8=True), lambda: ctx.ring_input_u8(1),
             lambda: ctx.ring_submit_u8(u8), lambda: ctx.ring_submit_u8(batch=1),
             lambda: vithip.op_im2col_u8(None, 1, 32, 16, 3, 768, np.ones(3), np.zeros(3), None, vithip.DTYPE_BF16)]
    for f in calls:
        with pytest.raises(vithip.VhError) as e:
            f()
        assert e.value.code == 1
    with pytest.raises(TypeError):
        ctx.forward_u8(u8.astype(np.float32))
    with pytest.raises(ValueError):
        ctx.set_input_norm(np.ones(2), np.zeros(2))
    if vithip.device_count() == 0:
        with pytest.raises(vithip.VhError) as e:
            vithip.VitContext(S.CONFIGS["vit_micro"]).forward_u8(u8)
        assert e.value.code == 5   # VH_ERR_NO_DEVICE


def test_the_u8_c_example_builds_as_c99(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(vithip.LIB_PATH)
    exe = tmp_path / "classify_u8"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "classify_u8.c"), "-L", lib_dir, "-lvithip", f"-Wl,-rpath,{lib_dir}",
                           "-o", str(exe)])
    if vithip.device_count() == 0:   # fails loudly, through the library's error string, without a device
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 1 and "vh_create" in r.stderr
