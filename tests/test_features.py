"""CPU suite of the token features (include/vithip.h, "Token features"): the descriptor's layout, the operator tap's refusals --
every argument is judged before a device is touched, so they are testable here --, the loud failure of the context calls, and the
numpy reference the GPU tests lean on."""
import ctypes as C

import numpy as np
import pytest

import features_ref as R
import oracle_lib as O
import vithip

VH_ERR_INVALID = 1
# device pointers that are never dereferenced: the tap refuses before it touches a device
HI, LO, GAMMA, BETA, PATCH, MEAN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def test_descriptor_layout():
    F = vithip.Features
    assert C.sizeof(F) == 32
    assert (F.cls.offset, F.patch.offset, F.mean.offset, F.elem.offset, F.norm.offset) == (0, 8, 16, 24, 28)
    assert (vithip.FEAT_NORM, vithip.FEAT_RAW) == (0, 1)


def tap(**kw):
    a = dict(hi=HI, lo=LO, form=vithip.DTYPE_BF16, batch=2, tokens=5, dim=256, gamma=GAMMA, beta=BETA, eps=1e-6,
             elem=vithip.ELEM_F32, norm=vithip.FEAT_NORM, patch=PATCH, mean=MEAN)
    a.update(kw)
    vithip.op_token_features(a["hi"], a["lo"], a["form"], a["batch"], a["tokens"], a["dim"], a["gamma"], a["beta"], a["eps"],
                             a["elem"], a["norm"], a["patch"], a["mean"])


REFUSALS = [
    ("dim_60", dict(dim=60)), ("dim_2056", dict(dim=2056)), ("dim_100", dict(dim=100)),
    ("tokens_1", dict(tokens=1)), ("tokens_4098", dict(tokens=4098)),
    ("no_output", dict(patch=None, mean=None)),
    ("elem_u8", dict(elem=vithip.ELEM_U8)),
    ("norm_2", dict(norm=2)),
    ("form_7", dict(form=7)),
    ("null_input", dict(hi=None)),
    ("planes_without_lo", dict(lo=None)),
    ("fp32_rows_with_lo", dict(form=vithip.FEAT_FORM_F32)),
    ("batch_0", dict(batch=0)),
    ("norm_without_gamma", dict(gamma=None)),
    ("eps_0", dict(eps=0.0)),
    ("misaligned_output", dict(patch=PATCH + 8)),
]


def refusal_message(kw):
    with pytest.raises(vithip.VhError) as e:
        tap(**kw)
    assert e.value.code == VH_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[n for n, _ in REFUSALS])
def test_operator_tap_refuses_before_touching_a_device(name, kw):
    assert "token_features" in refusal_message(kw)


def test_every_refusal_has_a_message_of_its_own():
    msgs = [refusal_message(kw) for _, kw in REFUSALS]
    assert len(set(msgs)) == len(msgs), msgs


def test_context_calls_fail_loudly_on_a_null_context():
    L = vithip.lib()
    desc = vithip.Features(None, PATCH, None, vithip.ELEM_F32, vithip.FEAT_NORM)
    for fn in (L.vh_read_features, L.vh_read_features_device, L.vh_read_features_device_async):
        assert fn(None, C.byref(desc)) == VH_ERR_INVALID
        assert b"null context" in L.vh_last_error(None)
    b = C.c_int(7)
    assert L.vh_features_dims(None, C.byref(b), None, None, None) == VH_ERR_INVALID


def test_reference_layernorm_agrees_with_the_oracle():
    rng = np.random.default_rng(5)
    for dim in (64, 192, 768):
        x = (rng.standard_normal((9, dim)) * 1.7 + 0.4).astype(np.float32)
        g = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
        b = (0.02 * rng.standard_normal(dim)).astype(np.float32)
        ref = R.layernorm64(x, g, b, 1e-6)
        got = O.layernorm(x, g, b, 1e-6)
        # the oracle computes in fp32: a few fp32 roundings of values of order max|ref|
        assert np.abs(got - ref).max() <= 2.0 ** -20 * np.abs(ref).max()


def test_reference_mean_chain_is_the_sequential_fp32_sum():
    rng = np.random.default_rng(6)
    p = rng.standard_normal((2, 36, 8)).astype(np.float32)
    got = R.mean_chain(p)
    for b in range(2):
        for k in range(8):
            acc = np.float32(0.0)
            for t in range(36):
                acc = np.float32(acc + p[b, t, k])
            assert got[b, k] == np.float32(acc * np.float32(1.0 / 36))
    assert got.dtype == np.float32


def test_reference_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -2.5], dtype=np.float32)
    assert np.array_equal(vithip.from_bf16_bits(R.rne16(x, vithip.ELEM_BF16)),
                          np.array([1.0, 1.0, 1.015625, 1.0, 1.0, -2.5], dtype=np.float32))
    assert np.array_equal(R.rne16(x, vithip.ELEM_F16).view(np.float16).astype(np.float32),
                          np.array([1.0, 1.00390625, 1.01171875, 1.0, 1.0 + 2.0 ** -9, -2.5], dtype=np.float32))


@pytest.mark.parametrize("form", [vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8, vithip.FEAT_FORM_F32])
def test_reference_split_planes_reconstruct_the_rows(form):
    rng = np.random.default_rng(7)
    x = R.rows_with_outlier(rng, 2, 5, 64)
    hi, lo, xr = R.split_planes(x, form)
    assert xr.dtype == np.float32 and xr.shape == x.shape
    # what the pair keeps of x: 12 / 15 significant bits (16-bit hi + 4-bit lo), e4m3 + bf16: 3 + 8
    rel = {vithip.DTYPE_BF16: 2.0 ** -12, vithip.DTYPE_FP16: 2.0 ** -15, vithip.DTYPE_FP8: 2.0 ** -11, vithip.FEAT_FORM_F32: 0.0}[form]
    assert np.all(np.abs(xr - x) <= rel * np.abs(x) + 2.0 ** -13)


def test_measurement_tool_compiles():
    import os
    import py_compile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    py_compile.compile(os.path.join(root, "tools", "features_bench.py"), doraise=True)
