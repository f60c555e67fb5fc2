"""CPU suite of the layer features (include/vithip.h, "Layer features"): the descriptor's layout, the new symbols, every refusal of the
second operator tap -- each argument is judged before a device is touched, so they are testable here --, the loud failure of the
context calls, and the numpy reference the GPU tests lean on."""
import ctypes as C
import os
import py_compile
import re
import subprocess

import numpy as np
import pytest

import features_ref as R
import layer_features_ref as LR
import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device pointers that are never dereferenced: the tap refuses before it touches a device
HI, LO, GAMMA, BETA, PATCH, MEAN, REG = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
NEW_SYMBOLS = ("vh_set_feature_layers", "vh_get_feature_layers", "vh_read_layer_features", "vh_read_layer_features_device",
               "vh_read_layer_features_device_async", "vh_op_token_features2")


def test_descriptor_layout():
    F = vithip.LayerFeatures
    assert C.sizeof(F) == 48
    assert (F.cls.offset, F.patch.offset, F.mean.offset, F.reg.offset) == (0, 8, 16, 24)
    assert (F.elem.offset, F.norm.offset, F.layer.offset, F.patch_layout.offset) == (32, 36, 40, 44)
    assert (vithip.FEAT_ROWS, vithip.FEAT_NCHW, vithip.MAX_FEATURE_LAYERS) == (0, 1, 8)
    assert C.sizeof(vithip.Features) == 32   # the older descriptor keeps its size


def test_header_states_the_layout_and_the_constants():
    text = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert re.search(r"#define\s+VH_MAX_FEATURE_LAYERS\s+8\b", text)
    assert re.search(r"#define\s+VH_FEAT_ROWS\s+0\b", text) and re.search(r"#define\s+VH_FEAT_NCHW\s+1\b", text)
    assert "sizeof == 48: cls 0, patch 8, mean 16, reg 24, elem 32, norm 36, layer 40, patch_layout 44" in text


def test_new_symbols_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vithip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vh_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in vithip.SYMBOLS, name
        assert getattr(vithip.lib(), name).argtypes == vithip.SYMBOLS[name][1]
    for name in ("set_feature_layers", "feature_layers", "read_layer_features", "read_layer_features_device",
                 "read_layer_features_device_async", "get_intermediate_layers"):
        assert callable(getattr(vithip.VitContext, name)), name


def tap2(**kw):
    a = dict(hi=HI, lo=LO, form=vithip.DTYPE_BF16, batch=2, tokens=9, lead=5, dim=256, gamma=GAMMA, beta=BETA, eps=1e-6,
             elem=vithip.ELEM_F32, norm=vithip.FEAT_NORM, patch=PATCH, layout=vithip.FEAT_NCHW, mean=MEAN, reg=REG)
    a.update(kw)
    vithip.op_token_features2(a["hi"], a["lo"], a["form"], a["batch"], a["tokens"], a["lead"], a["dim"], a["gamma"], a["beta"], a["eps"],
                              a["elem"], a["norm"], a["patch"], a["layout"], a["mean"], a["reg"])


REFUSALS = [
    ("dim_60", dict(dim=60)), ("dim_2056", dict(dim=2056)), ("dim_100", dict(dim=100)),
    ("tokens_1", dict(tokens=1, lead=1, reg=None)), ("tokens_4098", dict(tokens=4098)),
    ("lead_0", dict(lead=0)), ("lead_is_tokens", dict(lead=9)),
    ("no_output", dict(patch=None, mean=None, reg=None)),
    ("reg_without_register_rows", dict(lead=1)),
    ("layout_2", dict(layout=2)), ("layout_minus_1", dict(layout=-1)),
    ("elem_u8", dict(elem=vithip.ELEM_U8)),
    ("norm_2", dict(norm=2)),
    ("form_7", dict(form=7)),
    ("null_input", dict(hi=None)),
    ("planes_without_lo", dict(lo=None)),
    ("fp32_rows_with_lo", dict(form=vithip.FEAT_FORM_F32)),
    ("batch_0", dict(batch=0)),
    ("norm_without_gamma", dict(gamma=None)),
    ("eps_0", dict(eps=0.0)),
    ("misaligned_patch", dict(patch=PATCH + 8)),
    ("misaligned_reg", dict(reg=REG + 4)),
]
SAME_MESSAGE = [{"layout_2", "layout_minus_1"}, {"misaligned_patch", "misaligned_reg"}, {"lead_0", "lead_is_tokens"}]


def refusal_message(kw):
    with pytest.raises(vithip.VhError) as e:
        tap2(**kw)
    assert e.value.code == VH_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[n for n, _ in REFUSALS])
def test_second_tap_refuses_before_touching_a_device(name, kw):
    assert "token_features" in refusal_message(kw)


def test_every_kind_of_refusal_has_a_message_of_its_own():
    msgs = {n: refusal_message(kw) for n, kw in REFUSALS}
    groups = {}
    for n, m in msgs.items():
        groups.setdefault(m, set()).add(n)
    # one message per kind of refusal: names share a message only where they are the same refusal
    for names in groups.values():
        assert len(names) == 1 or any(names <= same for same in SAME_MESSAGE), names
    assert "register rows" in msgs["reg_without_register_rows"] and "patch_layout" in msgs["layout_2"] and "lead" in msgs["lead_0"]


def test_first_tap_still_refuses_what_it_refused():
    # the older tap is the newer one with lead 1, rows layout and no register output: same checks, same messages
    with pytest.raises(vithip.VhError) as e:
        vithip.op_token_features(HI, LO, vithip.DTYPE_BF16, 2, 5, 256, GAMMA, BETA, 1e-6, vithip.ELEM_F32, vithip.FEAT_NORM, None, None)
    assert e.value.code == VH_ERR_INVALID and "no output requested" in str(e.value)


def test_context_calls_fail_loudly_on_a_null_context():
    L = vithip.lib()
    desc = vithip.LayerFeatures(None, PATCH, None, None, vithip.ELEM_F32, vithip.FEAT_NORM, -1, vithip.FEAT_ROWS)
    for fn in (L.vh_read_layer_features, L.vh_read_layer_features_device, L.vh_read_layer_features_device_async):
        assert fn(None, C.byref(desc)) == VH_ERR_INVALID
        assert b"null context" in L.vh_last_error(None)
    one = (C.c_int * 1)(1)
    assert L.vh_set_feature_layers(None, one, 1) == VH_ERR_INVALID
    assert b"null context" in L.vh_last_error(None)
    n = C.c_int(7)
    assert L.vh_get_feature_layers(None, one, C.byref(n)) == VH_ERR_INVALID


def test_reference_nchw_is_the_transpose_of_the_rows():
    rng = np.random.default_rng(3)
    p = rng.standard_normal((2, 36, 24)).astype(np.float32)
    t = LR.nchw(p)
    assert t.shape == (2, 24, 36) and t.flags["C_CONTIGUOUS"]
    for b, k, q in ((0, 0, 0), (1, 23, 35), (1, 7, 20), (0, 5, 31)):
        assert t[b, k, q] == p[b, q, k]
    g = LR.nchw(p, (6, 6))
    assert g.shape == (2, 24, 6, 6) and g[1, 7, 3, 2] == p[1, 3 * 6 + 2, 7]   # p = y * gw + x, row-major over the grid
    assert np.array_equal(R.bits(LR.rows_of(g)), R.bits(p)) and np.array_equal(R.bits(LR.rows_of(t)), R.bits(p))
    # 16-bit outputs: rounding per element commutes with the transposition
    assert np.array_equal(LR.nchw(R.rne16(p, vithip.ELEM_BF16)), R.rne16(LR.nchw(p), vithip.ELEM_BF16))


@pytest.mark.parametrize("form", [vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8, vithip.FEAT_FORM_F32])
def test_reference_row_addressing_agrees_with_features_ref(form):
    rng = np.random.default_rng(4)
    batch, tokens, lead, dim = 3, 9, 5, 64
    _, _, x = R.split_planes(R.rows_with_outlier(rng, batch, tokens, dim), form)
    x = x.reshape(batch, tokens, dim)
    gamma = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.02 * rng.standard_normal(dim)).astype(np.float32)
    raw = LR.outputs(x, lead)
    assert raw["cls"].shape == (batch, dim) and raw["reg"].shape == (batch, lead - 1, dim) and raw["patch"].shape == (batch, tokens - lead, dim)
    flat = x.reshape(batch * tokens, dim)
    for b in range(batch):
        assert np.array_equal(raw["cls"][b], flat[b * tokens])
        for r in range(lead - 1):
            assert np.array_equal(raw["reg"][b, r], flat[b * tokens + 1 + r])
        for p in range(tokens - lead):
            assert np.array_equal(raw["patch"][b, p], flat[b * tokens + lead + p])
    ref = LR.outputs(x, lead, gamma, beta, 1e-6)
    assert ref["patch"].dtype == np.float64
    assert np.array_equal(ref["patch"], R.layernorm64(x[:, lead:, :], gamma, beta, 1e-6))
    assert np.array_equal(ref["reg"], R.layernorm64(x[:, 1:lead, :], gamma, beta, 1e-6))
    # lead 1: no register rows, and the patch rows of features_ref's own addressing
    assert LR.outputs(x, 1)["reg"].shape == (batch, 0, dim) and np.array_equal(LR.outputs(x, 1)["patch"], x[:, 1:, :])
    # the mean the device must reproduce is the chain over these patch rows
    assert R.mean_chain(raw["patch"]).shape == (batch, dim)


def test_measurement_tool_compiles():
    py_compile.compile(os.path.join(ROOT, "tools", "layer_features_bench.py"), doraise=True)
