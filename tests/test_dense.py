"""CPU suite of the dense heads (include/vithip.h, "Dense heads"): the refusals that need no device, the agreement of the header
with the binding's symbol table, and the BatchNorm fold of DINOv2's linear segmentation head."""
import os

import numpy as np
import pytest

import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device pointers that are never dereferenced: the taps refuse before they touch a device
ROWS, W, BIAS, OUT, CLS, SCORE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
DENSE_SYMBOLS = ["vh_set_dense_head", "vh_dense_dims", "vh_read_dense_logits", "vh_read_dense_logits_device", "vh_read_dense_logits_device_async",
                 "vh_read_dense_map", "vh_read_dense_map_device", "vh_read_dense_map_device_async", "vh_op_dense_head", "vh_op_dense_argmax"]


def head_tap(**kw):
    a = dict(rows_ptr=ROWS, rows=50, dim=256, w_ptr=W, bias_ptr=BIAS, classes=21, group=25, out_ptr=OUT, dtype=vithip.DTYPE_BF16)
    a.update(kw)
    vithip.op_dense_head(**a)


def argmax_tap(**kw):
    a = dict(logits_ptr=OUT, batch=2, classes=21, gh=5, gw=5, out_h=40, out_w=40, classes_ptr=CLS, score_ptr=SCORE)
    a.update(kw)
    vithip.op_dense_argmax(**a)


REFUSALS = [
    (head_tap, dict(rows_ptr=None)), (head_tap, dict(w_ptr=None)), (head_tap, dict(out_ptr=None)),
    (head_tap, dict(classes=0)), (head_tap, dict(classes=257)), (head_tap, dict(dtype=vithip.DTYPE_FP8)),
    (head_tap, dict(dim=48)), (head_tap, dict(dim=2064)), (head_tap, dict(dim=72)),
    (head_tap, dict(group=0)), (head_tap, dict(rows=0)), (head_tap, dict(rows=51)), (head_tap, dict(bias_ptr=BIAS + 4)),
    (argmax_tap, dict(logits_ptr=None)), (argmax_tap, dict(classes_ptr=None)), (argmax_tap, dict(batch=0)),
    (argmax_tap, dict(classes=257)), (argmax_tap, dict(gh=65)), (argmax_tap, dict(out_h=0)), (argmax_tap, dict(out_w=4097)),
    (argmax_tap, dict(score_ptr=SCORE + 8)),
]


def refusal_message(tap, kw):
    with pytest.raises(vithip.VhError) as e:
        tap(**kw)
    assert e.value.code == VH_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("tap,kw", REFUSALS, ids=[f"{t.__name__}-{k}" for t, k in REFUSALS])
def test_taps_refuse_before_touching_a_device(tap, kw):
    assert "dense_" in refusal_message(tap, kw)


def test_refusals_with_different_causes_have_different_messages():
    msgs = {}
    for tap, kw in REFUSALS:
        msgs.setdefault(refusal_message(tap, kw), []).append(kw)
    # the only causes that share a message: both ends of one range (classes 0 / 257 of the head tap, out_h 0 / out_w 4097)
    assert len(msgs) == len(REFUSALS) - 2, msgs


def test_context_calls_refuse_a_null_context():
    L = vithip.lib()
    calls = [lambda: L.vh_set_dense_head(None, W, None, 3, 0), lambda: L.vh_dense_dims(None, None, None, None, None),
             lambda: L.vh_read_dense_logits(None, 1, OUT, 0), lambda: L.vh_read_dense_logits_device(None, 1, OUT, 0),
             lambda: L.vh_read_dense_logits_device_async(None, 1, OUT, 0), lambda: L.vh_read_dense_map(None, 1, 8, 8, CLS, None),
             lambda: L.vh_read_dense_map_device(None, 1, 8, 8, CLS, None), lambda: L.vh_read_dense_map_device_async(None, 1, 8, 8, CLS, None)]
    for call in calls:
        assert call() == VH_ERR_INVALID
        assert b"null context" in L.vh_last_error(None)


def test_header_and_symbol_table_agree():
    header = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert "/* ---- Dense heads" in header and "#define VH_ABI_VERSION 1\n" in header
    for name in DENSE_SYMBOLS:
        assert f"int {name}(" in header, name
        assert name in vithip.SYMBOLS, name
        assert hasattr(vithip.lib(), name), name   # exported by the library that was built
    declared = {n for n in vithip.SYMBOLS if "dense" in n}
    assert declared == set(DENSE_SYMBOLS)


@pytest.mark.parametrize("conv_bias", [True, False])
def test_bnhead_fold_equals_batchnorm_then_conv(conv_bias):
    rng = np.random.default_rng(3)
    C, D, eps = 21, 384, 1e-5
    sd = {"decode_head.bn.weight": 1 + 0.1 * rng.standard_normal(D), "decode_head.bn.bias": 0.1 * rng.standard_normal(D),
          "decode_head.bn.running_mean": rng.standard_normal(D), "decode_head.bn.running_var": rng.uniform(0.5, 2.0, D),
          "decode_head.conv_seg.weight": 0.05 * rng.standard_normal((C, D, 1, 1))}
    if conv_bias:
        sd["decode_head.conv_seg.bias"] = 0.1 * rng.standard_normal(C)
    w, b = vithip.dense_head_from_dinov2_bnhead(sd)
    assert w.shape == (C, D) and b.shape == (C,) and w.dtype == np.float32 and b.dtype == np.float32
    x = rng.standard_normal((50, D))
    bn = (x - sd["decode_head.bn.running_mean"]) / np.sqrt(sd["decode_head.bn.running_var"] + eps) * sd["decode_head.bn.weight"] + sd["decode_head.bn.bias"]
    ref = bn @ sd["decode_head.conv_seg.weight"].reshape(C, D).T + (sd["decode_head.conv_seg.bias"] if conv_bias else 0.0)
    w64, b64 = vithip.dense_head_from_dinov2_bnhead(sd, dtype=np.float64)
    assert np.abs(x @ w64.T + b64 - ref).max() <= 1e-12
    assert np.array_equal(w, w64.astype(np.float32)) and np.array_equal(b, b64.astype(np.float32))   # one rounding to float32
    with pytest.raises(ValueError):   # the multi-scale head's convolution takes four layers' channels: out of scope
        vithip.dense_head_from_dinov2_bnhead({**sd, "decode_head.conv_seg.weight": np.zeros((C, 4 * D, 1, 1))})


def test_measurement_tool_compiles():
    import py_compile
    py_compile.compile(os.path.join(ROOT, "tools", "dense_bench.py"), doraise=True)
