"""CPU suite of the attention maps (include/vithip.h, "Attention maps"): the descriptor's layout, the new symbols, every argument
refusal of the two operator taps -- each is judged before a device is touched, so they are testable here --, the loud failure of the
context calls, and the numpy references the GPU tests lean on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import attn_maps_ref as AM
import vh_synth as S
import vit_ref as RR
import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device pointers that are never dereferenced: the taps refuse before they touch a device
QKV, PROBS, STORE, OUT, MEAN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
NEW_SYMBOLS = ("vh_set_attention_layers", "vh_get_attention_layers", "vh_attention_dims", "vh_read_attention", "vh_read_attention_device",
               "vh_read_attention_device_async", "vh_op_attention_probs", "vh_op_attention_readout")


def test_reference_self_test():
    assert AM.self_test()


def test_descriptor_layout():
    F = vithip.AttentionMaps
    assert C.sizeof(F) == 32
    assert (F.probs.offset, F.head_mean.offset, F.elem.offset, F.layer.offset, F.keys.offset, F.reserved.offset) == (0, 8, 16, 20, 24, 28)
    assert (vithip.ATTN_Q_CLS, vithip.ATTN_Q_LEAD, vithip.ATTN_KEYS_ALL, vithip.ATTN_KEYS_PATCH, vithip.MAX_ATTENTION_LAYERS) == (0, 1, 0, 1, 64)


def test_header_states_the_layout_and_the_constants():
    text = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert re.search(r"#define\s+VH_MAX_ATTENTION_LAYERS\s+64\b", text)
    assert re.search(r"#define\s+VH_ATTN_Q_CLS\s+0\b", text) and re.search(r"#define\s+VH_ATTN_Q_LEAD\s+1\b", text)
    assert re.search(r"#define\s+VH_ATTN_KEYS_ALL\s+0\b", text) and re.search(r"#define\s+VH_ATTN_KEYS_PATCH\s+1\b", text)
    assert "sizeof == 32: probs 0, head_mean 8, elem 16, layer 20, keys 24, reserved 28" in text


def test_new_symbols_are_exported_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vithip.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vh_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in vithip.SYMBOLS, name
        assert getattr(vithip.lib(), name).argtypes == vithip.SYMBOLS[name][1]
    for name in ("set_attention_layers", "attention_layers", "attention_dims", "read_attention", "read_attention_device",
                 "read_attention_device_async", "cls_attention"):
        assert callable(getattr(vithip.VitContext, name)), name


# ---- the two taps refuse every bad argument before a device is touched ---------------------------------------------------------
def probs_tap(**kw):
    a = dict(qkv=QKV, batch=2, tokens=37, heads=3, hd=64, queries=5, dtype=vithip.DTYPE_BF16, probs=PROBS, hm=0)
    a.update(kw)
    vithip.op_attention_probs(a["qkv"], a["batch"], a["tokens"], a["heads"], a["hd"], a["queries"], a["dtype"], a["probs"], a["hm"])


def readout_tap(**kw):
    a = dict(store=STORE, batch=2, heads=3, queries=5, tokens=37, lead=5, elem=vithip.ELEM_F32, keys=vithip.ATTN_KEYS_ALL, out=OUT, mean=MEAN)
    a.update(kw)
    vithip.op_attention_readout(a["store"], a["batch"], a["heads"], a["queries"], a["tokens"], a["lead"], a["elem"], a["keys"], a["out"], a["mean"])


PROBS_REFUSALS = [
    ("null_qkv", dict(qkv=None)), ("null_probs", dict(probs=None)),
    ("batch_0", dict(batch=0)),
    ("tokens_0", dict(tokens=0)), ("tokens_4098", dict(tokens=4098)),
    ("head_dim_72", dict(hd=72)), ("head_dim_144", dict(hd=144)),
    ("heads_0", dict(heads=0)), ("width_2112", dict(heads=33)),
    ("queries_0", dict(queries=0)), ("queries_18", dict(queries=18)), ("queries_beyond_tokens", dict(tokens=3)),
    ("dtype_fp8", dict(dtype=vithip.DTYPE_FP8)), ("dtype_9", dict(dtype=9)),
    ("head_major_at_80", dict(hd=80, hm=256)),
    ("head_major_short", dict(hm=73)), ("head_major_negative", dict(hm=-1)),
    ("misaligned_qkv", dict(qkv=QKV + 8)), ("misaligned_probs", dict(probs=PROBS + 4)),
]
PROBS_SAME = [{"null_qkv", "null_probs"}, {"tokens_0", "tokens_4098"}, {"head_dim_72", "head_dim_144"}, {"heads_0", "width_2112"},
              {"queries_0", "queries_18", "queries_beyond_tokens"}, {"dtype_fp8", "dtype_9"}, {"head_major_short", "head_major_negative"},
              {"misaligned_qkv", "misaligned_probs"}]
READOUT_REFUSALS = [
    ("null_store", dict(store=None)),
    ("no_output", dict(out=None, mean=None)),
    ("batch_0", dict(batch=0)),
    ("heads_0", dict(heads=0)), ("heads_65", dict(heads=65)),
    ("tokens_0", dict(tokens=0, lead=0)), ("tokens_4098", dict(tokens=4098)),
    ("queries_0", dict(queries=0)), ("queries_18", dict(queries=18)), ("queries_beyond_tokens", dict(tokens=4, lead=1)),
    ("lead_minus_1", dict(lead=-1)), ("lead_is_tokens", dict(lead=37)),
    ("elem_u8", dict(elem=vithip.ELEM_U8)),
    ("keys_2", dict(keys=2)),
    ("misaligned_store", dict(store=STORE + 4)), ("misaligned_out", dict(out=OUT + 2)), ("misaligned_mean", dict(mean=MEAN + 8)),
]
READOUT_SAME = [{"heads_0", "heads_65"}, {"tokens_0", "tokens_4098"}, {"queries_0", "queries_18", "queries_beyond_tokens"},
                {"lead_minus_1", "lead_is_tokens"}, {"misaligned_store", "misaligned_out", "misaligned_mean"}]


def message(tap, kw):
    with pytest.raises(vithip.VhError) as e:
        tap(**kw)
    assert e.value.code == VH_ERR_INVALID, str(e.value)
    return str(e.value)


def strip_numbers(m):
    return re.sub(r"0x[0-9a-f]+|\(nil\)|-?\d+", "#", m)


def distinct(tap, refusals, same):
    groups = {}
    for n, kw in refusals:
        groups.setdefault(strip_numbers(message(tap, kw)), set()).add(n)
    # one message per kind of refusal: names share a message only where they are the same refusal
    for names in groups.values():
        assert len(names) == 1 or any(names <= s for s in same), names
    return groups


@pytest.mark.parametrize("name,kw", PROBS_REFUSALS, ids=[n for n, _ in PROBS_REFUSALS])
def test_probs_tap_refuses_before_touching_a_device(name, kw):
    assert "attention_probs" in message(probs_tap, kw)


@pytest.mark.parametrize("name,kw", READOUT_REFUSALS, ids=[n for n, _ in READOUT_REFUSALS])
def test_readout_tap_refuses_before_touching_a_device(name, kw):
    assert "attention_readout" in message(readout_tap, kw)


def test_every_kind_of_refusal_has_a_message_of_its_own():
    g = distinct(probs_tap, PROBS_REFUSALS, PROBS_SAME)
    assert len(g) == len(PROBS_SAME) + 2        # the shared ones + batch_0 and head_major_at_80, each on its own
    # the shared ones + null_store, no_output, batch_0, elem_u8 and keys_2
    assert len(distinct(readout_tap, READOUT_REFUSALS, READOUT_SAME)) == len(READOUT_SAME) + 5
    assert "head_dim 64 only" in message(probs_tap, dict(hd=80, hm=256)) and "fewer than batch * tokens" in message(probs_tap, dict(hm=73))
    assert "16-byte aligned" in message(probs_tap, dict(probs=PROBS + 4)) and "VH_DTYPE_BF16 or VH_DTYPE_FP16" in message(probs_tap, dict(dtype=9))


def test_context_calls_fail_loudly_without_a_context():
    L = vithip.lib()
    desc = vithip.AttentionMaps(None, None, vithip.ELEM_F32, -1, vithip.ATTN_KEYS_ALL, 0)
    n = C.c_int(0)
    for rc in (L.vh_set_attention_layers(None, None, 0, 0), L.vh_get_attention_layers(None, None, C.byref(n), None),
               L.vh_attention_dims(None, None, None, None, None, None), L.vh_read_attention(None, C.byref(desc)),
               L.vh_read_attention_device(None, C.byref(desc)), L.vh_read_attention_device_async(None, C.byref(desc))):
        assert rc == VH_ERR_INVALID
        assert b"null" in L.vh_last_error(None)


# ---- the references -----------------------------------------------------------------------------------------------------------
def test_readout_emulation():
    rng = np.random.default_rng(5)
    store = rng.random((2, 3, 2, 9), dtype=np.float32)
    p, m = AM.readout(store, 2, vithip.ELEM_F32, vithip.ATTN_KEYS_PATCH)
    assert p.shape == (2, 3, 2, 7) and m.shape == (2, 2, 7) and AM.same_bits(p, store[..., 2:])
    want = ((np.float32(0) + store[:, 0, :, 2:]) + store[:, 1, :, 2:] + store[:, 2, :, 2:]) * np.float32(1.0 / 3)
    assert AM.same_bits(m, want.astype(np.float32))
    for elem, dt in ((vithip.ELEM_F16, vithip.DTYPE_FP16), (vithip.ELEM_BF16, vithip.DTYPE_BF16)):
        p16, m16 = AM.readout(store, 2, elem, vithip.ATTN_KEYS_ALL)
        assert p16.dtype == np.uint16 and np.array_equal(p16, vithip.to16(store, dt)) and np.array_equal(m16, vithip.to16(AM.readout(store, 2, vithip.ELEM_F32, 0)[1], dt))
        assert np.abs(AM.widen(p16, elem) - store).max() <= 2.0 ** (-11 if elem == vithip.ELEM_F16 else -8)


def test_layer_probabilities_of_the_reference_model():
    """attn_maps_ref.layer_probs64 on a golden config against the same quantity written differently: per (image, head) loops, q and k
    from one stacked projection, exp2 of log2-domain scores."""
    cfg, flags, batch, Q = S.CONFIGS["vit_micro"], RR.FLAG_REGISTERS(2), 2, 3
    blob = RR.make_blob(cfg, 11, flags)
    images = S.make_images(cfg, 12, batch)
    _, _, hidden = RR.forward(cfg, blob, images, flags, all_hidden=True)
    t = RR.unpack_blob(cfg, blob, flags)
    D, H = cfg["dim"], cfg["heads"]
    hd, T = D // H, RR.tokens(cfg, flags)
    for k in (1, 2):
        got = AM.layer_probs64(cfg, blob, hidden, k, batch, Q, flags)
        assert got.shape == (batch, H, Q, T) and np.abs(got.sum(-1) - 1).max() < 1e-13
        w = np.concatenate([t[f"l{k - 1}.q.weight"], t[f"l{k - 1}.k.weight"]]).astype(np.float64)
        b = np.concatenate([t[f"l{k - 1}.q.bias"], t[f"l{k - 1}.k.bias"]]).astype(np.float64)
        x = hidden[k - 1].astype(np.float64)
        mu = x.mean(1, keepdims=True)
        y = (x - mu) / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + 1e-6) * t[f"l{k - 1}.ln1.weight"] + t[f"l{k - 1}.ln1.bias"]
        qk = y @ w.T + b
        for i in range(batch):
            for h in range(H):
                q = qk[i * T:i * T + Q, h * hd:(h + 1) * hd] * (AM.LOG2E / np.sqrt(hd))
                kk = qk[i * T:(i + 1) * T, D + h * hd:D + (h + 1) * hd]
                s = q @ kk.T
                e = np.exp2(s - s.max(1, keepdims=True))
                assert np.abs(got[i, h] - e / e.sum(1, keepdims=True)).max() < 1e-12, (k, i, h)
