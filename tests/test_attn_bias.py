"""VH_FLAG_ATTN_BIAS without a GPU: the flag in the header and the binding, the blob's size, the refusals and their messages, the taps'
host-side argument checks, BEiT's relative-position index against a literal double loop, and the BEiT converter against a float64 fold."""
import os

import numpy as np
import pytest

import vit_ref as R
from vh_testlib import lib_blob_bytes, vit_cfg

vithip = pytest.importorskip("vithip")
BIAS = vithip.FLAG_ATTN_BIAS
MICRO = vit_cfg(32, 16, 64, 2, 128, 2, 8)   # 5 tokens, head dim 32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vithip.h")


def test_bit_27_in_the_header_and_the_binding():
    text = open(HEADER).read()
    assert "#define VH_FLAG_ATTN_BIAS (1 << 27)" in text and BIAS == 1 << 27
    for sym in ("vh_attention_bias_image_bytes", "vh_op_attention_bias_image", "vh_op_attention_bias"):
        assert sym in vithip.SYMBOLS and sym + "(" in text and hasattr(vithip.lib(), sym)


def test_the_blob_grows_by_the_bias_tensor():
    T = 5
    assert lib_blob_bytes(MICRO, BIAS) == lib_blob_bytes(MICRO, 0) + 4 * MICRO["layers"] * MICRO["heads"] * T * T
    table = vithip.blob_tensor_table(MICRO, BIAS | vithip.FLAG_ROPE)
    assert table[-1] == ("attn_bias", (2, 2, T, T)) and table[-2][0] == "rope.sin"


@pytest.mark.parametrize("flags, dtype, message", [
    (BIAS | vithip.FLAG_CLS_TAIL, vithip.DTYPE_BF16, "VH_FLAG_ATTN_BIAS excludes VH_FLAG_CLS_TAIL"),
    (BIAS, vithip.DTYPE_FP8, "VH_FLAG_ATTN_BIAS excludes VH_DTYPE_FP8"),
    (BIAS | 1 << 26, vithip.DTYPE_BF16, "unknown bits in flags"),
    (BIAS | 1 << 28, vithip.DTYPE_BF16, "unknown bits in flags"),
])
def test_refusals_arrive_with_their_own_message(flags, dtype, message):
    cfg = vit_cfg(32, 16, 128, 2, 128, 2, 8)   # (dims of 128: the fp8 case reaches the flag rule)
    assert lib_blob_bytes(cfg, flags, dtype) == 0
    with pytest.raises(vithip.VhError, match=message):
        vithip.VitContext(cfg, dtype=dtype, max_batch=1, flags=flags)


def test_the_taps_check_their_arguments_on_the_host():
    ok = 4096   # an aligned non-null "device" address: every call below is refused before a device is touched
    assert vithip.attention_bias_image_bytes(12, 197) == 12 * 7 * 7 * 4096
    assert vithip.attention_bias_image_bytes(2, 0) == 0 and vithip.attention_bias_image_bytes(2, 4098) == 0
    for args, message in (((None, 2, 5, ok), "null pointer"), ((ok, 2, 5, ok + 8), "aligned"), ((ok, 2, 0, ok), "tokens 0 outside"),
                          ((ok, 2, 4098, ok), "tokens 4098 outside")):
        with pytest.raises(vithip.VhError, match=message):
            vithip.op_attention_bias_image(*args)
    for args, message in (((ok, 1, 5, 2, 32, None, ok, vithip.DTYPE_BF16), "null pointer"),
                          ((ok + 2, 1, 5, 2, 32, ok, ok, vithip.DTYPE_BF16), "aligned"),
                          ((ok, 1, 0, 2, 32, ok, ok, vithip.DTYPE_BF16), "tokens outside"),
                          ((ok, 1, 4098, 2, 32, ok, ok, vithip.DTYPE_BF16), "tokens outside"),
                          ((ok, 1, 5, 2, 72, ok, ok, vithip.DTYPE_BF16), "head_dim must be"),
                          ((ok, 1, 5, 2, 32, ok, ok, vithip.DTYPE_FP8), "VH_DTYPE_FP8 is not supported")):
        with pytest.raises(vithip.VhError, match=message):
            vithip.op_attention_bias(*args)


@pytest.mark.parametrize("g", [2, 3])
def test_relative_position_bias_equals_a_literal_double_loop(g):
    n, H, T = (2 * g - 1) ** 2 + 3, 3, g * g + 1
    table = np.random.default_rng(g).standard_normal((n, H))
    want = np.empty((H, T, T))
    for q in range(T):
        for k in range(T):
            if q and k:
                row = ((q - 1) // g - (k - 1) // g + g - 1) * (2 * g - 1) + ((q - 1) % g - (k - 1) % g + g - 1)
            else:
                row = n - 1 if q == k else n - 3 if q == 0 else n - 2
            want[:, q, k] = table[row]
    assert np.array_equal(vithip.beit_relative_position_bias(table, g), want)


@pytest.mark.parametrize("mean, shared", [(True, False), (False, True)])
def test_the_beit_converter_gives_the_tensors_of_a_float64_fold(mean, shared):
    cfg, g = MICRO, 2
    D, M, H, L, E, n = cfg["dim"], cfg["mlp_dim"], cfg["heads"], cfg["layers"], cfg["classes"], (2 * g - 1) ** 2 + 3
    rng = np.random.default_rng(7)
    w = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    sd = {"embeddings.cls_token": w(1, 1, D), "embeddings.mask_token": w(1, 1, D), "embeddings.patch_embeddings.projection.weight": w(D, 3, 16, 16),
          "embeddings.patch_embeddings.projection.bias": w(D), ("pooler.layernorm." if mean else "layernorm.") + "weight": w(D),
          ("pooler.layernorm." if mean else "layernorm.") + "bias": w(D)}
    if shared:
        sd["encoder.relative_position_bias.relative_position_bias_table"] = w(n, H)
    for l in range(L):
        b = f"encoder.layer.{l}."
        for mod, shape in (("attention.attention.query", (D, D)), ("attention.attention.value", (D, D)), ("attention.output.dense", (D, D)),
                           ("intermediate.dense", (M, D)), ("output.dense", (D, M)), ("layernorm_before", (D,)), ("layernorm_after", (D,))):
            sd[b + mod + ".weight"], sd[b + mod + ".bias"] = w(*shape), w(shape[0])
        sd[b + "attention.attention.key.weight"] = w(D, D)
        sd[b + "lambda_1"], sd[b + "lambda_2"] = w(D), w(D)
        if not shared:
            sd[b + "attention.attention.relative_position_bias.relative_position_bias_table"] = w(n, H)
    sd = {"beit." + k: v for k, v in sd.items()}
    sd["classifier.weight"], sd["classifier.bias"] = w(E, D), w(E)
    blob = vithip.blob_from_beit_state_dict(sd, cfg)
    flags = BIAS | vithip.FLAG_POOL(vithip.POOL_AVG_FCNORM if mean else vithip.POOL_CLS)
    assert vithip.blob_flags_of(blob) == flags and blob.size == lib_blob_bytes(cfg, flags)
    plain = flags & ~BIAS
    t = R.unpack_blob(cfg, blob[:R.blob_bytes(cfg, plain)], plain)
    bias = blob[R.blob_bytes(cfg, plain):].view(np.float32).reshape(L, H, 5, 5)
    f64 = lambda k: sd["beit." + k].astype(np.float64)
    assert not t["pos"].any() and np.array_equal(t["head.weight"], sd["classifier.weight"])
    assert np.array_equal(t["lnf.weight"], sd["beit." + ("pooler.layernorm." if mean else "layernorm.") + "weight"])
    for l in range(L):
        b = f"encoder.layer.{l}."
        assert not t[f"l{l}.k.bias"].any() and np.array_equal(t[f"l{l}.k.weight"], sd["beit." + b + "attention.attention.key.weight"])
        assert np.array_equal(t[f"l{l}.o.weight"], (f64(b + "attention.output.dense.weight") * f64(b + "lambda_1")[:, None]).astype(np.float32))
        assert np.array_equal(t[f"l{l}.fc2.bias"], (f64(b + "output.dense.bias") * f64(b + "lambda_2")).astype(np.float32))
        table = f64("encoder.relative_position_bias.relative_position_bias_table" if shared
                    else b + "attention.attention.relative_position_bias.relative_position_bias_table")
        assert np.array_equal(bias[l], vithip.beit_relative_position_bias(table, g).astype(np.float32))
