"""GPU parity of attention with an additive per-head bias (VH_FLAG_ATTN_BIAS, kernels_attn_bias.hip): the tap against a plain
float64 softmax attention with the bias added (written here), a mask that only the rescale path can absorb, a zero bias against the
unbiased kernel's bits, and whole models on both layer loops.  Bounds: test_gpu_head_dim's ATT_TOL for the operator (the roundings are
the same: 16-bit P and O) and its model bounds (test_gpu_vit's) for the logits."""
import numpy as np
import pytest

import vh_synth as S
import vit_ref as R
from test_gpu_head_dim import ATT_TOL, DT, MODEL_TOL, NAME, _cfg, make_qkv
from vh_testlib import _release_buffers, dev, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
SHAPES = ((1, 2, 2), (33, 2, 3), (197, 2, 2), (289, 1, 2))   # (tokens, batch, heads): one key, a tile edge, seven tiles, two query slabs


def ref_attention(qkv, bias, batch, T, H, hd):
    """softmax(q k^T / sqrt(hd) + bias[h]) v in float64; qkv [batch * T][3 H hd] with q unscaled, bias [H][T][T] or None."""
    D = H * hd
    q, k, v = (np.asarray(qkv, np.float64)[:, i * D:(i + 1) * D].reshape(batch, T, H, hd).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(np.float64(hd))
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[None]
    p = np.exp(s - s.max(-1, keepdims=True))
    return ((p / p.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(batch * T, D)


def run_bias(pre, bias, batch, tokens, heads, hd, dt):
    image = dev(np.zeros(vithip.attention_bias_image_bytes(heads, tokens), dtype=np.uint8))
    vithip.op_attention_bias_image(dev(np.ascontiguousarray(bias, dtype=np.float32)).ptr, heads, tokens, image.ptr)
    out = dev(np.full(batch * tokens * heads * hd * 2, 0xFF, dtype=np.uint8))   # an unwritten element reads back as NaN
    vithip.op_attention_bias(dev(vithip.to16(pre, dt)).ptr, batch, tokens, heads, hd, image.ptr, out.ptr, dt)
    return out.to_numpy(np.uint16, (batch * tokens, heads * hd))


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", [32, 64, 80, 128])
def test_biased_attention_tap_matches_the_float64_reference(hd, dt):
    for tokens, batch, heads in SHAPES:
        pre, qkv = make_qkv(batch, tokens, heads, hd, dt, 41)
        bias = (2.0 * S.fill(heads * tokens * tokens, 43, tokens + hd, 0)).reshape(heads, tokens, tokens)   # spread 2, every entry its own
        ref = ref_attention(qkv, bias, batch, tokens, heads, hd)
        assert np.isfinite(ref).all()
        if tokens > 1:   # (one key: the softmax is 1 whatever the bias) the bias cannot be ignored and pass
            assert rel(ref_attention(qkv, None, batch, tokens, heads, hd), ref) > 10 * ATT_TOL[dt]
        got = vithip.from16(run_bias(pre, bias, batch, tokens, heads, hd, dt), dt)
        err = rel(got, ref)
        print(f"hd {hd} {NAME[dt]} tokens {tokens}: rel {err:.3e} (bound {ATT_TOL[dt]:g})")
        assert np.isfinite(got).all() and err <= ATT_TOL[dt], (hd, tokens, batch, heads, err)


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", [64, 80])
def test_bias_masks_through_the_rescale_path(hd, dt):
    # every row's first two key tiles sit at -1e4, so its tile-0 shift is ~1e4 below its later scores: the deferred rescale must run;
    # one late key per row carries +8 and takes essentially all of the row's weight
    tokens, batch, heads = 197, 1, 2
    pre, qkv = make_qkv(batch, tokens, heads, hd, dt, 45)
    late = 64 + (np.arange(tokens) * 7) % (tokens - 64)
    bias = np.zeros((heads, tokens, tokens), np.float32)
    bias[:, :, :64] = -1e4
    bias[:, np.arange(tokens), late] = 8.0
    ref = ref_attention(qkv, bias, batch, tokens, heads, hd)
    got = vithip.from16(run_bias(pre, bias, batch, tokens, heads, hd, dt), dt)
    assert np.isfinite(got).all() and rel(got, ref) <= ATT_TOL[dt], rel(got, ref)
    # each row sits on the V row of its late key: as near as the float64 softmax itself is (+8 leaves the row's other 132 unmasked
    # keys a few per cent of the weight, so that distance is no few ulp) plus a few ulp of the storage type
    ulp = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    v = qkv[:, 2 * heads * hd:].reshape(tokens, heads, hd)
    want = v[late, :, :].reshape(tokens, heads * hd)
    slack = np.abs(ref - want).max()
    assert np.abs(got - want).max() <= slack + 4 * ulp * np.abs(want).max() + 1e-6


@pytest.mark.parametrize("hd", [48, 64, 128])
def test_zero_bias_gives_the_unbiased_kernels_bits(hd):
    tokens, batch, heads = 197, 2, 2
    for dt in DT:
        pre, _ = make_qkv(batch, tokens, heads, hd, dt, 47)
        out = dev(np.full(batch * tokens * heads * hd * 2, 0xFF, dtype=np.uint8))
        vithip.op_attention_hd(dev(vithip.to16(pre, dt)).ptr, batch, tokens, heads, hd, out.ptr, dt)
        want = out.to_numpy(np.uint16, (batch * tokens, heads * hd))
        got = run_bias(pre, np.zeros((heads, tokens, tokens), np.float32), batch, tokens, heads, hd, dt)
        assert np.array_equal(got, want), (hd, NAME[dt], int((got != want).sum()))


def ref_forward(cfg, blob, images, flags):
    """float64 forward of a FLAG_ATTN_BIAS blob from vit_ref's pieces plus the biased attention above."""
    plain = flags & ~vithip.FLAG_ATTN_BIAS
    D, H, L = cfg["dim"], cfg["heads"], cfg["layers"]
    T = R.tokens(cfg, plain)
    t = {k: v.astype(np.float64) for k, v in R.unpack_blob(cfg, blob[:R.blob_bytes(cfg, plain)], plain).items()}
    bias = blob[R.blob_bytes(cfg, plain):].view(np.float32).reshape(L, H, T, T)
    images = np.asarray(images, np.float64)
    batch = len(images)
    x = R.assemble(R.patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg")).reshape(batch * T, D)
    for l in range(L):
        p = lambda n: t[f"l{l}.{n}"]
        y = R.layernorm(x, p("ln1.weight"), p("ln1.bias"), 1e-6)
        qkv = y @ np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")]).T + np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
        x = x + ref_attention(qkv, bias[l], batch, T, H, D // H) @ p("o.weight").T + p("o.bias")
        y = R.layernorm(x, p("ln2.weight"), p("ln2.bias"), 1e-6)
        x = x + R.gelu(y @ p("fc1.weight").T + p("fc1.bias")) @ p("fc2.weight").T + p("fc2.bias")
    hin = R.head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], 1e-6, 1, R.pool_of(plain))
    return hin @ t["head.weight"].T + t["head.bias"]


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
@pytest.mark.parametrize("cfg", [_cfg(96, 16, 256, 4, 512, 2), _cfg(64, 16, 320, 4, 640, 2)], ids=["d256_hd64_folded", "d320_hd80_plain"])
def test_whole_model_with_attention_bias(cfg, dt):
    pool = vithip.FLAG_POOL(vithip.POOL_AVG_FCNORM)
    flags = vithip.FLAG_ATTN_BIAS | pool
    images = S.make_images(cfg, 52, 3)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=3, flags=flags)
    ctx.init_weights_seeded(51)
    blob = ctx.export_weights()
    ref = ref_forward(cfg, blob, images, flags)
    got = ctx.forward(images)
    one = ctx.forward(images[:1])
    with pytest.raises(vithip.VhError, match="VH_FLAG_ATTN_BIAS context's maps would leave the bias out"):
        ctx.set_attention_layers([1])
    ctx.set_graph(True)
    replays = [ctx.forward(images) for _ in range(3)]
    ctx.close()
    err = rel(got, ref)
    print(f"{NAME[dt]}: logits rel {err:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and err <= MODEL_TOL[dt], err
    assert np.array_equal(one[0].view(np.uint32), got[0].view(np.uint32))
    for r in replays:
        assert np.array_equal(r.view(np.uint32), got.view(np.uint32))
    # the same weights without the flag (the blob minus its last tensor, header bit cleared) give other logits
    nb = blob[:R.blob_bytes(cfg, pool)].copy()
    nb[52:56] = np.array([pool], np.uint32).view(np.uint8)
    plain = vithip.VitContext(cfg, dtype=dt, max_batch=3, flags=pool)
    plain.load_weights(nb)
    off = plain.forward(images)
    plain.close()
    assert rel(off, got) > 10 * MODEL_TOL[dt], rel(off, got)
