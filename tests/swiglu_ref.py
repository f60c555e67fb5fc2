"""The reference of the SwiGLU model switch (TEST INFRASTRUCTURE), on top of vit_ref, which it does not change: the tensor table with
the doubled fc1, its own pack_blob / unpack_blob, a forward that reuses vit_ref.layer with the gate as the layer's activation, the
16-bit emulation of the device's two extra rounding points, and the recipes of the tests/golden/swiglu fixtures.

  SWIGLU   mlp_dim = M is the gated width.  l{l}.fc1.weight is [2 M][D], l{l}.fc1.bias [2 M]: rows 0 .. M - 1 the gate, M .. 2 M - 1 the
           value.  With z = LN2(x) W1^T + b1, g = z[:, :M], u = z[:, M:]:   x += (silu(g) * u) W2^T + b2,  silu(g) = g sigmoid(g).
           Header bit 25, the flag's own position.  Seeded: the longer tensors from vit_ref's tensor ids (the same streams, longer).
           Excludes QUICK_GELU, TANH_GELU, MAP_HEAD, CLS_TAIL (and, on the device, W8_E4M3 and the fp8 dtype).

q16 (a function that rounds an array to the 16-bit storage type) emulates what the device rounds beyond vit_ref's q16 points: fc1
stores z as 16-bit, the gate pass computes in fp32 from the stored g and u and rounds h once.  Nothing else is rounded here.
"""
from __future__ import annotations

import numpy as np

import vh_synth as S
import vit_ref as R

FLAG_SWIGLU = 1 << 25
EXCLUDES = R.FLAG_QUICK_GELU | R.FLAG_TANH_GELU | R.FLAG_MAP_HEAD | R.CLS_TAIL


def legal(cfg, flags):
    if not flags & FLAG_SWIGLU:
        return R.legal(cfg, flags)
    return not flags & EXCLUDES and R.legal(cfg, flags & ~FLAG_SWIGLU)


def tensor_table(cfg, flags=0):
    """vit_ref.tensor_table with fc1 of every layer [2 M][D] + [2 M] under SWIGLU (ids, sigmas and offsets kept)."""
    out = []
    for name, shape, tid, sigma, off in R.tensor_table(cfg, flags & ~FLAG_SWIGLU):
        if flags & FLAG_SWIGLU and name.startswith("l") and ".fc1." in name:
            shape = (2 * shape[0],) + tuple(shape[1:])
        out.append((name, tuple(shape), tid, sigma, off))
    return out


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = R.blob_header(cfg, flags & ~FLAG_SWIGLU, ln_eps)
    bits = int(h[52:56].view(np.uint32)[0]) | (flags & FLAG_SWIGLU)
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def make_tensors(cfg, seed, flags=0):
    t = {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape)
         for name, shape, tid, sigma, off in tensor_table(cfg, flags) if tid != R.TID_ROPE}
    if flags & R.FLAG_ROPE:
        t["rope.cos"], t["rope.sin"] = R.seeded_tables(cfg, seed)
    return t


def pack_blob(cfg, tensors, flags=0, ln_eps=1e-6):
    parts = [blob_header(cfg, flags, ln_eps)]
    for name, shape, *_ in tensor_table(cfg, flags):
        a = np.ascontiguousarray(tensors[name], dtype=np.float32)
        assert a.shape == tuple(shape), (name, a.shape, shape)
        parts.append(a.reshape(-1).view(np.uint8))
    return np.concatenate(parts)


def make_blob(cfg, seed, flags=0, ln_eps=1e-6):
    return pack_blob(cfg, make_tensors(cfg, seed, flags), flags, ln_eps)


def unpack_blob(cfg, blob, flags=0):
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    assert blob.size == blob_bytes(cfg, flags), (blob.size, blob_bytes(cfg, flags))
    out, off = {}, 64
    for name, shape, *_ in tensor_table(cfg, flags):
        n = int(np.prod(shape))
        out[name] = blob[off:off + 4 * n].view(np.float32).reshape(shape)
        off += 4 * n
    return out


def with_bit(blob, on):
    """The same bytes with header bit 25 forged on or off."""
    out = np.ascontiguousarray(blob, dtype=np.uint8).copy()
    bits = int(out[52:56].view(np.uint32)[0])
    out[52:56] = np.array([bits | FLAG_SWIGLU if on else bits & ~FLAG_SWIGLU], dtype=np.uint32).view(np.uint8)
    return out


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def silu(g):
    """g sigmoid(g), overflow-free for every finite g (float64 or float32 in, same type out)."""
    g = np.asarray(g)
    z = np.exp(-np.abs(g))
    return np.where(g >= 0, g / (1 + z), g * z / (1 + z))


def gate(M, q16=None):
    """The layer's activation over the whole fc1 output z [rows, 2 M] -> h [rows, M].  q16: z is rounded as fc1 stores it, the product is
    formed from the stored values in z's float type, and h is rounded once."""
    def act(z):
        if q16 is not None:
            z = q16(z).astype(z.dtype)
        h = silu(z[:, :M]) * z[:, M:]
        return q16(h).astype(z.dtype) if q16 is not None else h
    return act


def forward(cfg, blob, images, flags=FLAG_SWIGLU, ln_eps=1e-6, dtype=np.float64, q16=None, want_hidden=False, all_hidden=False,
            want_head=False, n_layers=-1, qkv16=None):
    """vit_ref.forward for a SWIGLU model (`blob`: the blob or its tensors): logits [batch, classes], then what is asked for, in
    vit_ref.forward's order.  q16 rounds z and h (the module docstring) and nothing else; qkv16 is vit_ref.forward's q16 (q|k|v).  Without
    the flag this is vit_ref.forward."""
    if not flags & FLAG_SWIGLU:
        return R.forward(cfg, blob, images, flags, ln_eps, dtype, n_layers, want_hidden, all_hidden=all_hidden, want_head=want_head, q16=qkv16)
    assert legal(cfg, flags), hex(flags)
    t = {k: np.asarray(v).astype(dtype) for k, v in (blob if isinstance(blob, dict) else unpack_blob(cfg, blob, flags)).items()}
    D, H, M = cfg["dim"], cfg["heads"], cfg["mlp_dim"]
    dh = D // H
    images = np.asarray(images, dtype=dtype)
    batch = images.shape[0]
    x = R.assemble(R.patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    assert T == R.tokens(cfg, flags & ~FLAG_SWIGLU)
    lead = T - (S.tokens(cfg) - 1)
    rope = (t["rope.cos"], t["rope.sin"], lead) if flags & R.FLAG_ROPE else None
    x = x.reshape(batch * T, D)
    if flags & R.FLAG_PRE_LN:
        x = R.layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    hidden = [x]
    act = gate(M, q16)
    for l in range(cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])):
        x = R.layer(x, lambda n: t[f"l{l}.{n}"], act, batch, T, H, dh, ln_eps, None, rope, qkv16)
        hidden.append(x)
    hin = R.head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, R.pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden or all_hidden else ()) + ((hidden,) if all_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


# ---- the fixtures (tests/golden/swiglu, written by tests/golden/make_golden_swiglu.py) -----------------------------------------------
# name: (kind, config without classes; mlp_dim is the BLOB's, hidden width of the checkpoint, registers, weight seed, image seed, batch)
A = dict(image_size=28, patch_size=14, channels=3, dim=128, heads=2, mlp_dim=384, layers=2)    # DINOv2, the plain loop; 344 padded to 384
B = dict(image_size=28, patch_size=14, channels=3, dim=256, heads=4, mlp_dim=768, layers=2)    # DINOv2 with registers, the folded loop; 688 padded to 768
Cc = dict(image_size=24, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2)    # DINOv3: RoPE + the gated MLP, no padding
FIXTURES = {"a": ("dinov2", A, 344, 0, 201, 202, 3), "b": ("dinov2", B, 688, 4, 203, 204, 2), "c": ("dinov3", Cc, 512, 4, 205, 206, 2)}
EPS = {"dinov2": 1e-6, "dinov3": 1e-5}
TID_LAMBDA = 0x7040     # LayerScale: lambda1 of layer l = id 0x7040 + 2 l, lambda2 = + 1; 1 + 0.3 sigma: a spread, so that the fold is tested
TID_VALUE = 0x7050      # the value half of fc1 as the checkpoint holds it: weight id 0x7050 + 2 l, bias + 1 (the gate half keeps vit_ref's ids)
QK_SCALE_C = 1.75       # model c: q and k weights as hf_state_dicts.QK_SCALE["a"] (the same shape), so that the positions matter


def fixture_cfg(name):
    """The fixture's model as a cfg dict: identity head (classes = dim), so that the logits are the model's pooler_output."""
    return dict(FIXTURES[name][1], classes=FIXTURES[name][1]["dim"], registers=FIXTURES[name][3])


def fixture_eps(name):
    return EPS[FIXTURES[name][0]]


def fixture_flags(name):
    kind, _, _, regs, *_ = FIXTURES[name]
    return FLAG_SWIGLU | R.FLAG_REGISTERS(regs) | (R.FLAG_ROPE if kind == "dinov3" else 0)


def fixture_images(name):
    return S.make_images(fixture_cfg(name), FIXTURES[name][5], FIXTURES[name][6])


def fixture_model_tensors(name):
    """The checkpoint's tensors under our names, before LayerScale, at the CHECKPOINT's hidden width Mc: vit_ref's seeded tensors of that
    shape, fc1 = the gate half, plus l{l}.up.{weight, bias} = the value half from ids of this module's own."""
    kind, cfg0, Mc, regs, wseed, *_ = FIXTURES[name]
    cfg = dict(fixture_cfg(name), mlp_dim=Mc)
    t = R.make_tensors(cfg, wseed, R.FLAG_REGISTERS(regs))
    for l in range(cfg["layers"]):
        t[f"l{l}.up.weight"] = S.fill(Mc * cfg["dim"], wseed, TID_VALUE + 2 * l, 1, 0.02, 0.0).reshape(Mc, cfg["dim"])
        t[f"l{l}.up.bias"] = S.fill(Mc, wseed, TID_VALUE + 2 * l + 1, 1, 0.02, 0.0)
        if kind == "dinov3":
            for n in ("q", "k"):
                t[f"l{l}.{n}.weight"] = t[f"l{l}.{n}.weight"] * np.float32(QK_SCALE_C)
    return t


def lambdas(name, l):
    D, wseed = FIXTURES[name][1]["dim"], FIXTURES[name][4]
    return [S.fill(D, wseed, TID_LAMBDA + 2 * l + i, 1, 0.3, 1.0) for i in (0, 1)]


def fixture_state_dict(name):
    """The seeded state dict of fixture `name` under Hugging Face's names: Dinov2Model / Dinov2WithRegistersModel with use_swiglu_ffn
    (mlp.weights_in = gate rows, then value rows; mlp.weights_out), or DINOv3ViTModel with use_gated_mlp (mlp.gate_proj, up_proj,
    down_proj).  Weights are regenerated from the seed, not stored."""
    kind, _, Mc, regs, *_ = FIXTURES[name]
    cfg = fixture_cfg(name)
    D = cfg["dim"]
    t = fixture_model_tensors(name)
    e = "embeddings."
    sd = {e + "cls_token": t["cls"].reshape(1, 1, D)}
    if regs:
        sd[e + "register_tokens"] = t["reg"].reshape(1, regs, D)
    if kind == "dinov2":
        sd[e + "mask_token"] = np.zeros((1, D), np.float32)
        sd[e + "position_embeddings"] = t["pos"].reshape(1, -1, D)
        sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
        prefix, final = "encoder.layer.", "layernorm."
        names = (("ln1", "norm1"), ("q", "attention.attention.query"), ("k", "attention.attention.key"), ("v", "attention.attention.value"),
                 ("o", "attention.output.dense"), ("ln2", "norm2"), ("fc2", "mlp.weights_out"))
    else:
        sd[e + "mask_token"] = np.zeros((1, 1, D), np.float32)
        sd[e + "patch_embeddings.weight"], sd[e + "patch_embeddings.bias"] = t["patch.weight"], t["patch.bias"]
        prefix, final = "model.layer.", "norm."
        names = (("ln1", "norm1"), ("q", "attention.q_proj"), ("k", "attention.k_proj"), ("v", "attention.v_proj"), ("o", "attention.o_proj"),
                 ("ln2", "norm2"), ("fc1", "mlp.gate_proj"), ("up", "mlp.up_proj"), ("fc2", "mlp.down_proj"))
    for l in range(cfg["layers"]):
        b = f"{prefix}{l}."
        for ours, theirs in names:
            for wb in ("weight", "bias"):
                sd[f"{b}{theirs}.{wb}"] = t[f"l{l}.{ours}.{wb}"]
        if kind == "dinov2":
            sd[b + "mlp.weights_in.weight"] = np.concatenate([t[f"l{l}.fc1.weight"], t[f"l{l}.up.weight"]])
            sd[b + "mlp.weights_in.bias"] = np.concatenate([t[f"l{l}.fc1.bias"], t[f"l{l}.up.bias"]])
        sd[b + "layer_scale1.lambda1"], sd[b + "layer_scale2.lambda1"] = lambdas(name, l)
    sd[final + "weight"], sd[final + "bias"] = t["lnf.weight"], t["lnf.bias"]
    return sd


def fixture_tensors64(name, rope_cos=None, rope_sin=None):
    """The fixture's model under our names in float64 with NOTHING rounded on the way, at the BLOB's width: fc1 = gate rows, value rows,
    each zero-padded to mlp_dim; LayerScale folded into o and fc2 in float64 (the converter rounds that product to fp32); fc2's padding
    columns zero; the identity head; for DINOv3 pos zeros and the given tables (the model's own)."""
    kind, _, Mc, *_ = FIXTURES[name]
    cfg = fixture_cfg(name)
    D, M, h = cfg["dim"], cfg["mlp_dim"], cfg["dim"] // cfg["heads"] // 2
    t = {k: np.asarray(v, np.float64) for k, v in fixture_model_tensors(name).items()}
    t["head.weight"], t["head.bias"] = np.eye(D), np.zeros(D)
    if kind == "dinov3":
        t["pos"] = np.zeros_like(t["pos"])
        t["rope.cos"], t["rope.sin"] = np.asarray(rope_cos, np.float64)[:, :h], np.asarray(rope_sin, np.float64)[:, :h]
    for l in range(cfg["layers"]):
        l1, l2 = (np.asarray(v, np.float64) for v in lambdas(name, l))
        t[f"l{l}.o.weight"], t[f"l{l}.o.bias"] = t[f"l{l}.o.weight"] * l1[:, None], t[f"l{l}.o.bias"] * l1
        w1, b1, w2 = np.zeros((2 * M, D)), np.zeros(2 * M), np.zeros((D, M))
        w1[:Mc], w1[M:M + Mc] = t[f"l{l}.fc1.weight"], t.pop(f"l{l}.up.weight")
        b1[:Mc], b1[M:M + Mc] = t[f"l{l}.fc1.bias"], t.pop(f"l{l}.up.bias")
        w2[:, :Mc] = t[f"l{l}.fc2.weight"] * l2[:, None]
        t[f"l{l}.fc1.weight"], t[f"l{l}.fc1.bias"], t[f"l{l}.fc2.weight"], t[f"l{l}.fc2.bias"] = w1, b1, w2, t[f"l{l}.fc2.bias"] * l2
    return t


def fixture_blob(name):
    """The converter's blob of the fixture's state dict, with the identity head: logits = pooler_output."""
    import vithip
    cfg = fixture_cfg(name)
    D = cfg["dim"]
    head = (np.eye(D, dtype=np.float32), np.zeros(D, np.float32))
    conv = vithip.blob_from_dinov2_state_dict if FIXTURES[name][0] == "dinov2" else vithip.blob_from_dinov3_state_dict
    return conv(fixture_state_dict(name), cfg, ln_eps=fixture_eps(name), head=head, swiglu=True)
