"""The reference for the rotary model flag (TEST INFRASTRUCTURE): VH_FLAG_ROPE on top of tests/vit_ref.py and tests/siglip_ref.py, whose
patch_embed / assemble / layernorm / attention and blob tables are reused; the rotation, its two blob tensors and the header bit are
stated here, independently of include/vithip.h (tests/test_rope.py compares the two).

  ROPE  (1 << 23)  in every layer, q and k of the patch rows (row lead + p of an image is patch p; the lead rows -- class token,
        registers -- are left alone) are rotated per head: for d < hd / 2, c = rope.cos[p][d], s = rope.sin[p][d]
            out[d] = x[d] c - x[d + hd/2] s          out[d + hd/2] = x[d + hd/2] c + x[d] s
        (Hugging Face's rotate_half form).  v is not rotated.

Blob: siglip_ref's (= vit_ref's, then the map.* tensors where there are any), then -- ROPE -- at the very end rope.cos [NP][hd / 2] and
rope.sin [NP][hd / 2], fp32.  Seeded: the angle a[i] = pi * u[i], u = the generator's uniform stream of tensor id 0x7030; cos(a) and
sin(a) in float64, rounded once.  The header's flags word carries the bit at its flag position.

Rounding emulations of forward(): q16 = a function that rounds an array to the 16-bit storage type: q|k|v are rounded when the
projection stores them, and q and k of the patch rows once more behind the rotation (the device's two rounding points).  fp8 = "plain" /
"folded": vit_ref's emulation, with the bf16 rounding of q|k|v and the extra bf16 rounding behind the rotation.
"""
from __future__ import annotations

import math

import numpy as np

import siglip_ref as SR
import vh_synth as S
import vit_ref as R

FLAG_ROPE = 1 << 23
TID_ROPE = 0x7030
CLS_TAIL = 8


def old(flags):
    """The bits siglip_ref knows."""
    return int(flags) & ~FLAG_ROPE


def legal(cfg, flags):
    """The combinations vh_create accepts."""
    if flags & FLAG_ROPE and flags & CLS_TAIL:
        return False
    return SR.legal(cfg, old(flags))


# ---- layout -------------------------------------------------------------------------------------------------------------------
def rope_shape(cfg):
    g = cfg["image_size"] // cfg["patch_size"]
    return (g * g, cfg["dim"] // cfg["heads"] // 2)


def tensor_table(cfg, flags=0):
    """[(name, shape, tensor_id, sigma, offset)]; the two rope tensors share the id of their angle stream (sigma / offset unused)."""
    t = SR.tensor_table(cfg, old(flags))
    if flags & FLAG_ROPE:
        t = t + [("rope.cos", rope_shape(cfg), TID_ROPE, None, None), ("rope.sin", rope_shape(cfg), TID_ROPE, None, None)]
    return t


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = SR.blob_header(cfg, old(flags), ln_eps)
    bits = int(h[52:56].view(np.uint32)[0]) | (int(flags) & FLAG_ROPE)
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def seeded_tables(cfg, seed):
    shape = rope_shape(cfg)
    a = math.pi * S.fill(int(np.prod(shape)), seed, TID_ROPE, 0).astype(np.float64)
    return np.cos(a).astype(np.float32).reshape(shape), np.sin(a).astype(np.float32).reshape(shape)


def make_tensors(cfg, seed, flags=0):
    t = SR.make_tensors(cfg, seed, old(flags))
    if flags & FLAG_ROPE:
        t["rope.cos"], t["rope.sin"] = seeded_tables(cfg, seed)
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


def without_rope(cfg, blob, flags):
    """The same model with the flag cleared: the blob minus its last two tensors, the header bit cleared.  -> (blob, flags)"""
    assert flags & FLAG_ROPE
    n = 2 * 4 * int(np.prod(rope_shape(cfg)))
    out = np.ascontiguousarray(blob, dtype=np.uint8)[:-n].copy()
    bits = int(out[52:56].view(np.uint32)[0]) & ~FLAG_ROPE
    out[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return out, old(flags)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def rotate_rows(x, cos, sin):
    """x [..., NP, hd] in any float type, cos / sin [NP, hd / 2] -> the rotated rows, in x's type, every operation in that type."""
    h = x.shape[-1] // 2
    c, s = cos.astype(x.dtype), sin.astype(x.dtype)
    lo, hi = x[..., :h], x[..., h:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], -1)


def rotate_qkv(qkv, cos, sin, batch, T, H, dh, lead, q16=None):
    """Row-major q|k|v [batch * T, 3 H dh] -> the same with q and k of rows lead .. T - 1 of every image and head rotated (and, with
    q16, rounded once more); v and the lead rows are returned as they came."""
    out = qkv.reshape(batch, T, 3, H, dh).copy()
    rot = rotate_rows(out[:, lead:, :2].transpose(0, 2, 3, 1, 4), cos, sin)      # [batch, 2, H, NP, dh]
    if q16 is not None:
        rot = q16(rot).astype(qkv.dtype)
    out[:, lead:, :2] = rot.transpose(0, 3, 1, 2, 4)
    return out.reshape(batch * T, 3 * H * dh)


def layer(x, p, act, batch, T, H, dh, eps, rope, fp8=None, q16=None, want_qkv=False):
    """vit_ref.layer with the rotation between the projection and attention.  rope = (cos, sin, lead) or None."""
    wqkv = np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")])
    bqkv = np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
    if fp8:
        q16 = R.bf16
    if fp8 == "folded":
        qkv = R.ln_linear_f8_folded(x, p("ln1.weight"), p("ln1.bias"), wqkv, bqkv, eps)
    elif fp8:
        qkv = R.linear_f8(R.e4m3(R.layernorm(x, p("ln1.weight"), p("ln1.bias"), eps)), wqkv, bqkv)
    else:
        qkv = R.layernorm(x, p("ln1.weight"), p("ln1.bias"), eps) @ wqkv.T + bqkv
    if q16 is not None:
        qkv = q16(qkv).astype(x.dtype)
    if rope is not None:
        qkv = rotate_qkv(qkv, rope[0], rope[1], batch, T, H, dh, rope[2], q16)
    if want_qkv:
        return qkv
    att = R.attention(qkv, batch, T, H, dh)
    if fp8:
        x = x + R.linear_f8(R.e4m3(att), p("o.weight"), p("o.bias"))
        if fp8 == "folded":
            hid = R.e4m3(act(R.ln_linear_f8_folded(x, p("ln2.weight"), p("ln2.bias"), p("fc1.weight"), p("fc1.bias"), eps)))
        else:
            y = R.e4m3(R.layernorm(x, p("ln2.weight"), p("ln2.bias"), eps))
            hid = R.e4m3(act(R.linear_f8(y, p("fc1.weight"), p("fc1.bias")).astype(np.float32)))
        return (x + R.linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
    x = x + att @ p("o.weight").T + p("o.bias")
    y = R.layernorm(x, p("ln2.weight"), p("ln2.bias"), eps)
    return x + act(y @ p("fc1.weight").T + p("fc1.bias")) @ p("fc2.weight").T + p("fc2.bias")


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, want_head=False,
            q16=None, lead_probs=None):
    """siglip_ref.forward for every flag, ROPE included (`blob`: the blob, or its tensors as a dict of arrays of any float type, which
    need not have passed through fp32): logits [batch, classes], then -- when asked for -- the residual rows
    [batch * tokens, dim] after n_layers layers and the head's input [batch, W].
    lead_probs = (k, Q): instead, the softmax rows [batch][heads][Q][tokens] of the first Q queries of layer k (1-based)."""
    f = dtype if fp8 is None else np.float32
    t = {k: np.asarray(v).astype(f) for k, v in (blob if isinstance(blob, dict) else unpack_blob(cfg, blob, flags)).items()}
    D, H = cfg["dim"], cfg["heads"]
    dh = D // H
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = SR.activation(flags)
    x = R.assemble(R.patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    lead = T - (S.tokens(cfg) - 1)
    rope = (t["rope.cos"], t["rope.sin"], lead) if flags & FLAG_ROPE else None
    x = x.reshape(batch * T, D)
    if flags & SR.PRE:
        x = R.layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    nl = cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])
    for l in range(nl):
        p = lambda n: t[f"l{l}.{n}"]
        if lead_probs is not None and lead_probs[0] == l + 1:
            qkv = layer(x, p, act, batch, T, H, dh, ln_eps, rope, fp8, q16, want_qkv=True).reshape(batch, T, 3, H, dh)
            s = np.einsum("bqhd,bthd->bhqt", qkv[:, :lead_probs[1], 0], qkv[:, :, 1]) / math.sqrt(dh)
            e = np.exp(s - s.max(-1, keepdims=True))
            return e / e.sum(-1, keepdims=True)
        x = layer(x, p, act, batch, T, H, dh, ln_eps, rope, fp8, q16)
    assert lead_probs is None, "lead_probs names a layer that does not run"
    if flags & SR.FLAG_MAP_HEAD:
        y = R.layernorm(x.reshape(batch, T, D)[:, lead:], t["lnf.weight"], t["lnf.bias"], ln_eps)
        hin = SR.map_head(y, t, H, act, ln_eps)
    else:
        hin = R.head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, R.pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


def final_norm(cfg, blob, x, flags=0, ln_eps=1e-6):
    t = blob if isinstance(blob, dict) else unpack_blob(cfg, blob, flags)
    return R.layernorm(x, t["lnf.weight"].astype(x.dtype), t["lnf.bias"].astype(x.dtype), ln_eps)


def fp16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


# ---- the DINOv3 fixtures (tests/golden/dinov3, written by tests/golden/make_golden_dinov3.py) ----------------------------------------
# name: (config without classes, registers, key_bias, weight seed, image seed, batch)
A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2)      # hd 64: the fold + split path
B = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2)      # hd 64: the fp32-residual path
Cc = dict(image_size=24, patch_size=8, channels=3, dim=320, heads=4, mlp_dim=384, layers=2)     # hd 80 (dim is a multiple of 64), row-major, an odd 3 x 3 grid
FIXTURES = {"a": (A, 4, True, 101, 102, 3), "b": (B, 4, True, 103, 104, 3), "c": (Cc, 0, False, 105, 106, 2)}
DINOV3_EPS = 1e-5
# q.weight and k.weight are the seeded tensors times QK_SCALE[name]: attention sharp enough for the positions to matter (without the
# rotation the outputs move by 0.16 / 0.29 / 0.28 of their largest magnitude; at the plain sigma of 0.02, by 0.05 / 0.01 / 0.06), and no
# sharper: at 4 the 16-bit roundings of EVERY operand move model c by 1.3e-3 in fp16 (measured on the device), past the model bound, and at 2
# the fp16 attention rows of model a's second layer are 7.2e-5 from the reference, past the attention-map tolerance of 7.0e-5
QK_SCALE = {"a": 1.75, "b": 4.0, "c": 2.0}
TID_LAMBDA = 0x7040     # LayerScale: lambda1 of layer l = id 0x7040 + 2 l, lambda2 = + 1; 1 + 0.3 sigma: a spread, so that the fold is tested


def fixture_cfg(name):
    """The fixture's model as a cfg dict: identity head (classes = dim), so that the logits are the model's pooler_output."""
    cfg, R_, *_ = FIXTURES[name]
    return dict(cfg, classes=cfg["dim"], registers=R_)


def fixture_model_tensors(name):
    """The fixture's seeded tensors under our names, before LayerScale: vit_ref's, with q.weight and k.weight times QK_SCALE[name]."""
    cfg = fixture_cfg(name)
    t = R.make_tensors(cfg, FIXTURES[name][3], R.FLAG_REGISTERS(FIXTURES[name][1]))
    for l in range(cfg["layers"]):
        for n in ("q", "k"):
            t[f"l{l}.{n}.weight"] = t[f"l{l}.{n}.weight"] * np.float32(QK_SCALE[name])
    return t


def dinov3_state_dict(name, prefix="model.layer."):
    """The seeded state dict of fixture `name` under Hugging Face's DINOv3ViTModel names (weights are regenerated from the seed, not
    stored: a 256-wide model's fp32 weights are 4 MB).  o_proj / down_proj are the raw matrices; the LayerScale vectors are separate."""
    cfg0, R_, key_bias, wseed, *_ = FIXTURES[name]
    cfg = fixture_cfg(name)
    D = cfg["dim"]
    t = fixture_model_tensors(name)
    sd = {"embeddings.cls_token": t["cls"].reshape(1, 1, D), "embeddings.mask_token": np.zeros((1, 1, D), np.float32),
          "embeddings.patch_embeddings.weight": t["patch.weight"], "embeddings.patch_embeddings.bias": t["patch.bias"]}
    if R_:
        sd["embeddings.register_tokens"] = t["reg"].reshape(1, R_, D)
    names = (("ln1", "norm1"), ("q", "attention.q_proj"), ("k", "attention.k_proj"), ("v", "attention.v_proj"), ("o", "attention.o_proj"),
             ("ln2", "norm2"), ("fc1", "mlp.up_proj"), ("fc2", "mlp.down_proj"))
    for l in range(cfg["layers"]):
        for ours, theirs in names:
            for wb in ("weight", "bias"):
                if ours == "k" and wb == "bias" and not key_bias:
                    continue
                sd[f"{prefix}{l}.{theirs}.{wb}"] = t[f"l{l}.{ours}.{wb}"]
        for i in (1, 2):
            sd[f"{prefix}{l}.layer_scale{i}.lambda1"] = S.fill(D, wseed, TID_LAMBDA + 2 * l + i - 1, 1, 0.3, 1.0)
    sd["norm.weight"], sd["norm.bias"] = t["lnf.weight"], t["lnf.bias"]
    return sd


def fixture_images(name):
    _, _, _, _, iseed, batch = FIXTURES[name]
    return S.make_images(fixture_cfg(name), iseed, batch)


def fixture_flags(name):
    return FLAG_ROPE | R.FLAG_REGISTERS(FIXTURES[name][1])


def fixture_tensors64(name, rope_cos, rope_sin):
    """The fixture's model under our names in float64 with NOTHING rounded on the way: LayerScale folded into o and fc2 in float64 (the
    converter rounds that product to fp32, a 2^-24 relative change of those weights), pos zeros, a zero key bias where the model has
    none, the identity head, and the given tables [NP, hd] or [NP, hd / 2] (the model's own: its module computes them in float32)."""
    cfg = fixture_cfg(name)
    D, h = cfg["dim"], cfg["dim"] // cfg["heads"] // 2
    sd = {k: np.asarray(v, np.float64) for k, v in dinov3_state_dict(name).items()}
    t = {k: np.asarray(v, np.float64) for k, v in fixture_model_tensors(name).items()}
    t["pos"] = np.zeros_like(t["pos"])
    t["head.weight"], t["head.bias"] = np.eye(D), np.zeros(D)
    for l in range(cfg["layers"]):
        if f"model.layer.{l}.attention.k_proj.bias" not in sd:
            t[f"l{l}.k.bias"] = np.zeros(D)
        for ours, i in (("o", 1), ("fc2", 2)):
            lam = sd[f"model.layer.{l}.layer_scale{i}.lambda1"]
            t[f"l{l}.{ours}.weight"] = t[f"l{l}.{ours}.weight"] * lam[:, None]
            t[f"l{l}.{ours}.bias"] = t[f"l{l}.{ours}.bias"] * lam
    t["rope.cos"], t["rope.sin"] = np.asarray(rope_cos, np.float64)[:, :h], np.asarray(rope_sin, np.float64)[:, :h]
    return t


def fixture_blob(name, identity_head=True):
    """The converter's blob of the fixture's state dict (ln_eps 1e-5), with the identity head: logits = pooler_output."""
    import vithip
    cfg = fixture_cfg(name)
    D = cfg["dim"]
    head = (np.eye(D, dtype=np.float32), np.zeros(D, np.float32)) if identity_head else None
    return vithip.blob_from_dinov3_state_dict(dinov3_state_dict(name), cfg, ln_eps=DINOV3_EPS, head=head)
