"""Other projects' checkpoint names and the recipes of the `transformers` fixtures (TEST INFRASTRUCTURE): vit_ref's seeded tensors
as the state dicts of numpy arrays that the converters take, so that the CPU tests rebuild a fixture's model without torch or
transformers, and tests/golden/make_golden_{clip,reg,pool,siglip,dinov3}.py load the same tensors into the Hugging Face models.
Behind the SigLIP names stand the inputs of the map_pool kernel test and the float32 statements its bounds come from."""
from __future__ import annotations

import math

import numpy as np

import vh_synth as S
import vit_ref as R

# The DINOv2 model of a fixture = the seeded tensors + seeded LayerScale vectors with tensor ids of the fixture scripts' own
# (uniform in 0.5 .. 1.5).
TID_LS1, TID_LS2 = 0x6000, 0x6100   # + layer
HF_LAYER_NAMES = (("ln1", "layernorm_before"), ("q", "attention.q_proj"), ("k", "attention.k_proj"), ("v", "attention.v_proj"),
                  ("o", "attention.o_proj"), ("ln2", "layernorm_after"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))


def make_clip_tensors(cfg, seed, flags):
    """The seeded tensors as a CLIP tower holds them: no patch-convolution bias, no projection bias (both zero)."""
    t = R.make_tensors(cfg, seed, flags)
    t["patch.bias"] = np.zeros_like(t["patch.bias"])
    t["head.bias"] = np.zeros_like(t["head.bias"])
    return t


def fixture_tensors(kind, cfg, flags, wseed):
    """The seeded tensors of a tests/golden/pool case.  BEiT has no key bias: there k.bias is zero."""
    t = R.make_tensors(cfg, wseed, flags)
    if kind == "beit":
        for l in range(cfg["layers"]):
            t[f"l{l}.k.bias"] = np.zeros_like(t[f"l{l}.k.bias"])
    return t


def layer_scale(cfg, seed, l):
    D = cfg["dim"]
    return (1.0 + 0.5 * S.fill(D, seed, TID_LS1 + l, 0).astype(np.float64)).astype(np.float32), \
           (1.0 + 0.5 * S.fill(D, seed, TID_LS2 + l, 0).astype(np.float64)).astype(np.float32)


def dinov2_state_dict(cfg, tensors, seed, unit_scale=False):
    """The seeded tensors (make_tensors) as a Hugging Face Dinov2(WithRegisters)Model state dict of numpy arrays."""
    D = cfg["dim"]
    t, sd, e = tensors, {}, "embeddings."
    sd[e + "cls_token"] = t["cls"].reshape(1, 1, D)
    sd[e + "mask_token"] = np.zeros((1, D), np.float32)
    sd[e + "position_embeddings"] = t["pos"].reshape(1, -1, D)
    if "reg" in t:
        sd[e + "register_tokens"] = t["reg"].reshape(1, -1, D)
    sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
    for l in range(cfg["layers"]):
        b = f"encoder.layer.{l}."
        for ours, theirs in (("ln1", "norm1"), ("q", "attention.attention.query"), ("k", "attention.attention.key"),
                             ("v", "attention.attention.value"), ("o", "attention.output.dense"), ("ln2", "norm2"),
                             ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
        l1, l2 = layer_scale(cfg, seed, l)
        sd[b + "layer_scale1.lambda1"] = np.ones_like(l1) if unit_scale else l1
        sd[b + "layer_scale2.lambda1"] = np.ones_like(l2) if unit_scale else l2
    sd["layernorm.weight"], sd["layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    return sd


def dinov2_classifier_state_dict(cfg, tensors, seed, unit_scale=False):
    """Seeded POOL_CLS_AVG tensors as a Dinov2(WithRegisters)ForImageClassification state dict (the backbone's names under
    `dinov2.` / `dinov2_with_registers.`, plus `classifier`)."""
    prefix = "dinov2_with_registers." if "reg" in tensors else "dinov2."
    sd = {prefix + k: v for k, v in dinov2_state_dict(cfg, tensors, seed, unit_scale).items()}
    sd["classifier.weight"], sd["classifier.bias"] = tensors["head.weight"], tensors["head.bias"]
    return sd


def ijepa_state_dict(cfg, tensors):
    """Seeded NO_CLS tensors as a Hugging Face IJepaForImageClassification state dict of numpy arrays."""
    D = cfg["dim"]
    t, sd, e = tensors, {}, "ijepa.embeddings."
    sd[e + "position_embeddings"] = t["pos"].reshape(1, -1, D)
    sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
    for l in range(cfg["layers"]):
        b = f"ijepa.layers.{l}."
        for ours, theirs in HF_LAYER_NAMES:
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
    sd["ijepa.layernorm.weight"], sd["ijepa.layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    sd["classifier.weight"], sd["classifier.bias"] = t["head.weight"], t["head.bias"]
    return sd


# ---- SigLIP (tests/golden/siglip, written by tests/golden/make_golden_siglip.py) ---------------------------------------------------
def siglip_tensors(cfg, seed, classifier):
    """Seeded tensors of a SigLIP vision tower under our names plus the raw head of the Hugging Face model: probe, in_proj (weights and
    ALL three biases), so that the converter's fold is exercised.  classifier: the model is SiglipForImageClassification (head [C][D]);
    otherwise SiglipVisionModel (no classifier: the blob's head is the identity)."""
    D, M = cfg["dim"], cfg["mlp_dim"]
    flags = R.FLAG_NO_CLS | R.FLAG_TANH_GELU | (R.FLAG_POOL(R.POOL_AVG_NORM) if classifier else R.FLAG_MAP_HEAD)
    t = R.make_tensors(cfg, seed, R.FLAG_NO_CLS | R.FLAG_TANH_GELU | R.FLAG_MAP_HEAD)
    raw = {"probe": S.fill(D, seed, 0x7020, 1, 0.5, 0.0), "in_proj_weight": S.fill(3 * D * D, seed, 0x7021, 1, 0.05, 0.0).reshape(3 * D, D),
           "in_proj_bias": S.fill(3 * D, seed, 0x7022, 1, 0.1, 0.0)}
    if not classifier:
        t["head.weight"], t["head.bias"] = np.eye(D, dtype=np.float32), np.zeros(D, np.float32)
    return t, raw, flags


def siglip_state_dict(cfg, t, raw, classifier, prefix=""):
    """The state dict of SiglipVisionModel (prefix "") / SiglipForImageClassification (prefix "vision_model." + classifier.*)."""
    D = cfg["dim"]
    sd = {prefix + "embeddings.patch_embedding.weight": t["patch.weight"], prefix + "embeddings.patch_embedding.bias": t["patch.bias"],
          prefix + "embeddings.position_embedding.weight": t["pos"]}
    names = (("ln1", "layer_norm1"), ("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"), ("v", "self_attn.v_proj"), ("o", "self_attn.out_proj"),
             ("ln2", "layer_norm2"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))
    for l in range(cfg["layers"]):
        for ours, theirs in names:
            for wb in ("weight", "bias"):
                sd[f"{prefix}encoder.layers.{l}.{theirs}.{wb}"] = t[f"l{l}.{ours}.{wb}"]
    sd[prefix + "post_layernorm.weight"], sd[prefix + "post_layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    h = prefix + "head."
    sd[h + "probe"] = raw["probe"].reshape(1, 1, D)
    sd[h + "attention.in_proj_weight"] = np.concatenate([raw["in_proj_weight"][:2 * D], t["map.v.weight"]])
    sd[h + "attention.in_proj_bias"] = np.concatenate([raw["in_proj_bias"][:2 * D], t["map.v.bias"]])
    sd[h + "attention.out_proj.weight"], sd[h + "attention.out_proj.bias"] = t["map.o.weight"], t["map.o.bias"]
    sd[h + "layernorm.weight"], sd[h + "layernorm.bias"] = t["map.ln.weight"], t["map.ln.bias"]
    for n in ("fc1", "fc2"):
        sd[f"{h}mlp.{n}.weight"], sd[f"{h}mlp.{n}.bias"] = t[f"map.{n}.weight"], t[f"map.{n}.bias"]
    if classifier:
        sd["classifier.weight"], sd["classifier.bias"] = t["head.weight"], t["head.bias"]
    return sd


def fixture_blob_tensors(cfg, t, raw, flags):
    """The tensors of the fixture's blob under our names: map.qk folded from the raw head, no map.* without MAP_HEAD."""
    D = cfg["dim"]
    out = dict(t)
    if flags & R.FLAG_MAP_HEAD:
        w, b = raw["in_proj_weight"], raw["in_proj_bias"]
        out["map.qk"] = R.fold_qk(raw["probe"], w[:D], b[:D], w[D:2 * D], cfg["heads"]).astype(np.float32)
    else:
        out = {k: v for k, v in out.items() if not k.startswith("map.")}
    return out


# ---- the inputs of the map_pool kernel test (tests/test_gpu_siglip.py) and the statements its bound comes from (tests/test_siglip.py) ----
MAP_DIMS = (64, 512, 520, 1032, 2048)      # the row kernels' piece-count boundaries (<= 512, <= 1024, <= 1536, above)
MAP_HEADS = (1, 2, 12, 16)
MAP_EPS = 1e-6


def map_pool_group(dim, heads):
    """The kernel's rows per group (kernels_features.hip map_pool_group): 16 waves, 8 in its widest instantiation, and 64 KiB of rows."""
    waves = 8 if dim > 1536 and heads > 12 else 16
    return min(waves, 16384 // dim)


def map_pool_inputs(dim, heads, NP, lead, batch, order="random"):
    """x [batch, lead + NP, dim] fp32 rows (sigma 1, a common-mode offset, one 300 sigma element in a patch row), gamma, beta, qk [heads, dim].
    order: "random" -- independent heads, scores of sigma 2;  "ascending" / "descending" -- every head a positive multiple of one
    direction and each image's patch rows sorted by their float64 score, so that the running maximum rises in every group / never
    after the first;  "gap" -- that direction again, rows in token order, the scores of one group of rows 200 or more (about 350) above those of the group before it."""
    rng = np.random.default_rng([dim, heads, NP, lead, batch, ("random", "ascending", "descending", "gap").index(order)])
    tokens = lead + NP
    x = (rng.standard_normal((batch, tokens, dim)) + rng.uniform(-0.8, 0.8, (batch, tokens, 1))).astype(np.float32)
    gamma = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.02 * rng.standard_normal(dim)).astype(np.float32)
    if order == "random":
        qk = (rng.standard_normal((heads, dim)) * (2.0 / math.sqrt(dim))).astype(np.float32)
    else:
        d = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
        scale = 2000.0 if order == "gap" else 6.0
        qk = ((1.0 + 0.02 * np.arange(heads))[:, None] * d[None, :] * (scale / dim)).astype(np.float32)
        g = map_pool_group(dim, heads)
        if order == "gap":   # rows without a component along d, then 0.2 k of it in group k: the score is 2000 b / sqrt(1 + b^2)
            r = x[:, lead:].astype(np.float64)
            r -= (r @ d)[:, :, None] * d[None, None, :] / dim
            x[:, lead:] = (r / r.std(-1, keepdims=True)).astype(np.float32)      # unit sigma: the score depends on the group alone
            step = np.broadcast_to(0.2 * (np.arange(NP) // g), (batch, NP))
        else:
            step = 2.0 * rng.uniform(-1.0, 1.0, (batch, NP))
        x[:, lead:] += (step[:, :, None] * d[None, None, :]).astype(np.float32)
    k3 = dim // 3
    x[batch - 1, lead + min(1, NP - 1), k3] = np.float32(300.0 if order != "gap" else -300.0 * (1.0 if k3 % 2 == 0 else -1.0))   # (gap: against d)
    if order in ("ascending", "descending"):   # sort every image's patch rows by the score of head 0 (all heads order alike)
        y = R.layernorm(x[:, lead:].astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), MAP_EPS)
        s0 = y @ qk[0].astype(np.float64)
        for b in range(batch):
            idx = np.argsort(s0[b], kind="stable")
            x[b, lead:] = x[b, lead:][idx[::-1] if order == "descending" else idx]
    return x, gamma, beta, qk


def map_pool_cases(dim):
    """(heads, NP, lead, batch, order) of the kernel test at this dim: NP on and around the group size, both leads and batches for the
    independent-head inputs; the arranged scores at the longest NP."""
    out = []
    for heads in MAP_HEADS:
        g = map_pool_group(dim, heads)
        for NP in sorted({1, g - 1, g, g + 1, 2 * g + 3}):
            for lead in (0, 3):
                for batch in (1, 3):
                    out.append((heads, NP, lead, batch, "random"))
        if heads >= 12:
            out += [(heads, 2 * g + 3, 0, 3, o) for o in ("ascending", "descending", "gap")]
    return out


def map_z64(x, gamma, beta, qk, lead):
    """The float64 z [batch, heads, dim] of rows x [batch, tokens, dim] (any float type), and the float64 scores [batch, heads, NP]."""
    y = R.layernorm(np.asarray(x, np.float64)[:, lead:], gamma.astype(np.float64), beta.astype(np.float64), MAP_EPS)
    return R.map_z(y, qk.astype(np.float64)), np.einsum("btk,hk->bht", y, qk.astype(np.float64))


def map_z32(x, gamma, beta, qk, lead):
    """The same function with every operation in float32, in the plainest order: the two-pass LayerNorm, one dot product per score,
    softmax with the row maximum taken off, rows added in ascending order, one division at the end."""
    f = np.float32
    x = np.asarray(x, f)[:, lead:]
    mean = x.mean(-1, keepdims=True, dtype=f)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=f)
    y = (d * (f(1.0) / np.sqrt(var + f(MAP_EPS)))) * gamma + beta
    s = np.einsum("btk,hk->bht", y, qk.astype(f)).astype(f)
    p = np.exp(s - s.max(-1, keepdims=True))
    acc = np.zeros((x.shape[0], qk.shape[0], x.shape[2]), f)
    l = np.zeros((x.shape[0], qk.shape[0], 1), f)
    for t in range(x.shape[1]):
        acc = acc + p[:, :, t, None] * y[:, None, t, :]
        l = l + p[:, :, t, None]
    return acc / l


def seq_linear32(a, w, b):
    """a [rows, K] w[N, K]^T + b with every operation in float32 and the products added in ascending k: the plainest order."""
    f = np.float32
    a, w = np.asarray(a, f), np.asarray(w, f)
    acc = np.zeros((a.shape[0], w.shape[0]), f)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * w[None, :, k]
    return acc + np.asarray(b, f)


def map_head32(x, t, heads, flags, eps):
    """The whole head in float32 from the patch rows x [batch, NP, D]: map_z32, then the [batch]-row stages through seq_linear32.  The
    statement the bound of the head-stage test comes from (4 x its error against float64, as for the kernel)."""
    f = np.float32
    t = {k: v.astype(f) for k, v in t.items()}
    batch, _, D = x.shape
    hd = D // heads
    z = map_z32(x, t["lnf.weight"], t["lnf.bias"], t["map.qk"], 0) if eps == MAP_EPS else None
    assert z is not None, "map_head32 is written for ln_eps = MAP_EPS"
    a = np.concatenate([seq_linear32(z[:, h], t["map.v.weight"][h * hd:(h + 1) * hd], t["map.v.bias"][h * hd:(h + 1) * hd]) for h in range(heads)], 1)
    o = seq_linear32(a, t["map.o.weight"], t["map.o.bias"])
    mean = o.mean(-1, keepdims=True, dtype=f)
    d = o - mean
    ln = d * (f(1.0) / np.sqrt((d * d).mean(-1, keepdims=True, dtype=f) + f(eps))) * t["map.ln.weight"] + t["map.ln.bias"]
    hid = R.activation(flags)(seq_linear32(ln, t["map.fc1.weight"], t["map.fc1.bias"]))
    return o + seq_linear32(hid.astype(f), t["map.fc2.weight"], t["map.fc2.bias"])


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
    return R.FLAG_ROPE | R.FLAG_REGISTERS(FIXTURES[name][1])


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
