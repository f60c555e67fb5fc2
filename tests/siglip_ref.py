"""The reference for the two SigLIP model flags (TEST INFRASTRUCTURE): VH_FLAG_TANH_GELU and VH_FLAG_MAP_HEAD on top of tests/vit_ref.py,
whose patch_embed / assemble / layer / layernorm run the backbone; the activation, the attention-pooling head, the blob's eleven
map.* tensors and the two header bits are stated here, independently of include/vithip.h (tests/test_siglip.py compares the two).

  TANH_GELU  (1 << 21)  the MLP activation is 0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3)))
  MAP_HEAD   (1 << 19)  the head's input is the attention-pooling block; per image, t over the NP patch rows:
        y_t = LN(x_t; lnf);  s[h,t] = qk[h] . y_t;  p[h,.] = softmax_t s[h,.];  z[h] = sum_t p[h,t] y_t
        a[h hd + j] = v.weight[h hd + j] . z[h] + v.bias[h hd + j];  o = o.weight a + o.bias
        u = o + fc2(act(fc1(LN(o; map.ln))));  logits = head(u)
      map.qk[h] = W_k,h^T (W_q,h probe + b_q,h) / sqrt(hd) is folded by whoever builds the blob (fold_qk, float64): the query is one
      learned vector, and the key bias shifts every score of a head by the same constant, which the softmax cancels.
      literal_map() is the block as torch.nn.MultiheadAttention states it (K and V of every token, every in_proj bias).

Blob: vit_ref's, then -- MAP_HEAD -- directly after head.bias, all fp32: map.qk [H][D], map.v.weight [D][D], map.v.bias [D],
map.o.weight [D][D], map.o.bias [D], map.ln.weight [D], map.ln.bias [D], map.fc1.weight [M][D], map.fc1.bias [M], map.fc2.weight [D][M],
map.fc2.bias [D]; seeded tensor ids 0x7010 .. 0x701A in that order.  The header's flags word carries both bits at their flag positions.
"""
from __future__ import annotations

import math

import numpy as np

import vh_synth as S
import vit_ref as R

FLAG_MAP_HEAD, FLAG_TANH_GELU = 1 << 19, 1 << 21
NEW_BITS = FLAG_MAP_HEAD | FLAG_TANH_GELU
TID_MAP = 0x7010
MAX_HEADS = 16
NO_CLS, QUICK, PRE = R.FLAG_NO_CLS, R.FLAG_QUICK_GELU, R.FLAG_PRE_LN


def old(flags):
    """The bits vit_ref knows."""
    return int(flags) & ~NEW_BITS


def legal(cfg, flags):
    """The combinations vh_create accepts."""
    if flags & FLAG_TANH_GELU and flags & QUICK:
        return False
    if flags & FLAG_MAP_HEAD:
        return bool(flags & NO_CLS) and R.pool_of(flags) == 0 and R.registers_of(flags) == 0 and cfg["heads"] <= MAX_HEADS and not flags & 8   # (8: CLS_TAIL)
    return R.legal(old(flags))


# ---- layout -------------------------------------------------------------------------------------------------------------------
def map_table(cfg):
    D, M, H = cfg["dim"], cfg["mlp_dim"], cfg["heads"]
    sw, sb, sg = 0.02, 0.02, 0.05
    rows = [("map.qk", (H, D), sw, 0.0), ("map.v.weight", (D, D), sw, 0.0), ("map.v.bias", (D,), sb, 0.0), ("map.o.weight", (D, D), sw, 0.0),
            ("map.o.bias", (D,), sb, 0.0), ("map.ln.weight", (D,), sg, 1.0), ("map.ln.bias", (D,), sb, 0.0),
            ("map.fc1.weight", (M, D), sw, 0.0), ("map.fc1.bias", (M,), sb, 0.0), ("map.fc2.weight", (D, M), sw, 0.0), ("map.fc2.bias", (D,), sb, 0.0)]
    return [(n, s, TID_MAP + i, sig, off) for i, (n, s, sig, off) in enumerate(rows)]


def tensor_table(cfg, flags=0):
    return R.tensor_table(cfg, old(flags)) + (map_table(cfg) if flags & FLAG_MAP_HEAD else [])


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = R.blob_header(cfg, old(flags), ln_eps)
    bits = int(h[52:56].view(np.uint32)[0]) | (int(flags) & NEW_BITS)
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def make_tensors(cfg, seed, flags=0):
    return {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape) for name, shape, tid, sigma, off in tensor_table(cfg, flags)}


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


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def tanh_gelu(v):
    """0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3))) in v's float type."""
    v = np.asarray(v)
    f = v.dtype.type
    return f(0.5) * v * (f(1.0) + np.tanh(f(math.sqrt(2.0 / math.pi)) * (v + f(0.044715) * v * v * v)))


def activation(flags):
    return tanh_gelu if flags & FLAG_TANH_GELU else R.quick_gelu if flags & QUICK else R.gelu


def fold_qk(probe, wq, bq, wk, heads):
    """map.qk [H][D] in float64: qk[h] = W_k,h^T (W_q,h probe + b_q,h) / sqrt(hd)."""
    probe, wq, bq, wk = (np.asarray(a, dtype=np.float64) for a in (probe, wq, bq, wk))
    D = wq.shape[0]
    hd = D // heads
    q = (wq @ probe.reshape(D) + bq).reshape(heads, hd) / math.sqrt(hd)
    return np.einsum("hj,hjk->hk", q, wk.reshape(heads, hd, D))


def map_z(y, qk):
    """y [batch, NP, D] (the normalised patch rows), qk [H, D] -> z [batch, H, D], in y's float type."""
    s = np.einsum("btk,hk->bht", y, qk.astype(y.dtype))
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return np.einsum("bht,btk->bhk", p, y)


def map_tail(z, t, heads, act, eps):
    """z [batch, H, D] -> u [batch, D]: the per-head V product, the out-projection, LayerNorm + MLP with the residual."""
    batch, H, D = z.shape
    hd = D // heads
    vw = t["map.v.weight"].reshape(H, hd, D)
    a = np.einsum("bhk,hjk->bhj", z, vw).reshape(batch, D) + t["map.v.bias"]
    o = a @ t["map.o.weight"].T + t["map.o.bias"]
    hid = act(R.layernorm(o, t["map.ln.weight"], t["map.ln.bias"], eps) @ t["map.fc1.weight"].T + t["map.fc1.bias"])
    return o + hid @ t["map.fc2.weight"].T + t["map.fc2.bias"]


def map_head(y, t, heads, act, eps):
    return map_tail(map_z(y, t["map.qk"]), t, heads, act, eps)


def literal_map(y, probe, in_w, in_b, out_w, out_b, heads):
    """torch.nn.MultiheadAttention(probe, y, y) stated literally in y's float type: q, k, v through in_proj (weights [3 D][D], biases
    [3 D]), K and V of EVERY token, softmax(q k^T / sqrt(hd)) v per head, the out-projection.  y [batch, NP, D] -> o [batch, D]."""
    batch, NP, D = y.shape
    hd = D // heads
    q = (in_w[:D] @ probe.reshape(D) + in_b[:D]).reshape(heads, hd)
    k = (y @ in_w[D:2 * D].T + in_b[D:2 * D]).reshape(batch, NP, heads, hd)
    v = (y @ in_w[2 * D:].T + in_b[2 * D:]).reshape(batch, NP, heads, hd)
    s = np.einsum("hj,bthj->bht", q, k) / y.dtype.type(math.sqrt(hd))
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    a = np.einsum("bht,bthj->bhj", p, v).reshape(batch, D)
    return a @ out_w.T + out_b


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, want_head=False):
    """vit_ref.forward for every flag, the two new ones included: logits [batch, classes], then -- when asked for -- the residual rows
    [batch * tokens, dim] and the head's input [batch, W] (MAP_HEAD: u)."""
    f = dtype if fp8 is None else np.float32
    t = {k: v.astype(f) for k, v in unpack_blob(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = activation(flags)
    x = R.assemble(R.patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    x = x.reshape(batch * T, D)
    if flags & PRE:
        x = R.layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    for l in range(cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])):
        x = R.layer(x, lambda n: t[f"l{l}.{n}"], act, batch, T, H, D // H, ln_eps, fp8)
    lead = T - (S.tokens(cfg) - 1)
    if flags & FLAG_MAP_HEAD:
        y = R.layernorm(x.reshape(batch, T, D)[:, lead:], t["lnf.weight"], t["lnf.bias"], ln_eps)
        hin = map_head(y, t, H, act, ln_eps)
    else:
        hin = R.head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, R.pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


# ---- Hugging Face names ---------------------------------------------------------------------------------------------------------
def siglip_tensors(cfg, seed, classifier):
    """Seeded tensors of a SigLIP vision tower under our names plus the raw head of the Hugging Face model: probe, in_proj (weights and
    ALL three biases), so that the converter's fold is exercised.  classifier: the model is SiglipForImageClassification (head [C][D]);
    otherwise SiglipVisionModel (no classifier: the blob's head is the identity)."""
    D, M = cfg["dim"], cfg["mlp_dim"]
    flags = NO_CLS | FLAG_TANH_GELU | (R.FLAG_POOL(R.POOL_AVG_NORM) if classifier else FLAG_MAP_HEAD)
    t = make_tensors(cfg, seed, NO_CLS | FLAG_TANH_GELU | FLAG_MAP_HEAD)
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
    if flags & FLAG_MAP_HEAD:
        w, b = raw["in_proj_weight"], raw["in_proj_bias"]
        out["map.qk"] = fold_qk(raw["probe"], w[:D], b[:D], w[D:2 * D], cfg["heads"]).astype(np.float32)
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
    return map_z(y, qk.astype(np.float64)), np.einsum("btk,hk->bht", y, qk.astype(np.float64))


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
    hid = activation(flags)(seq_linear32(ln, t["map.fc1.weight"], t["map.fc1.bias"]))
    return o + seq_linear32(hid.astype(f), t["map.fc2.weight"], t["map.fc2.bias"])
