"""Reference forward for pooled heads and models without a class token (TEST INFRASTRUCTURE): VH_FLAG_NO_CLS, VH_FLAG_POOL(m).

Built on reg_ref / clip_ref (not edited), as reg_ref was built on clip_ref: a numpy forward in float32 or float64 over the canonical
blob with
  * NO_CLS   no class-token row: tokens = NP + R, rows reg[0 .. R - 1], then patch p + pos[p]; the blob has no `cls`, pos is [NP][D]
  * POOL(m)  what the head multiplies; p runs over the NP patch rows only, the LayerNorm is lnf.* in every mode:
               POOL_CLS        head(LN(row 0))
               POOL_AVG_NORM   head(mean_p LN(x_p))
               POOL_AVG_FCNORM head(LN(mean_p x_p))
               POOL_CLS_AVG    head(concat(LN(row 0), mean_p LN(x_p))), head.weight [C][2 D]
The layers, the quantisers and the VH_DTYPE_FP8 data-flow emulation are reg_ref's and clip_ref's.  With both switches clear this is
reg_ref.forward, bit for bit (tests/test_pool.py ties them together).

It also states the blob layout: reg_ref.tensor_table without `cls` and with pos [NP][D] under NO_CLS, head.weight [C][2 D] under
POOL_CLS_AVG, every tensor id kept; the header flags word (byte 52) carries bit 15 and bits 16 .. 17 beside reg_ref's bits.
"""
from __future__ import annotations

import numpy as np

import clip_ref as CR
import reg_ref as R
import vh_synth as S

FLAG_PRE_LN, FLAG_QUICK_GELU, FLAG_REGISTERS, registers_of = R.FLAG_PRE_LN, R.FLAG_QUICK_GELU, R.FLAG_REGISTERS, R.registers_of
FLAG_NO_CLS, FLAG_POOL_MASK = 1 << 15, 3 << 16
POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM, POOL_CLS_AVG = range(4)
POOL_NAMES = {POOL_CLS: "cls", POOL_AVG_NORM: "avg_norm", POOL_AVG_FCNORM: "avg_fcnorm", POOL_CLS_AVG: "cls_avg"}


def FLAG_POOL(m):
    return (int(m) & 3) << 16


def pool_of(flags):
    return (int(flags) & FLAG_POOL_MASK) >> 16


def legal(flags):
    """The combinations vh_create accepts: NO_CLS goes with the two modes that do not read a class token."""
    return not (flags & FLAG_NO_CLS) or pool_of(flags) in (POOL_AVG_NORM, POOL_AVG_FCNORM)


def tokens(cfg, flags=0):
    return S.tokens(cfg) - (1 if flags & FLAG_NO_CLS else 0) + registers_of(flags)


def head_width(cfg, flags=0):
    return cfg["dim"] * (2 if pool_of(flags) == POOL_CLS_AVG else 1)


def tensor_table(cfg, flags=0):
    t = R.tensor_table(cfg, flags & ~(FLAG_NO_CLS | FLAG_POOL_MASK))
    D, NP = cfg["dim"], S.tokens(cfg) - 1
    out = []
    for name, shape, tid, sigma, off in t:
        if flags & FLAG_NO_CLS and name == "cls":
            continue
        if flags & FLAG_NO_CLS and name == "pos":
            shape = (NP, D)
        if name == "head.weight":
            shape = (cfg["classes"], head_width(cfg, flags))
        out.append((name, tuple(shape), tid, sigma, off))
    return out


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = R.blob_header(cfg, flags, ln_eps)
    bits = int(h[52:56].view(np.uint32)[0]) | (int(flags) & (FLAG_NO_CLS | FLAG_POOL_MASK))
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def make_tensors(cfg, seed, flags=0):
    return {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape)
            for name, shape, tid, sigma, off in tensor_table(cfg, flags)}


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


def without_cls(tensors):
    """The tensors of the class-token model of the same patch rows -> the NO_CLS model's: no `cls`, pos without its row 0."""
    t = {k: v for k, v in tensors.items() if k != "cls"}
    t["pos"] = np.ascontiguousarray(tensors["pos"][1:])
    return t


def assemble(emb, cls, pos, reg=None):
    """Token assembly.  cls is None: no row 0 -- x [batch, R + NP, D] = reg rows, then emb + pos with pos [NP, D]."""
    if cls is not None:
        return R.assemble(emb, cls, pos, reg)
    batch, NP, D = emb.shape
    Rn = 0 if reg is None else reg.shape[0]
    assert pos.shape == (NP, D), (pos.shape, NP, D)
    x = np.empty((batch, Rn + NP, D), dtype=emb.dtype)
    if Rn:
        x[:, :Rn] = reg
    x[:, Rn:] = emb + pos
    return x


def head_input(x, lnw, lnb, eps, lead, pool):
    """x [batch, T, D] -> the head's input [batch, W]."""
    ln = lambda v: CR.layernorm(v, lnw, lnb, eps)
    if pool == POOL_CLS:
        return ln(x[:, 0])
    if pool == POOL_AVG_NORM:
        return ln(x[:, lead:]).mean(1)
    if pool == POOL_AVG_FCNORM:
        return ln(x[:, lead:].mean(1))
    return np.concatenate([ln(x[:, 0]), ln(x[:, lead:]).mean(1)], -1)


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, want_head=False):
    """logits [batch, classes]; want_hidden: also the residual rows [batch * tokens, dim] after `n_layers` layers; want_head: also
    the head's input [batch, W].  fp8 as reg_ref.forward."""
    f = dtype if fp8 is None else np.float32
    t = {k: v.astype(f) for k, v in unpack_blob(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    dh = D // H
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = CR.quick_gelu if flags & FLAG_QUICK_GELU else CR.gelu
    x = assemble(R.patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    assert T == tokens(cfg, flags)
    x = x.reshape(batch * T, D)
    if flags & FLAG_PRE_LN:
        x = CR.layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    L = cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])
    for l in range(L):   # reg_ref.forward's layer, statement for statement
        p = lambda n: t[f"l{l}.{n}"]
        wqkv = np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")])
        bqkv = np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
        if fp8 == "folded":
            qkv = CR._bf16(CR._ln_linear_f8_folded(x, p("ln1.weight"), p("ln1.bias"), wqkv, bqkv, ln_eps))
            x = x + CR._linear_f8(CR._e4m3(CR._attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
            hid = CR._e4m3(act(CR._ln_linear_f8_folded(x, p("ln2.weight"), p("ln2.bias"), p("fc1.weight"), p("fc1.bias"), ln_eps)))
            x = (x + CR._linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
        elif fp8:
            y = CR._e4m3(CR.layernorm(x, p("ln1.weight"), p("ln1.bias"), ln_eps))
            qkv = CR._bf16(CR._linear_f8(y, wqkv, bqkv))
            x = x + CR._linear_f8(CR._e4m3(CR._attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
            y = CR._e4m3(CR.layernorm(x, p("ln2.weight"), p("ln2.bias"), ln_eps))
            hid = CR._e4m3(act(CR._linear_f8(y, p("fc1.weight"), p("fc1.bias")).astype(np.float32)))
            x = (x + CR._linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
        else:
            y = CR.layernorm(x, p("ln1.weight"), p("ln1.bias"), ln_eps)
            x = x + CR._attention(y @ wqkv.T + bqkv, batch, T, H, dh) @ p("o.weight").T + p("o.bias")
            y = CR.layernorm(x, p("ln2.weight"), p("ln2.bias"), ln_eps)
            x = x + act(y @ p("fc1.weight").T + p("fc1.bias")) @ p("fc2.weight").T + p("fc2.bias")
    lead = tokens(cfg, flags) - (S.tokens(cfg) - 1)
    hin = head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


# ---- state dicts of the fixtures' models (tests/golden/make_golden_pool.py) and of the converter tests -----------------------
HF_LAYER_NAMES = (("ln1", "layernorm_before"), ("q", "attention.q_proj"), ("k", "attention.k_proj"), ("v", "attention.v_proj"),
                  ("o", "attention.o_proj"), ("ln2", "layernorm_after"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))


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


def fixture_tensors(kind, cfg, flags, wseed):
    """The seeded tensors of a tests/golden/pool case.  BEiT has no key bias: there k.bias is zero."""
    t = make_tensors(cfg, wseed, flags)
    if kind == "beit":
        for l in range(cfg["layers"]):
            t[f"l{l}.k.bias"] = np.zeros_like(t[f"l{l}.k.bias"])
    return t


def dinov2_classifier_state_dict(cfg, tensors, seed, unit_scale=False):
    """Seeded POOL_CLS_AVG tensors as a Dinov2(WithRegisters)ForImageClassification state dict (reg_ref's backbone names under
    `dinov2.` / `dinov2_with_registers.`, plus `classifier`)."""
    prefix = "dinov2_with_registers." if "reg" in tensors else "dinov2."
    sd = {prefix + k: v for k, v in R.dinov2_state_dict(cfg, tensors, seed, unit_scale).items()}
    sd["classifier.weight"], sd["classifier.bias"] = tensors["head.weight"], tensors["head.bias"]
    return sd
