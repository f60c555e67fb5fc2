"""Reference forward with register tokens (TEST INFRASTRUCTURE): VH_FLAG_REGISTERS(R).

The C oracle (oracle/) does not know register tokens, so the register tests bring their own reference, as tests/clip_ref.py
did for the CLIP switches: a numpy forward in float32 or float64 over the canonical blob, with R learned rows between the class
token and the patch rows of every image (DINOv2 "with registers", Hugging Face's hidden_states order):
    row 0          cls + pos[0]
    rows 1 .. R    reg[r]                    (no position row)
    row 1 + R + p  patch embedding + pos[1 + p]
Token assembly is its own function (`assemble`); layers, quantisers and the VH_DTYPE_FP8 data-flow emulation are clip_ref's and
oracle_lib's (not edited).  With R = 0 this is clip_ref.forward (tests/test_registers.py ties them together on vit_micro).

It also states the blob layout with the new tensor, in numpy, on top of vh_synth / clip_ref: `pos` stays [(NP + 1)][D]; `reg`
[R][D] sits directly after `pos`, in front of pre_ln.* when both are present; tensor id 7, sigma as `cls` (0.02), offset 0;
the header flags word (byte 52) carries the count in bits 9 .. 13, beside clip_ref's bits 1 and 2.
"""
from __future__ import annotations

import numpy as np

import clip_ref as CR
import vh_synth as S

FLAG_PRE_LN, FLAG_QUICK_GELU = CR.FLAG_PRE_LN, CR.FLAG_QUICK_GELU
FLAG_REGISTERS_MASK = 31 << 9
TID_REG = 7


def FLAG_REGISTERS(n):
    return (int(n) & 31) << 9


def registers_of(flags):
    return (int(flags) & FLAG_REGISTERS_MASK) >> 9


def tokens(cfg, flags=0):
    return S.tokens(cfg) + registers_of(flags)


def tensor_table(cfg, flags=0):
    """clip_ref.tensor_table with reg [R][D] directly after `pos` (in front of pre_ln.*)."""
    t = CR.tensor_table(cfg, flags)
    R = registers_of(flags)
    if R:
        i = [n for n, *_ in t].index("pos") + 1
        t[i:i] = [("reg", (R, cfg["dim"]), TID_REG, 0.02, 0.0)]
    return t


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = CR.blob_header(cfg, flags, ln_eps)
    bits = int(h[52:56].view(np.uint32)[0]) | (int(flags) & FLAG_REGISTERS_MASK)
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


def patch_embed(cfg, t, images):
    """[batch, NP, D]: patches in NHWC order against the conv kernel [D][c][ky][kx] permuted to [D][ky][kx][c], plus the bias."""
    D, P, CH = cfg["dim"], cfg["patch_size"], cfg["channels"]
    g = cfg["image_size"] // P
    batch = images.shape[0]
    col = images.reshape(batch, g, P, g, P, CH).transpose(0, 1, 3, 2, 4, 5).reshape(batch * g * g, P * P * CH)
    pw = t["patch.weight"].transpose(0, 2, 3, 1).reshape(D, P * P * CH)
    return (col @ pw.T + t["patch.bias"]).reshape(batch, g * g, D)


def assemble(emb, cls, pos, reg=None):
    """Token assembly: emb [batch, NP, D] -> x [batch, 1 + R + NP, D] in the row order of the module docstring."""
    batch, NP, D = emb.shape
    R = 0 if reg is None else reg.shape[0]
    assert pos.shape == (NP + 1, D), (pos.shape, NP, D)
    x = np.empty((batch, 1 + R + NP, D), dtype=emb.dtype)
    x[:, 0] = cls + pos[0]
    if R:
        x[:, 1:1 + R] = reg
    x[:, 1 + R:] = emb + pos[1:]
    return x


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, all_hidden=False):
    """logits [batch, classes]; want_hidden: also the residual rows [batch * tokens, dim] after `n_layers` layers (n_layers = 0:
    the embedded rows, after the pre-LayerNorm if there is one); all_hidden: also the list of the rows after 0, 1, .. layers.
    fp8: None, "plain" or "folded" (float32 only): clip_ref's emulation of the VH_DTYPE_FP8 data flow."""
    f = dtype if fp8 is None else np.float32
    t = {k: v.astype(f) for k, v in unpack_blob(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    dh = D // H
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = CR.quick_gelu if flags & FLAG_QUICK_GELU else CR.gelu
    x = assemble(patch_embed(cfg, t, images), t["cls"], t["pos"], t.get("reg"))
    T = x.shape[1]
    assert T == tokens(cfg, flags)
    x = x.reshape(batch * T, D)
    if flags & FLAG_PRE_LN:
        x = CR.layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    hidden = [x]
    L = cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])
    for l in range(L):
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
        hidden.append(x)
    cls = CR.layernorm(x.reshape(batch, T, D)[:, 0], t["lnf.weight"], t["lnf.bias"], ln_eps)
    logits = cls @ t["head.weight"].T + t["head.bias"]
    if all_hidden:
        return logits, x, hidden
    return (logits, x) if want_hidden else logits


def final_norm(cfg, blob, x, flags=0, ln_eps=1e-6):
    """The model's final LayerNorm over residual rows x [rows, dim] (DINOv2's last_hidden_state), in x's float type."""
    t = unpack_blob(cfg, blob, flags)
    return CR.layernorm(x, t["lnf.weight"].astype(x.dtype), t["lnf.bias"].astype(x.dtype), ln_eps)


# ---- the fixtures of tests/golden/reg (make_golden_reg.py) --------------------------------------------------------------
# The DINOv2 model of a fixture = this repository's seeded tensors under the Hugging Face names + seeded LayerScale vectors with
# tensor ids of the fixture script's own (uniform in 0.5 .. 1.5).  Stated here so that the tests can rebuild the state dict
# without torch or transformers.
TID_LS1, TID_LS2 = 0x6000, 0x6100   # + layer


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
