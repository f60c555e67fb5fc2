"""The reference model (TEST INFRASTRUCTURE): one numpy forward, in float32 or float64, for every model flag, and the one
description of the canonical blob with every optional tensor.  The C oracle (oracle/) knows none of the flags; with flags = 0 this
is the oracle's function and vh_synth's blob (tests/test_clip.py, tests/test_registers.py), and each flag is pinned by fixtures
computed with Hugging Face `transformers` (tests/golden/clip, reg, pool).  A new model flag extends this module in place.

Flags (the values of include/vithip.h, stated here independently; the tests compare the two):
  PRE_LN        a LayerNorm over the embedded tokens in front of layer 0 (CLIP's ln_pre)
  QUICK_GELU    x * sigmoid(1.702 x) instead of erf GELU in the MLP
  REGISTERS(R)  R learned rows without a position row (DINOv2 "with registers", Hugging Face's hidden_states order)
  NO_CLS        no class-token row; legal with the two pool modes that do not read one
  POOL(m)       what the head multiplies; p runs over the NP patch rows only, the LayerNorm is lnf.* in every mode:
                  POOL_CLS        head(LN(row 0))
                  POOL_AVG_NORM   head(mean_p LN(x_p))
                  POOL_AVG_FCNORM head(LN(mean_p x_p))
                  POOL_CLS_AVG    head(concat(LN(row 0), mean_p LN(x_p)))

Row order of one image, tokens = (1 or 0) + R + NP:
    row 0                cls + pos[0]                      (absent under NO_CLS, where pos has NP rows and patch p adds pos[p])
    the next R rows      reg[r]
    the last NP rows     patch embedding p + pos[1 + p]

Blob: vh_synth's 64-byte header and fp32 tensors in vh_synth.tensor_table's order, every tensor keeping its id, sigma and offset,
with  `cls` dropped and pos [NP][D] under NO_CLS;  reg [R][D] directly after `pos` (id 7, sigma as `cls`, offset 0);  then
pre_ln.weight [D], pre_ln.bias [D] (ids 5 and 6, sigma and offset of the other LayerNorms);  head.weight [C][2 D] under
POOL_CLS_AVG.  The header's flags word (byte 52; bit 0 belongs to the file form's checksum): bit 1 = pre-LN, bit 2 = QuickGELU,
the register count, NO_CLS and the pool mode at their flag positions (bits 9 .. 13, 15, 16 .. 17).

fp8 = "plain" / "folded" emulates the VH_DTYPE_FP8 data flow in float32: e4m3 operands through oracle_lib's quantisers, the same
rounding points as oracle/vit_oracle.c oracle_vit_forward_fp8 / _fp8_folded.
"""
from __future__ import annotations

import math

import numpy as np

import vh_synth as S

FLAG_PRE_LN, FLAG_QUICK_GELU = 16, 32
FLAG_REGISTERS_MASK, FLAG_NO_CLS, FLAG_POOL_MASK = 31 << 9, 1 << 15, 3 << 16
POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM, POOL_CLS_AVG = range(4)
POOL_NAMES = {POOL_CLS: "cls", POOL_AVG_NORM: "avg_norm", POOL_AVG_FCNORM: "avg_fcnorm", POOL_CLS_AVG: "cls_avg"}
HDR_PRE_LN, HDR_QUICK_GELU = 2, 4
TID_PRE_LN_W, TID_PRE_LN_B, TID_REG = 5, 6, 7
_erf = np.vectorize(math.erf, otypes=[np.float64])


def FLAG_REGISTERS(n):
    return (int(n) & 31) << 9


def registers_of(flags):
    return (int(flags) & FLAG_REGISTERS_MASK) >> 9


def FLAG_POOL(m):
    return (int(m) & 3) << 16


def pool_of(flags):
    return (int(flags) & FLAG_POOL_MASK) >> 16


def legal(flags):
    """The combinations vh_create accepts: NO_CLS goes with the two modes that do not read a class token."""
    return not (flags & FLAG_NO_CLS) or pool_of(flags) in (POOL_AVG_NORM, POOL_AVG_FCNORM)


# ---- layout -------------------------------------------------------------------------------------------------------------------
def tokens(cfg, flags=0):
    return S.tokens(cfg) - (1 if flags & FLAG_NO_CLS else 0) + registers_of(flags)


def head_width(cfg, flags=0):
    return cfg["dim"] * (2 if pool_of(flags) == POOL_CLS_AVG else 1)


def tensor_table(cfg, flags=0):
    """[(name, shape, tensor_id, sigma, offset)] in blob order: vh_synth.tensor_table with the changes of the module docstring."""
    D, R, no_cls = cfg["dim"], registers_of(flags), bool(flags & FLAG_NO_CLS)
    out = []
    for name, shape, tid, sigma, off in S.tensor_table(cfg):
        if name == "cls" and no_cls:
            continue
        if name == "pos" and no_cls:
            shape = (S.tokens(cfg) - 1, D)
        if name == "head.weight":
            shape = (cfg["classes"], head_width(cfg, flags))
        out.append((name, tuple(shape), tid, sigma, off))
        if name == "pos":
            if R:
                out.append(("reg", (R, D), TID_REG, 0.02, 0.0))
            if flags & FLAG_PRE_LN:
                out += [("pre_ln.weight", (D,), TID_PRE_LN_W, 0.05, 1.0), ("pre_ln.bias", (D,), TID_PRE_LN_B, 0.02, 0.0)]
    return out


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = S.blob_header(cfg, ln_eps)
    bits = (HDR_PRE_LN if flags & FLAG_PRE_LN else 0) | (HDR_QUICK_GELU if flags & FLAG_QUICK_GELU else 0) \
        | (int(flags) & (FLAG_REGISTERS_MASK | FLAG_NO_CLS | FLAG_POOL_MASK))
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def make_tensors(cfg, seed, flags=0):
    return {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape)
            for name, shape, tid, sigma, off in tensor_table(cfg, flags)}


def without_cls(tensors):
    """The tensors of the class-token model of the same patch rows -> the NO_CLS model's: no `cls`, pos without its row 0."""
    t = {k: v for k, v in tensors.items() if k != "cls"}
    t["pos"] = np.ascontiguousarray(tensors["pos"][1:])
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


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def quick_gelu(v):
    """x * sigmoid(1.702 x), overflow-free for every finite x (float64 or float32 in, same type out)."""
    v = np.asarray(v)
    z = np.exp(-np.abs(v) * v.dtype.type(1.702))
    return np.where(v >= 0, v / (1 + z), v * z / (1 + z))


def gelu(v):
    return (0.5 * v * (1.0 + _erf(v.astype(np.float64) * (1.0 / math.sqrt(2.0))))).astype(v.dtype)


def layernorm(x, g, b, eps):
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + x.dtype.type(eps)) * g + b


def attention(qkv, batch, T, H, dh):
    D = H * dh
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(batch, T, H, dh).transpose(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(0, 1, 3, 2)) * qkv.dtype.type(1.0 / math.sqrt(dh))
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(batch * T, D)


def e4m3(a):
    import oracle_lib as O
    return O.quant_e4m3(np.asarray(a, dtype=np.float32))


def bf16(a):
    import oracle_lib as O
    return O.round_bf16(np.asarray(a, dtype=np.float32))


def qrows(w):
    """e4m3 row quantiser: decoded values and per-row scales (oracle_quantize_rows)."""
    import oracle_lib as O
    _, wq, sc = O.quantize_rows(np.asarray(w, dtype=np.float32))
    return wq, sc


def linear_f8(a8, w, b):
    wq, sc = qrows(w)
    return (a8 @ wq.T) * sc + b


def ln_linear_f8_folded(x, lnw, lnb, W, B, eps):
    """oracle/vit_oracle.c ln_linear_f8_folded: e4m3 of the RAW rows times the quantised gamma o W, statistics in the epilogue."""
    wq, sc = qrows(lnw[None, :] * W)
    c = (wq.astype(np.float64).sum(1) * sc).astype(np.float32)
    d = (W.astype(np.float64) @ lnb.astype(np.float64) + B).astype(np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean(1)
    rstd = 1.0 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + eps)
    acc = e4m3(x) @ wq.T
    return (rstd[:, None].astype(np.float32) * (acc * sc - mean[:, None].astype(np.float32) * c) + d).astype(np.float32)


def patch_embed(cfg, t, images):
    """[batch, NP, D]: patches in NHWC order against the conv kernel [D][c][ky][kx] permuted to [D][ky][kx][c], plus the bias."""
    D, P, CH = cfg["dim"], cfg["patch_size"], cfg["channels"]
    g = cfg["image_size"] // P
    batch = images.shape[0]
    col = images.reshape(batch, g, P, g, P, CH).transpose(0, 1, 3, 2, 4, 5).reshape(batch * g * g, P * P * CH)
    pw = t["patch.weight"].transpose(0, 2, 3, 1).reshape(D, P * P * CH)
    return (col @ pw.T + t["patch.bias"]).reshape(batch, g * g, D)


def assemble(emb, cls, pos, reg=None):
    """Token assembly: emb [batch, NP, D] -> x [batch, tokens, D] in the row order of the module docstring.  cls is None: NO_CLS."""
    batch, NP, D = emb.shape
    R = 0 if reg is None else reg.shape[0]
    c = 0 if cls is None else 1
    assert pos.shape == (NP + c, D), (pos.shape, NP, D)
    x = np.empty((batch, c + R + NP, D), dtype=emb.dtype)
    if c:
        x[:, 0] = cls + pos[0]
    if R:
        x[:, c:c + R] = reg
    x[:, c + R:] = emb + pos[c:]
    return x


def layer(x, p, act, batch, T, H, dh, eps, fp8=None):
    """One transformer layer over the residual rows x [batch * T, D]; p(name) is the layer's tensor, e.g. p("q.weight")."""
    wqkv = np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")])
    bqkv = np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
    if fp8 == "folded":
        qkv = bf16(ln_linear_f8_folded(x, p("ln1.weight"), p("ln1.bias"), wqkv, bqkv, eps))
        x = x + linear_f8(e4m3(attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
        hid = e4m3(act(ln_linear_f8_folded(x, p("ln2.weight"), p("ln2.bias"), p("fc1.weight"), p("fc1.bias"), eps)))
        return (x + linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
    if fp8:
        y = e4m3(layernorm(x, p("ln1.weight"), p("ln1.bias"), eps))
        qkv = bf16(linear_f8(y, wqkv, bqkv))
        x = x + linear_f8(e4m3(attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
        y = e4m3(layernorm(x, p("ln2.weight"), p("ln2.bias"), eps))
        hid = e4m3(act(linear_f8(y, p("fc1.weight"), p("fc1.bias")).astype(np.float32)))
        return (x + linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
    y = layernorm(x, p("ln1.weight"), p("ln1.bias"), eps)
    x = x + attention(y @ wqkv.T + bqkv, batch, T, H, dh) @ p("o.weight").T + p("o.bias")
    y = layernorm(x, p("ln2.weight"), p("ln2.bias"), eps)
    return x + act(y @ p("fc1.weight").T + p("fc1.bias")) @ p("fc2.weight").T + p("fc2.bias")


def head_input(x, lnw, lnb, eps, lead, pool):
    """x [batch, T, D] -> the head's input [batch, W]; `lead` rows (class token, registers) stand in front of the patch rows."""
    ln = lambda v: layernorm(v, lnw, lnb, eps)
    if pool == POOL_CLS:
        return ln(x[:, 0])
    if pool == POOL_AVG_NORM:
        return ln(x[:, lead:]).mean(1)
    if pool == POOL_AVG_FCNORM:
        return ln(x[:, lead:].mean(1))
    return np.concatenate([ln(x[:, 0]), ln(x[:, lead:]).mean(1)], -1)


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, all_hidden=False,
            want_head=False):
    """logits [batch, classes], followed by what is asked for, in this order: want_hidden or all_hidden: the residual rows
    [batch * tokens, dim] after `n_layers` layers (n_layers = 0: the embedded rows, after the pre-LayerNorm if there is one);
    all_hidden: the list of the rows after 0, 1, .. layers; want_head: the head's input [batch, W].  A bare array when nothing is
    asked for.  fp8: None, "plain" or "folded" (float32 only)."""
    f = dtype if fp8 is None else np.float32
    t = {k: v.astype(f) for k, v in unpack_blob(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = quick_gelu if flags & FLAG_QUICK_GELU else gelu
    x = assemble(patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    assert T == tokens(cfg, flags)
    x = x.reshape(batch * T, D)
    if flags & FLAG_PRE_LN:
        x = layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    hidden = [x]
    for l in range(cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])):
        x = layer(x, lambda n: t[f"l{l}.{n}"], act, batch, T, H, D // H, ln_eps, fp8)
        hidden.append(x)
    lead = T - (S.tokens(cfg) - 1)
    hin = head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden or all_hidden else ()) + ((hidden,) if all_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


def final_norm(cfg, blob, x, flags=0, ln_eps=1e-6):
    """The model's final LayerNorm over residual rows x [rows, dim] (DINOv2's last_hidden_state), in x's float type."""
    t = unpack_blob(cfg, blob, flags)
    return layernorm(x, t["lnf.weight"].astype(x.dtype), t["lnf.bias"].astype(x.dtype), ln_eps)
