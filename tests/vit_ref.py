"""The reference model (TEST INFRASTRUCTURE): one numpy forward, in float32 or float64, for every model flag, and the one
description of the canonical blob with every optional tensor.  The C oracle (oracle/) knows none of the flags; with flags = 0 this
is the oracle's function and vh_synth's blob (tests/test_clip.py, tests/test_registers.py), and each flag is pinned by fixtures
computed with Hugging Face `transformers` (tests/golden/clip, reg, pool, siglip, dinov3; the recipes are in tests/hf_state_dicts.py).
A new model flag extends this module in place; tests/golden/ref_digests.json records its seeded blobs (tests/test_ref_digests.py).

The nine flags (the values of include/vithip.h, stated here independently; the tests compare the two):
  PRE_LN        a LayerNorm over the embedded tokens in front of layer 0 (CLIP's ln_pre)
  QUICK_GELU    x * sigmoid(1.702 x) instead of erf GELU in the MLP
  TANH_GELU     0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3))) instead (SigLIP); excludes QUICK_GELU
  REGISTERS(R)  R learned rows without a position row (DINOv2 "with registers", Hugging Face's hidden_states order)
  NO_CLS        no class-token row; legal with the two pool modes that do not read one, and with MAP_HEAD
  POOL(m)       what the head multiplies; p runs over the NP patch rows only, the LayerNorm is lnf.* in every mode:
                  POOL_CLS        head(LN(row 0))
                  POOL_AVG_NORM   head(mean_p LN(x_p))
                  POOL_AVG_FCNORM head(LN(mean_p x_p))
                  POOL_CLS_AVG    head(concat(LN(row 0), mean_p LN(x_p)))
  MAP_HEAD      the head's input is SigLIP's attention-pooling block; per image, t over the NP patch rows:
                  y_t = LN(x_t; lnf);  s[h,t] = qk[h] . y_t;  p[h,.] = softmax_t s[h,.];  z[h] = sum_t p[h,t] y_t
                  a[h hd + j] = v.weight[h hd + j] . z[h] + v.bias[h hd + j];  o = o.weight a + o.bias
                  u = o + fc2(act(fc1(LN(o; map.ln))));  logits = head(u)
                map.qk[h] = W_k,h^T (W_q,h probe + b_q,h) / sqrt(hd) is folded by whoever builds the blob (fold_qk, float64): the
                query is one learned vector, and the key bias shifts every score of a head by the same constant, which the softmax
                cancels.  literal_map() is the block as torch.nn.MultiheadAttention states it (K and V of every token, every
                in_proj bias).  Needs NO_CLS, POOL_CLS, no registers, at most MAX_HEADS heads.
  ROPE          in every layer, q and k of the patch rows (row lead + p of an image is patch p; the lead rows -- class token,
                registers -- are left alone) are rotated per head: for d < hd / 2, c = rope.cos[p][d], s = rope.sin[p][d]
                  out[d] = x[d] c - x[d + hd/2] s          out[d + hd/2] = x[d + hd/2] c + x[d] s
                (Hugging Face's rotate_half form).  v is not rotated.
  CLS_TAIL is no model flag (it moves no tensor and changes no result); legal() knows it because MAP_HEAD and ROPE exclude it.

Row order of one image, tokens = (1 or 0) + R + NP:
    row 0                cls + pos[0]                      (absent under NO_CLS, where pos has NP rows and patch p adds pos[p])
    the next R rows      reg[r]
    the last NP rows     patch embedding p + pos[1 + p]

Blob: vh_synth's 64-byte header and fp32 tensors in vh_synth.tensor_table's order, every tensor keeping its id, sigma and offset,
with  `cls` dropped and pos [NP][D] under NO_CLS;  reg [R][D] directly after `pos` (id 7, sigma as `cls`, offset 0);  then
pre_ln.weight [D], pre_ln.bias [D] (ids 5 and 6, sigma and offset of the other LayerNorms);  head.weight [C][2 D] under
POOL_CLS_AVG;  under MAP_HEAD, directly after head.bias: map.qk [H][D], map.v.weight [D][D], map.v.bias [D], map.o.weight [D][D],
map.o.bias [D], map.ln.weight [D], map.ln.bias [D], map.fc1.weight [M][D], map.fc1.bias [M], map.fc2.weight [D][M], map.fc2.bias [D]
(seeded tensor ids 0x7010 .. 0x701A in that order);  under ROPE, at the very end, rope.cos [NP][hd / 2] and rope.sin [NP][hd / 2]
(seeded: the angle a[i] = pi * u[i], u = the generator's uniform stream of tensor id 0x7030; cos(a) and sin(a) in float64, rounded
once).  The header's flags word (byte 52; bit 0 belongs to the file form's checksum): bit 1 = pre-LN, bit 2 = QuickGELU; the
register count, NO_CLS, the pool mode, MAP_HEAD, TANH_GELU and ROPE at their flag positions (bits 9 .. 13, 15, 16 .. 17, 19, 21, 23).

Rounding emulations of forward(), float32 only:  fp8 = "plain" / "folded": the VH_DTYPE_FP8 data flow, e4m3 operands through
oracle_lib's quantisers, the same rounding points as oracle/vit_oracle.c oracle_vit_forward_fp8 / _fp8_folded, q|k|v rounded to bf16.
q16 = a function that rounds an array to the 16-bit storage type: q|k|v are rounded when the projection stores them, and q and k of
the patch rows once more behind the rotation (the device's two rounding points under ROPE).
"""
from __future__ import annotations

import math
import re

import numpy as np

import vh_synth as S

FLAG_PRE_LN, FLAG_QUICK_GELU = 16, 32
FLAG_REGISTERS_MASK, FLAG_NO_CLS, FLAG_POOL_MASK = 31 << 9, 1 << 15, 3 << 16
FLAG_MAP_HEAD, FLAG_TANH_GELU, FLAG_ROPE = 1 << 19, 1 << 21, 1 << 23
CLS_TAIL = 8
POOL_CLS, POOL_AVG_NORM, POOL_AVG_FCNORM, POOL_CLS_AVG = range(4)
POOL_NAMES = {POOL_CLS: "cls", POOL_AVG_NORM: "avg_norm", POOL_AVG_FCNORM: "avg_fcnorm", POOL_CLS_AVG: "cls_avg"}
HDR_PRE_LN, HDR_QUICK_GELU = 2, 4
TID_PRE_LN_W, TID_PRE_LN_B, TID_REG, TID_MAP, TID_ROPE = 5, 6, 7, 0x7010, 0x7030
MAX_HEADS = 16
_erf = np.vectorize(math.erf, otypes=[np.float64])


def FLAG_REGISTERS(n):
    return (int(n) & 31) << 9


def registers_of(flags):
    return (int(flags) & FLAG_REGISTERS_MASK) >> 9


def FLAG_POOL(m):
    return (int(m) & 3) << 16


def pool_of(flags):
    return (int(flags) & FLAG_POOL_MASK) >> 16


def legal(cfg, flags):
    """The combinations vh_create accepts."""
    if (flags & FLAG_TANH_GELU and flags & FLAG_QUICK_GELU) or (flags & FLAG_ROPE and flags & CLS_TAIL):
        return False
    if flags & FLAG_MAP_HEAD:
        return bool(flags & FLAG_NO_CLS) and pool_of(flags) == POOL_CLS and registers_of(flags) == 0 and cfg["heads"] <= MAX_HEADS \
            and not flags & CLS_TAIL
    return not (flags & FLAG_NO_CLS) or pool_of(flags) in (POOL_AVG_NORM, POOL_AVG_FCNORM)      # the two modes that read no class token


# ---- layout -------------------------------------------------------------------------------------------------------------------
def tokens(cfg, flags=0):
    return S.tokens(cfg) - (1 if flags & FLAG_NO_CLS else 0) + registers_of(flags)


def head_width(cfg, flags=0):
    return cfg["dim"] * (2 if pool_of(flags) == POOL_CLS_AVG else 1)


def rope_shape(cfg):
    g = cfg["image_size"] // cfg["patch_size"]
    return (g * g, cfg["dim"] // cfg["heads"] // 2)


def tensor_table(cfg, flags=0):
    """[(name, shape, tensor_id, sigma, offset)] in blob order: vh_synth.tensor_table with the changes of the module docstring.  The two
    rope tensors share the id of their angle stream (sigma / offset unused)."""
    D, M, H, R, no_cls = cfg["dim"], cfg["mlp_dim"], cfg["heads"], registers_of(flags), bool(flags & FLAG_NO_CLS)
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
    if flags & FLAG_MAP_HEAD:
        sw, sb, sg = 0.02, 0.02, 0.05
        rows = [("map.qk", (H, D), sw, 0.0), ("map.v.weight", (D, D), sw, 0.0), ("map.v.bias", (D,), sb, 0.0), ("map.o.weight", (D, D), sw, 0.0),
                ("map.o.bias", (D,), sb, 0.0), ("map.ln.weight", (D,), sg, 1.0), ("map.ln.bias", (D,), sb, 0.0),
                ("map.fc1.weight", (M, D), sw, 0.0), ("map.fc1.bias", (M,), sb, 0.0), ("map.fc2.weight", (D, M), sw, 0.0), ("map.fc2.bias", (D,), sb, 0.0)]
        out += [(n, s, TID_MAP + i, sig, off) for i, (n, s, sig, off) in enumerate(rows)]
    if flags & FLAG_ROPE:
        out += [("rope.cos", rope_shape(cfg), TID_ROPE, None, None), ("rope.sin", rope_shape(cfg), TID_ROPE, None, None)]
    return out


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = S.blob_header(cfg, ln_eps)
    bits = (HDR_PRE_LN if flags & FLAG_PRE_LN else 0) | (HDR_QUICK_GELU if flags & FLAG_QUICK_GELU else 0) \
        | (int(flags) & (FLAG_REGISTERS_MASK | FLAG_NO_CLS | FLAG_POOL_MASK | FLAG_MAP_HEAD | FLAG_TANH_GELU | FLAG_ROPE))
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def seeded_tables(cfg, seed):
    shape = rope_shape(cfg)
    a = math.pi * S.fill(int(np.prod(shape)), seed, TID_ROPE, 0).astype(np.float64)
    return np.cos(a).astype(np.float32).reshape(shape), np.sin(a).astype(np.float32).reshape(shape)


def make_tensors(cfg, seed, flags=0):
    t = {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape)
         for name, shape, tid, sigma, off in tensor_table(cfg, flags) if tid != TID_ROPE}
    if flags & FLAG_ROPE:
        t["rope.cos"], t["rope.sin"] = seeded_tables(cfg, seed)
    return t


def without_cls(tensors):
    """The tensors of the class-token model of the same patch rows -> the NO_CLS model's: no `cls`, pos without its row 0."""
    t = {k: v for k, v in tensors.items() if k != "cls"}
    t["pos"] = np.ascontiguousarray(tensors["pos"][1:])
    return t


def without_rope(cfg, blob, flags):
    """The same model with the flag cleared: the blob minus its last two tensors, the header bit cleared.  -> (blob, flags)"""
    assert flags & FLAG_ROPE
    n = 2 * 4 * int(np.prod(rope_shape(cfg)))
    out = np.ascontiguousarray(blob, dtype=np.uint8)[:-n].copy()
    bits = int(out[52:56].view(np.uint32)[0]) & ~FLAG_ROPE
    out[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return out, int(flags) & ~FLAG_ROPE


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


def weight_only_e4m3_blob(cfg, blob, flags=0):
    """The blob whose layers' q/k/v/o/fc1/fc2 matrices went through the oracle's e4m3 row quantiser and back (fp32 values)."""
    out = np.ascontiguousarray(blob, dtype=np.uint8).copy()
    for name, w in unpack_blob(cfg, out, flags).items():
        if re.fullmatch(r"l\d+\.(q|k|v|o|fc1|fc2)\.weight", name):
            wq, sc = qrows(w)
            w[...] = wq * sc[:, None]
    return out


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def quick_gelu(v):
    """x * sigmoid(1.702 x), overflow-free for every finite x (float64 or float32 in, same type out)."""
    v = np.asarray(v)
    z = np.exp(-np.abs(v) * v.dtype.type(1.702))
    return np.where(v >= 0, v / (1 + z), v * z / (1 + z))


def gelu(v):
    return (0.5 * v * (1.0 + _erf(v.astype(np.float64) * (1.0 / math.sqrt(2.0))))).astype(v.dtype)


def tanh_gelu(v):
    """0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3))) in v's float type."""
    v = np.asarray(v)
    f = v.dtype.type
    return f(0.5) * v * (f(1.0) + np.tanh(f(math.sqrt(2.0 / math.pi)) * (v + f(0.044715) * v * v * v)))


def activation(flags):
    return tanh_gelu if flags & FLAG_TANH_GELU else quick_gelu if flags & FLAG_QUICK_GELU else gelu


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


def fp16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


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


def layer(x, p, act, batch, T, H, dh, eps, fp8=None, rope=None, q16=None, want_qkv=False):
    """One transformer layer over the residual rows x [batch * T, D]; p(name) is the layer's tensor, e.g. p("q.weight").
    rope = (cos, sin, lead) or None: the rotation between the projection and attention.  want_qkv: q|k|v as attention reads them."""
    wqkv = np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")])
    bqkv = np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
    if fp8:
        q16 = bf16
    if fp8 == "folded":
        qkv = ln_linear_f8_folded(x, p("ln1.weight"), p("ln1.bias"), wqkv, bqkv, eps)
    elif fp8:
        qkv = linear_f8(e4m3(layernorm(x, p("ln1.weight"), p("ln1.bias"), eps)), wqkv, bqkv)
    else:
        qkv = layernorm(x, p("ln1.weight"), p("ln1.bias"), eps) @ wqkv.T + bqkv
    if q16 is not None:
        qkv = q16(qkv).astype(x.dtype)
    if rope is not None:
        qkv = rotate_qkv(qkv, rope[0], rope[1], batch, T, H, dh, rope[2], q16)
    if want_qkv:
        return qkv
    att = attention(qkv, batch, T, H, dh)
    if fp8:
        x = x + linear_f8(e4m3(att), p("o.weight"), p("o.bias"))
        if fp8 == "folded":
            hid = e4m3(act(ln_linear_f8_folded(x, p("ln2.weight"), p("ln2.bias"), p("fc1.weight"), p("fc1.bias"), eps)))
        else:
            y = e4m3(layernorm(x, p("ln2.weight"), p("ln2.bias"), eps))
            hid = e4m3(act(linear_f8(y, p("fc1.weight"), p("fc1.bias")).astype(np.float32)))
        return (x + linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
    x = x + att @ p("o.weight").T + p("o.bias")
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
    hid = act(layernorm(o, t["map.ln.weight"], t["map.ln.bias"], eps) @ t["map.fc1.weight"].T + t["map.fc1.bias"])
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


def _tensors(cfg, blob, flags):
    return blob if isinstance(blob, dict) else unpack_blob(cfg, blob, flags)


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None, all_hidden=False,
            want_head=False, q16=None, lead_probs=None):
    """`blob`: the blob, or its tensors as a dict of arrays of any float type, which need not have passed through fp32.
    logits [batch, classes], followed by what is asked for, in this order: want_hidden or all_hidden: the residual rows
    [batch * tokens, dim] after `n_layers` layers (n_layers = 0: the embedded rows, after the pre-LayerNorm if there is one);
    all_hidden: the list of the rows after 0, 1, .. layers; want_head: the head's input [batch, W] (MAP_HEAD: u).  A bare array when
    nothing is asked for.  fp8: None, "plain" or "folded"; q16: see the module docstring (both float32 only).
    lead_probs = (k, Q): instead, the softmax rows [batch][heads][Q][tokens] of the first Q queries of layer k (1-based)."""
    f = dtype if fp8 is None else np.float32
    t = {k: np.asarray(v).astype(f) for k, v in _tensors(cfg, blob, flags).items()}
    D, H = cfg["dim"], cfg["heads"]
    dh = D // H
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = activation(flags)
    x = assemble(patch_embed(cfg, t, images), t.get("cls"), t["pos"], t.get("reg"))
    T = x.shape[1]
    assert T == tokens(cfg, flags)
    lead = T - (S.tokens(cfg) - 1)
    rope = (t["rope.cos"], t["rope.sin"], lead) if flags & FLAG_ROPE else None
    x = x.reshape(batch * T, D)
    if flags & FLAG_PRE_LN:
        x = layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    hidden = [x]
    for l in range(cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])):
        p = lambda n: t[f"l{l}.{n}"]
        if lead_probs is not None and lead_probs[0] == l + 1:
            qkv = layer(x, p, act, batch, T, H, dh, ln_eps, fp8, rope, q16, want_qkv=True).reshape(batch, T, 3, H, dh)
            s = np.einsum("bqhd,bthd->bhqt", qkv[:, :lead_probs[1], 0], qkv[:, :, 1]) / math.sqrt(dh)
            e = np.exp(s - s.max(-1, keepdims=True))
            return e / e.sum(-1, keepdims=True)
        x = layer(x, p, act, batch, T, H, dh, ln_eps, fp8, rope, q16)
        hidden.append(x)
    assert lead_probs is None, "lead_probs names a layer that does not run"
    if flags & FLAG_MAP_HEAD:
        y = layernorm(x.reshape(batch, T, D)[:, lead:], t["lnf.weight"], t["lnf.bias"], ln_eps)
        hin = map_head(y, t, H, act, ln_eps)
    else:
        hin = head_input(x.reshape(batch, T, D), t["lnf.weight"], t["lnf.bias"], ln_eps, lead, pool_of(flags))
    logits = hin @ t["head.weight"].T + t["head.bias"]
    out = (logits,) + ((x,) if want_hidden or all_hidden else ()) + ((hidden,) if all_hidden else ()) + ((hin,) if want_head else ())
    return out if len(out) > 1 else logits


def final_norm(cfg, blob, x, flags=0, ln_eps=1e-6):
    """The model's final LayerNorm over residual rows x [rows, dim] (DINOv2's last_hidden_state), in x's float type."""
    t = _tensors(cfg, blob, flags)
    return layernorm(x, t["lnf.weight"].astype(x.dtype), t["lnf.bias"].astype(x.dtype), ln_eps)
