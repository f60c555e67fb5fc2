"""Reference forward for the two CLIP switches (TEST INFRASTRUCTURE): VH_FLAG_PRE_LN and VH_FLAG_QUICK_GELU.

The C oracle (oracle/) has neither switch, so the CLIP tests bring their own reference: a numpy forward in float32 or float64
over the canonical blob, written from the model's definition, with
  * pre_ln   a LayerNorm over the embedded tokens in front of layer 0 (CLIP's ln_pre),
  * quick    x * sigmoid(1.702 x) instead of erf GELU in the MLP,
and an emulation of the VH_DTYPE_FP8 data flow (e4m3 operands through oracle_lib's quantisers; the same rounding points as
oracle/vit_oracle.c oracle_vit_forward_fp8 / _fp8_folded) for the statistical fp8 criterion.  With neither switch it is the
oracle's function (tests/test_clip.py ties the two together on vit_micro).

It also states the blob layout with the two new tensors, in numpy, on top of vh_synth (which is not edited): pre_ln.weight [D]
and pre_ln.bias [D] directly after `pos`, tensor ids 5 and 6, sigma and offset of the other LayerNorms; header flags word
(byte 52) bit 1 = pre-LN, bit 2 = QuickGELU.
"""
from __future__ import annotations

import math

import numpy as np

import vh_synth as S

FLAG_PRE_LN, FLAG_QUICK_GELU = 16, 32
TID_PRE_LN_W, TID_PRE_LN_B = 5, 6
HDR_PRE_LN, HDR_QUICK_GELU = 2, 4
_erf = np.vectorize(math.erf, otypes=[np.float64])


def tensor_table(cfg, flags=0):
    """vh_synth.tensor_table with pre_ln.weight / pre_ln.bias after `pos` when FLAG_PRE_LN is set."""
    t = S.tensor_table(cfg)
    if flags & FLAG_PRE_LN:
        D = cfg["dim"]
        i = [n for n, *_ in t].index("pos") + 1
        t[i:i] = [("pre_ln.weight", (D,), TID_PRE_LN_W, 0.05, 1.0), ("pre_ln.bias", (D,), TID_PRE_LN_B, 0.02, 0.0)]
    return t


def blob_bytes(cfg, flags=0):
    return 64 + 4 * sum(int(np.prod(s)) for _, s, *_ in tensor_table(cfg, flags))


def blob_header(cfg, flags=0, ln_eps=1e-6):
    h = S.blob_header(cfg, ln_eps)
    bits = (HDR_PRE_LN if flags & FLAG_PRE_LN else 0) | (HDR_QUICK_GELU if flags & FLAG_QUICK_GELU else 0)
    h[52:56] = np.array([bits], dtype=np.uint32).view(np.uint8)
    return h


def make_tensors(cfg, seed, flags=0):
    return {name: S.fill(int(np.prod(shape)), seed, tid, 1, sigma, off).reshape(shape)
            for name, shape, tid, sigma, off in tensor_table(cfg, flags)}


def make_clip_tensors(cfg, seed, flags):
    """The seeded tensors as a CLIP tower holds them: no patch-convolution bias, no projection bias (both zero)."""
    t = make_tensors(cfg, seed, flags)
    t["patch.bias"] = np.zeros_like(t["patch.bias"])
    t["head.bias"] = np.zeros_like(t["head.bias"])
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


def _attention(qkv, batch, T, H, dh):
    D = H * dh
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(batch, T, H, dh).transpose(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(0, 1, 3, 2)) * qkv.dtype.type(1.0 / math.sqrt(dh))
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(batch * T, D)


def _e4m3(a):
    import oracle_lib as O
    return O.quant_e4m3(np.asarray(a, dtype=np.float32))


def _bf16(a):
    import oracle_lib as O
    return O.round_bf16(np.asarray(a, dtype=np.float32))


def _qrows(w):
    """e4m3 row quantiser: decoded values and per-row scales (oracle_quantize_rows)."""
    import oracle_lib as O
    _, wq, sc = O.quantize_rows(np.asarray(w, dtype=np.float32))
    return wq, sc


def _linear_f8(a8, w, b):
    wq, sc = _qrows(w)
    return (a8 @ wq.T) * sc + b


def _ln_linear_f8_folded(x, lnw, lnb, W, B, eps):
    """oracle/vit_oracle.c ln_linear_f8_folded: e4m3 of the RAW rows times the quantised gamma o W, statistics in the epilogue."""
    wq, sc = _qrows(lnw[None, :] * W)
    c = (wq.astype(np.float64).sum(1) * sc).astype(np.float32)
    d = (W.astype(np.float64) @ lnb.astype(np.float64) + B).astype(np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean(1)
    rstd = 1.0 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + eps)
    acc = _e4m3(x) @ wq.T
    return (rstd[:, None].astype(np.float32) * (acc * sc - mean[:, None].astype(np.float32) * c) + d).astype(np.float32)


def forward(cfg, blob, images, flags=0, ln_eps=1e-6, dtype=np.float64, n_layers=-1, want_hidden=False, fp8=None):
    """logits [batch, classes] (and, want_hidden, the residual rows [batch * tokens, dim] after `n_layers` layers: with
    n_layers = 0 the embedded rows AFTER the pre-LayerNorm).  fp8: None, "plain" or "folded" (float32 only)."""
    f = dtype if fp8 is None else np.float32
    t = {k: v.astype(f) for k, v in unpack_blob(cfg, blob, flags).items()}
    D, H, P, CH = cfg["dim"], cfg["heads"], cfg["patch_size"], cfg["channels"]
    dh, g = D // H, cfg["image_size"] // cfg["patch_size"]
    T = g * g + 1
    images = np.asarray(images, dtype=f)
    batch = images.shape[0]
    act = quick_gelu if flags & FLAG_QUICK_GELU else gelu
    # patches in NHWC order against the conv kernel [D][c][ky][kx] permuted to [D][ky][kx][c]
    col = images.reshape(batch, g, P, g, P, CH).transpose(0, 1, 3, 2, 4, 5).reshape(batch * g * g, P * P * CH)
    pw = t["patch.weight"].transpose(0, 2, 3, 1).reshape(D, P * P * CH)
    emb = (col @ pw.T + t["patch.bias"]).reshape(batch, g * g, D)
    x = np.empty((batch, T, D), dtype=f)
    x[:, 0] = t["cls"] + t["pos"][0]
    x[:, 1:] = emb + t["pos"][1:]
    x = x.reshape(batch * T, D)
    if flags & FLAG_PRE_LN:
        x = layernorm(x, t["pre_ln.weight"], t["pre_ln.bias"], ln_eps)
    L = cfg["layers"] if n_layers < 0 else min(n_layers, cfg["layers"])
    for l in range(L):
        p = lambda n: t[f"l{l}.{n}"]
        wqkv = np.concatenate([p("q.weight"), p("k.weight"), p("v.weight")])
        bqkv = np.concatenate([p("q.bias"), p("k.bias"), p("v.bias")])
        if fp8 == "folded":
            qkv = _bf16(_ln_linear_f8_folded(x, p("ln1.weight"), p("ln1.bias"), wqkv, bqkv, ln_eps))
            x = x + _linear_f8(_e4m3(_attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
            hid = _e4m3(act(_ln_linear_f8_folded(x, p("ln2.weight"), p("ln2.bias"), p("fc1.weight"), p("fc1.bias"), ln_eps)))
            x = (x + _linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
        elif fp8:
            y = _e4m3(layernorm(x, p("ln1.weight"), p("ln1.bias"), ln_eps))
            qkv = _bf16(_linear_f8(y, wqkv, bqkv))
            x = x + _linear_f8(_e4m3(_attention(qkv, batch, T, H, dh)), p("o.weight"), p("o.bias"))
            y = _e4m3(layernorm(x, p("ln2.weight"), p("ln2.bias"), ln_eps))
            hid = _e4m3(act(_linear_f8(y, p("fc1.weight"), p("fc1.bias")).astype(np.float32)))
            x = (x + _linear_f8(hid, p("fc2.weight"), p("fc2.bias"))).astype(np.float32)
        else:
            y = layernorm(x, p("ln1.weight"), p("ln1.bias"), ln_eps)
            x = x + _attention(y @ wqkv.T + bqkv, batch, T, H, dh) @ p("o.weight").T + p("o.bias")
            y = layernorm(x, p("ln2.weight"), p("ln2.bias"), ln_eps)
            x = x + act(y @ p("fc1.weight").T + p("fc1.bias")) @ p("fc2.weight").T + p("fc2.bias")
    cls = layernorm(x.reshape(batch, T, D)[:, 0], t["lnf.weight"], t["lnf.bias"], ln_eps)
    logits = cls @ t["head.weight"].T + t["head.bias"]
    return (logits, x) if want_hidden else logits
