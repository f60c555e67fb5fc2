"""Reference of the attention rollout (include/vithip.h, "Attention rollout"; TEST INFRASTRUCTURE): float64 numpy, no GPU.

Everything is in the exp2 domain, as the kernel is: q arrives scaled by head_dim^-1/2 * log2(e).  q|k|v is row-major
[batch * T][3 * heads * hd]; R is [batch][T][T]."""
import math

import numpy as np

import attn_maps_ref as AM
import vit_ref as RR
import vithip

MEAN, MAX = vithip.ROLLOUT_MEAN, vithip.ROLLOUT_MAX


def fused64(qkv, batch, tokens, heads, hd, fusion):
    """A^ = rownorm(fuse_h softmax_h + I), float64 [batch][T][T]."""
    p = AM.probs64(qkv, batch, tokens, heads, hd, tokens)
    a = (p.mean(1) if fusion == MEAN else p.max(1)) + np.eye(tokens)
    return a / a.sum(-1, keepdims=True)


def step64(qkv, batch, tokens, heads, hd, fusion, r_prev=None):
    """One step: A^ R_prev (r_prev None: the identity)."""
    a = fused64(qkv, batch, tokens, heads, hd, fusion)
    return a if r_prev is None else a @ np.asarray(r_prev, dtype=np.float64)


def chain64(qkvs, batch, tokens, heads, hd, fusion, r0=None):
    r = r0
    for qkv in qkvs:
        r = step64(qkv, batch, tokens, heads, hd, fusion, r)
    return r


def model_qkv64(cfg, blob, images, flags=0, ln_eps=1e-6):
    """The float64 model's q|k|v of every layer as attention reads it (rotated under ROPE), q scaled into the exp2 domain."""
    t = {n: v.astype(np.float64) for n, v in RR.unpack_blob(cfg, blob, flags).items()}
    batch, D, H = len(images), cfg["dim"], cfg["heads"]
    hd, T = D // H, RR.tokens(cfg, flags)
    hidden = RR.forward(cfg, blob, images, flags, ln_eps=ln_eps, all_hidden=True)[2]
    rope = (t["rope.cos"], t["rope.sin"], T - (cfg["image_size"] // cfg["patch_size"]) ** 2) if flags & RR.FLAG_ROPE else None
    out = []
    for l in range(cfg["layers"]):
        qkv = RR.layer(np.asarray(hidden[l], dtype=np.float64), lambda n: t[f"l{l}.{n}"], RR.activation(flags), batch, T, H, hd, ln_eps, None, rope,
                       want_qkv=True).copy()
        qkv[:, :D] *= AM.LOG2E / math.sqrt(hd)
        out.append(qkv)
    return out
