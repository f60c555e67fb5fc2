#!/usr/bin/env python3
"""Generate tests/golden/eva02/*.npz -- the vectors that pin tests/subln_ref.py, the EVA-02 converter's permutation and padding, and
through them the device on VH_FLAG_SUB_LN.  No timm was at hand: the model below is a plain float64 RESTATEMENT of timm's EVA-02 block
(interleaved rotary pairs (2 i, 2 i + 1) on the patch rows of q and k, a q / v bias only, SwiGLU with the LayerNorm in front of fc2),
written independently of vit_ref and of the converter, on the model's own tensors: unpermuted, unpadded.
  a  image 32, patch 8 (NP 16), dim 128, 2 heads, gated width 344 (padded to 384 by the converter), class-token head, batch 3  (plain loop)
  b  dim 256, 4 heads, gated width 688 (padded to 768), fc_norm mean-pool head, batch 3                                        (folded loop)
  c  as a, gated width 346 = 43 * 8 + 2 (padded to 384): the width ends inside a 16-byte chunk, as EVA-02-L's 2730 does       (plain loop)
Each file stores the images, the logits, the per-pair rotary tables the model used and the meta; the weights are regenerated from the
seed (subln_ref.fixture_state_dict: numpy's default_rng streams, stable by numpy's policy; fixture b's weights are 6 MB).  Re-run:  python tests/golden/make_golden_eva02.py   (numpy only)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import subln_ref as U

EPS = 1e-6


def ln(x, w, b):
    m = x.mean(-1, keepdims=True)
    return (x - m) / np.sqrt(((x - m) ** 2).mean(-1, keepdims=True) + EPS) * w + b


def rot_interleaved(x, cos, sin):
    """x [B, H, NP, hd]: the pair (x[2 i], x[2 i + 1]) turns by the angle of column i of cos / sin [NP, hd / 2]."""
    a, b = x[..., 0::2], x[..., 1::2]
    return np.stack([a * cos - b * sin, b * cos + a * sin], -1).reshape(x.shape)


def model(cfg, sd, images, n, mean):
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    D, H, P, g = cfg["dim"], cfg["heads"], cfg["patch_size"], cfg["image_size"] // cfg["patch_size"]
    hd, B = D // H, len(images)
    # rotary angles per pair: the first hd / 4 pairs turn with y, the others with x (the formula of vithip.rope_tables_eva02)
    bands = 10000.0 ** (-np.arange(hd // 4) / (hd // 4))
    yy, xx = (v.reshape(-1, 1).astype(np.float64) for v in np.meshgrid(np.arange(g), np.arange(g), indexing="ij"))
    ang = np.concatenate([yy * bands, xx * bands], 1)
    cos, sin = np.cos(ang), np.sin(ang)
    patches = np.asarray(images, np.float64).reshape(B, g, P, g, P, -1).transpose(0, 1, 3, 5, 2, 4).reshape(B, g * g, -1)   # NHWC -> (c, ky, kx)
    x = patches @ sd["patch_embed.proj.weight"].reshape(D, -1).T + sd["patch_embed.proj.bias"]
    x = np.concatenate([np.broadcast_to(sd["cls_token"], (B, 1, D)), x], 1) + sd["pos_embed"]
    silu = lambda v: v / (1 + np.exp(-v))
    for l in range(cfg["layers"]):
        p = lambda k: sd[f"blocks.{l}.{k}"]
        y = ln(x, p("norm1.weight"), p("norm1.bias"))
        heads = lambda v: v.reshape(B, -1, H, hd).transpose(0, 2, 1, 3)
        q, k, v = heads(y @ p("attn.q_proj.weight").T + p("attn.q_bias")), heads(y @ p("attn.k_proj.weight").T), heads(y @ p("attn.v_proj.weight").T + p("attn.v_bias"))
        q = np.concatenate([q[:, :, :1], rot_interleaved(q[:, :, 1:], cos, sin)], 2)
        k = np.concatenate([k[:, :, :1], rot_interleaved(k[:, :, 1:], cos, sin)], 2)
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        s = np.exp(s - s.max(-1, keepdims=True))
        o = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, -1, D)
        x = x + o @ p("attn.proj.weight").T + p("attn.proj.bias")
        y = ln(x, p("norm2.weight"), p("norm2.bias"))
        h = silu(y @ p("mlp.fc1_g.weight").T + p("mlp.fc1_g.bias")) * (y @ p("mlp.fc1_x.weight").T + p("mlp.fc1_x.bias"))
        assert h.shape[-1] == n
        x = x + ln(h, p("mlp.norm.weight"), p("mlp.norm.bias")) @ p("mlp.fc2.weight").T + p("mlp.fc2.bias")
    f = ln(x[:, 1:].mean(1), sd["fc_norm.weight"], sd["fc_norm.bias"]) if mean else ln(x, sd["norm.weight"], sd["norm.bias"])[:, 0]
    return f @ sd["head.weight"].T + sd["head.bias"], cos, sin


if __name__ == "__main__":
    os.makedirs(os.path.join(HERE, "eva02"), exist_ok=True)
    for name, (cfg, n, mean, seed, iseed, batch) in U.FIXTURES.items():
        images = U.fixture_images(name)
        logits, cos, sin = model(cfg, U.fixture_state_dict(name), images, n, mean)
        path = os.path.join(HERE, "eva02", f"{name}_s{seed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, images=images, logits=logits, rope_cos=cos, rope_sin=sin, meta=np.array([seed, iseed, batch, n, int(mean)]))
        print(path, os.path.getsize(path), "bytes; logits", float(np.abs(logits).max()), "top-1", logits.argmax(1))
