#!/usr/bin/env python3
"""Generate tests/golden/pool/*.npz -- the vectors that pin tests/vit_ref.py (and through it the device) on the pooled heads and
on models without a class token.  Four micro cases, each an independent implementation from `transformers`, built from a random
config (no download), eager attention, float64, loaded with this repository's seeded tensors (vit_ref.make_tensors) under the
Hugging Face names, evaluated on seeded images, layer_norm_eps = 1e-6:
  ijepa_a      IJepaForImageClassification                 NO_CLS | POOL_AVG_NORM   shape A
  dinov2_a     Dinov2ForImageClassification                POOL_CLS_AVG             shape A, seeded LayerScale (hf_state_dicts.layer_scale)
  dinov2reg_b  Dinov2WithRegistersForImageClassification   POOL_CLS_AVG, R = 4      shape B, seeded LayerScale
  beit_a       BeitForImageClassification                  POOL_AVG_FCNORM          shape A; use_mean_pooling, absolute positions, no
               relative positions, no LayerScale.  BEiT has no key bias: the fixture's k.bias is zero.  Its encoder's final norm is
               the identity and pooler.layernorm is lnf.
  shape A = image 40, patch 8 (NP 25), dim 256, heads 4, mlp 512, 2 layers, 8 classes (the fold + split-residual path)
  shape B = image 32, patch 8 (NP 16), dim 128, heads 2, mlp 256, 2 layers, 8 classes (the fp32 residual path)
Each file stores the logits [batch, classes], the head's input [batch, W] (what `classifier` is called with) and last_hidden_state
[batch, T, D], plus the meta; weights are regenerated from the seeds and not stored.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_pool.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import (BeitConfig, BeitForImageClassification, Dinov2Config, Dinov2ForImageClassification,
                          Dinov2WithRegistersConfig, Dinov2WithRegistersForImageClassification, IJepaConfig,
                          IJepaForImageClassification)

import hf_state_dicts as H
import vh_synth as S
import vit_ref as PR

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-6
A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=8)
B = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=8)
CASES = [  # (name, kind, config, flags, weight seed, image seed, batch)
    ("ijepa_a", "ijepa", A, PR.FLAG_NO_CLS | PR.FLAG_POOL(PR.POOL_AVG_NORM), 81, 82, 3),
    ("dinov2_a", "dinov2", A, PR.FLAG_POOL(PR.POOL_CLS_AVG), 83, 84, 3),
    ("dinov2reg_b", "dinov2", B, PR.FLAG_POOL(PR.POOL_CLS_AVG) | PR.FLAG_REGISTERS(4), 85, 86, 3),
    ("beit_a", "beit", A, PR.FLAG_POOL(PR.POOL_AVG_FCNORM), 87, 88, 3),
]


def beit_state_dict(cfg, t):
    D = cfg["dim"]
    sd, e = {}, "beit.embeddings."
    sd[e + "cls_token"], sd[e + "position_embeddings"] = t["cls"].reshape(1, 1, D), t["pos"].reshape(1, -1, D)
    sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
    for l in range(cfg["layers"]):
        b = f"beit.layers.{l}."
        for ours, theirs in H.HF_LAYER_NAMES:
            sd[b + theirs + ".weight"] = t[f"l{l}.{ours}.weight"]
            if ours != "k":
                sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.bias"]
    sd["beit.pooler.layernorm.weight"], sd["beit.pooler.layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    sd["classifier.weight"], sd["classifier.bias"] = t["head.weight"], t["head.bias"]
    return sd


def hf_model(kind, cfg, flags, sd):
    common = dict(hidden_size=cfg["dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], image_size=cfg["image_size"],
                  patch_size=cfg["patch_size"], num_channels=cfg["channels"], layer_norm_eps=EPS, hidden_act="gelu",
                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_labels=cfg["classes"])
    if kind == "ijepa":
        hc, cls = IJepaConfig(intermediate_size=cfg["mlp_dim"], qkv_bias=True, **common), IJepaForImageClassification
    elif kind == "beit":
        hc = BeitConfig(intermediate_size=cfg["mlp_dim"], use_mean_pooling=True, use_absolute_position_embeddings=True,
                        use_relative_position_bias=False, use_shared_relative_position_bias=False, layer_scale_init_value=0.0,
                        drop_path_rate=0.0, use_mask_token=False, **common)
        cls = BeitForImageClassification
    else:
        regs = PR.registers_of(flags)
        kw = dict(mlp_ratio=cfg["mlp_dim"] // cfg["dim"], qkv_bias=True, use_swiglu_ffn=False, drop_path_rate=0.0, **common)
        hc = Dinov2WithRegistersConfig(num_register_tokens=regs, **kw) if regs else Dinov2Config(**kw)
        cls = Dinov2WithRegistersForImageClassification if regs else Dinov2ForImageClassification
    hc._attn_implementation = "eager"
    m = cls(hc).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(torch.float64)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "pool"), exist_ok=True)
    for name, kind, cfg, flags, wseed, iseed, batch in CASES:
        t = H.fixture_tensors(kind, cfg, flags, wseed)
        sd = {"ijepa": lambda: H.ijepa_state_dict(cfg, t), "beit": lambda: beit_state_dict(cfg, t),
              "dinov2": lambda: H.dinov2_classifier_state_dict(cfg, t, wseed)}[kind]()
        images = S.make_images(cfg, iseed, batch)
        m = hf_model(kind, cfg, flags, sd)
        seen = {}
        m.classifier.register_forward_hook(lambda mod, inp, out: seen.__setitem__("head_input", inp[0].detach().numpy().copy()))
        px = torch.from_numpy(images.transpose(0, 3, 1, 2).copy()).to(torch.float64)
        with torch.no_grad():
            logits = m(pixel_values=px).logits.numpy()
            last = getattr(m, m.base_model_prefix)(pixel_values=px).last_hidden_state.numpy()
        T, W = PR.tokens(cfg, flags), PR.head_width(cfg, flags)
        assert logits.shape == (batch, cfg["classes"]) and seen["head_input"].shape == (batch, W) and last.shape == (batch, T, cfg["dim"]), \
            (logits.shape, seen["head_input"].shape, last.shape)
        path = os.path.join(HERE, "pool", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, flags], dtype=np.int64), kind=np.array(kind),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(EPS),
                            logits=logits, head_input=seen["head_input"], last_hidden_state=last,
                            weights_checksum=np.array([float(v.astype(np.float64).sum()) for v in t.values()][:8]),
                            images_checksum=np.array([float(images.astype(np.float64).sum())]))
        print(name, "logits[0,:3] =", logits[0, :3], "->", os.path.relpath(path, HERE), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
