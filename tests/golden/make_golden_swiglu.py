#!/usr/bin/env python3
"""Generate tests/golden/swiglu/*.npz -- the vectors that pin tests/swiglu_ref.py (and through it the device) on the SwiGLU model flag.
Three micro cases of `transformers`, built from random configs (no download), eager attention, float64, loaded with this repository's
seeded tensors (swiglu_ref.fixture_state_dict) with a SPREAD of LayerScale values:
  a  Dinov2Model(use_swiglu_ffn), image 28, patch 14 (NP 4), dim 128, 2 heads, hidden 344 (padded to 384), 2 layers, batch 3   (the plain loop)
  b  Dinov2WithRegistersModel(use_swiglu_ffn), image 28, patch 14, dim 256, 4 heads, hidden 688 (padded to 768), 4 registers, batch 2   (the folded loop)
  c  DINOv3ViTModel(use_gated_mlp, hidden_act silu), image 24, patch 8 (NP 9), dim 256, 4 heads, intermediate 512, 4 registers, batch 2   (RoPE + gate)
Each file stores the images, last_hidden_state, pooler_output, for model c the model's own rope tables, and the meta.  The weights are
regenerated from the seed and not stored; state_checksum is the float64 sum of every tensor of the state dict.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_swiglu.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import DINOv3ViTConfig, DINOv3ViTModel, Dinov2Config, Dinov2Model, Dinov2WithRegistersConfig, Dinov2WithRegistersModel

import swiglu_ref as W

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


def hf_model(name, sd):
    kind, _, Mc, regs, *_ = W.FIXTURES[name]
    cfg = W.fixture_cfg(name)
    if kind == "dinov2":
        kw = dict(hidden_size=cfg["dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], mlp_ratio=4,
                  image_size=cfg["image_size"], patch_size=cfg["patch_size"], num_channels=cfg["channels"], layer_norm_eps=W.fixture_eps(name),
                  hidden_act="gelu", qkv_bias=True, layerscale_value=1.0, drop_path_rate=0.0, use_swiglu_ffn=True)
        c = Dinov2WithRegistersConfig(num_register_tokens=regs, **kw) if regs else Dinov2Config(**kw)
        c._attn_implementation = "eager"
        m = (Dinov2WithRegistersModel if regs else Dinov2Model)(c).eval()
        assert m.encoder.layer[0].mlp.weights_out.in_features == Mc, m.encoder.layer[0].mlp.weights_out.in_features
    else:
        c = DINOv3ViTConfig(patch_size=cfg["patch_size"], hidden_size=cfg["dim"], intermediate_size=Mc, num_hidden_layers=cfg["layers"],
                            num_attention_heads=cfg["heads"], hidden_act="silu", layer_norm_eps=W.fixture_eps(name), rope_theta=100.0,
                            image_size=cfg["image_size"], num_channels=cfg["channels"], query_bias=True, key_bias=True, value_bias=True,
                            proj_bias=True, mlp_bias=True, use_gated_mlp=True, num_register_tokens=regs)
        c._attn_implementation = "eager"
        m = DINOv3ViTModel(c).eval()
        prefix = "model.layer." if any(k.startswith("model.layer.") for k in m.state_dict()) else "layer."
        sd = {k.replace("model.layer.", prefix): v for k, v in sd.items()}
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(torch.float64)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "swiglu"), exist_ok=True)
    for name, (kind, _, Mc, regs, wseed, iseed, batch) in W.FIXTURES.items():
        cfg = W.fixture_cfg(name)
        sd = W.fixture_state_dict(name)
        images = W.fixture_images(name)
        m = hf_model(name, sd)
        px = torch.from_numpy(images.transpose(0, 3, 1, 2).copy()).to(torch.float64)
        extra = {}
        with torch.no_grad():
            r = m(pixel_values=px)
            if kind == "dinov3":
                cos, sin = m.rope_embeddings(px)
                extra = dict(rope_cos=cos.numpy(), rope_sin=sin.numpy())
        last, pooled = r.last_hidden_state.numpy(), r.pooler_output.numpy()
        NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
        assert last.shape == (batch, 1 + regs + NP, cfg["dim"]) and pooled.shape == (batch, cfg["dim"]), (last.shape, pooled.shape)
        path = os.path.join(HERE, "swiglu", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, regs, Mc], dtype=np.int64),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(W.fixture_eps(name)),
                            images=images, last_hidden_state=last, pooler_output=pooled,
                            state_checksum=np.array([sum(float(np.asarray(v, np.float64).sum()) for v in sd.values())]), **extra)
        print(name, "pooler_output[0,:3] =", pooled[0, :3], "->", os.path.relpath(path, HERE), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
