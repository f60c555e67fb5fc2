#!/usr/bin/env python3
"""Generate tests/golden/dinov3/*.npz -- the vectors that pin tests/vit_ref.py (and through it the device) on the rotary model flag.
Three micro cases of `transformers`' DINOv3ViTModel, built from a random config (no download), eager attention, float64, erf GELU,
layer_norm_eps = 1e-5, loaded with this repository's seeded tensors (hf_state_dicts.dinov3_state_dict) with a SPREAD of LayerScale values and q / k weights of two or four times the usual sigma (hf_state_dicts.QK_SCALE):
  a  image 40, patch 8 (NP 25), dim 256, 4 heads (hd 64), mlp 512, 2 layers, 4 registers, batch 3   (the fold + split-residual path)
  b  image 32, patch 8 (NP 16), dim 128, 2 heads (hd 64), mlp 256, 2 layers, 4 registers, batch 3   (the fp32-residual path)
  c  image 24, patch 8 (NP 9),  dim 320, 4 heads (hd 80), mlp 384, 2 layers, no register, no key bias, batch 2   (row-major head-dim kernel)
Each file stores the images, last_hidden_state [batch, tokens, dim], pooler_output [batch, dim], the model's own rope_embeddings output
(rope_cos / rope_sin [NP, hd] as the float64 model applies them: float32 coordinates and frequencies, float64 cosine and sine) and the meta.  The weights are regenerated from the seed and not
stored (4 MB at dim 256); state_checksum is the float64 sum of every tensor of the state dict.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_dinov3.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import DINOv3ViTConfig, DINOv3ViTModel

import hf_state_dicts as H

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


def hf_model(cfg, registers, key_bias, sd):
    c = DINOv3ViTConfig(patch_size=cfg["patch_size"], hidden_size=cfg["dim"], intermediate_size=cfg["mlp_dim"],
                        num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], hidden_act="gelu", layer_norm_eps=H.DINOV3_EPS,
                        rope_theta=100.0, image_size=cfg["image_size"], num_channels=cfg["channels"], query_bias=True, key_bias=key_bias,
                        value_bias=True, proj_bias=True, mlp_bias=True, use_gated_mlp=False, num_register_tokens=registers)
    c._attn_implementation = "eager"
    m = DINOv3ViTModel(c).eval()
    prefix = "model.layer." if any(k.startswith("model.layer.") for k in m.state_dict()) else "layer."
    sd = {k.replace("model.layer.", prefix): v for k, v in sd.items()}
    if registers == 0:   # the module keeps an empty parameter
        sd.setdefault("embeddings.register_tokens", np.zeros((1, 0, cfg["dim"]), np.float32))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(torch.float64)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "dinov3"), exist_ok=True)
    for name, (_, registers, key_bias, wseed, iseed, batch) in H.FIXTURES.items():
        cfg = H.fixture_cfg(name)
        sd = H.dinov3_state_dict(name)
        images = H.fixture_images(name)
        m = hf_model(cfg, registers, key_bias, sd)
        px = torch.from_numpy(images.transpose(0, 3, 1, 2).copy()).to(torch.float64)
        with torch.no_grad():
            r = m(pixel_values=px)
            cos, sin = m.rope_embeddings(px)
        last, pooled = r.last_hidden_state.numpy(), r.pooler_output.numpy()
        NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
        assert last.shape == (batch, 1 + registers + NP, cfg["dim"]) and pooled.shape == (batch, cfg["dim"]), (last.shape, pooled.shape)
        path = os.path.join(HERE, "dinov3", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, registers, int(key_bias)], dtype=np.int64),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(H.DINOV3_EPS),
                            images=images, last_hidden_state=last, pooler_output=pooled,
                            rope_cos=cos.numpy(), rope_sin=sin.numpy(),
                            state_checksum=np.array([sum(float(np.asarray(v, np.float64).sum()) for v in sd.values())]))
        print(name, "pooler_output[0,:3] =", pooled[0, :3], "->", os.path.relpath(path, HERE), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
