#!/usr/bin/env python3
"""Generate tests/golden/siglip/*.npz -- the vectors that pin tests/vit_ref.py (and through it the device) on the two SigLIP flags,
tanh GELU and the attention-pooling head.  Three micro cases, each an independent implementation from `transformers`, built from a
random config (no download), eager attention, float64, hidden_act gelu_pytorch_tanh, layer_norm_eps = 1e-6, loaded with this
repository's seeded tensors (hf_state_dicts.siglip_tensors: the backbone's and the head's under our names, plus a seeded probe and seeded
q / k thirds of in_proj with ALL biases, so that the converter's fold -- and the key bias dropping out -- is part of what is pinned):
  vision_a  SiglipVisionModel             NO_CLS | MAP_HEAD | TANH_GELU         shape A, identity head: `pooler_output`
  vision_b  SiglipVisionModel             NO_CLS | MAP_HEAD | TANH_GELU         shape B
  cls_a     SiglipForImageClassification  NO_CLS | POOL_AVG_NORM | TANH_GELU    shape A, 8 classes: tanh GELU without the MAP head
  shape A = image 40, patch 8 (NP 25), dim 256, heads 4, mlp 512, 2 layers (the fold + split-residual path)
  shape B = image 32, patch 8 (NP 16), dim 128, heads 2, mlp 256, 2 layers (the fp32 residual path)
Each file stores `output` (pooler_output [batch, dim] or the logits [batch, classes]), last_hidden_state [batch, NP, dim] and the meta;
weights are regenerated from the seeds and not stored.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_siglip.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import SiglipConfig, SiglipForImageClassification, SiglipVisionConfig, SiglipVisionModel

import hf_state_dicts as H
import vh_synth as S

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-6
A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2)
B = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2)
CASES = [  # (name, classifier, config, weight seed, image seed, batch)
    ("vision_a", False, dict(A, classes=A["dim"]), 91, 92, 3),
    ("vision_b", False, dict(B, classes=B["dim"]), 93, 94, 3),
    ("cls_a", True, dict(A, classes=8), 95, 96, 3),
]


def hf_model(cfg, classifier, sd):
    vc = SiglipVisionConfig(hidden_size=cfg["dim"], intermediate_size=cfg["mlp_dim"], num_hidden_layers=cfg["layers"],
                            num_attention_heads=cfg["heads"], num_channels=cfg["channels"], image_size=cfg["image_size"],
                            patch_size=cfg["patch_size"], hidden_act="gelu_pytorch_tanh", layer_norm_eps=EPS, attention_dropout=0.0)
    vc._attn_implementation = "eager"
    if classifier:
        hc = SiglipConfig(vision_config=vc.to_dict(), num_labels=cfg["classes"])
        hc._attn_implementation = "eager"
        hc.vision_config._attn_implementation = "eager"
        m = SiglipForImageClassification(hc).eval()
    else:
        m = SiglipVisionModel(vc).eval()
    have = set(m.state_dict())
    if not classifier and not any(k.startswith("embeddings.") for k in have):   # releases that keep the tower under `vision_model.`
        sd = {"vision_model." + k: v for k, v in sd.items()}
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(torch.float64)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "siglip"), exist_ok=True)
    for name, classifier, cfg, wseed, iseed, batch in CASES:
        t, raw, flags = H.siglip_tensors(cfg, wseed, classifier)
        sd = H.siglip_state_dict(cfg, t, raw, classifier, prefix="vision_model." if classifier else "")
        images = S.make_images(cfg, iseed, batch)
        m = hf_model(cfg, classifier, sd)
        px = torch.from_numpy(images.transpose(0, 3, 1, 2).copy()).to(torch.float64)
        with torch.no_grad():
            if classifier:
                output = m(pixel_values=px).logits.numpy()
                last = m.vision_model(pixel_values=px).last_hidden_state.numpy()
            else:
                r = m(pixel_values=px)
                output, last = r.pooler_output.numpy(), r.last_hidden_state.numpy()
        NP = (cfg["image_size"] // cfg["patch_size"]) ** 2
        assert output.shape == (batch, cfg["classes"]) and last.shape == (batch, NP, cfg["dim"]), (output.shape, last.shape)
        path = os.path.join(HERE, "siglip", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, flags, int(classifier)], dtype=np.int64),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(EPS),
                            output=output, last_hidden_state=last,
                            images_checksum=np.array([float(images.astype(np.float64).sum())]))
        print(name, "output[0,:3] =", output[0, :3], "->", os.path.relpath(path, HERE), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
