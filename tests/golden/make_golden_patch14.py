#!/usr/bin/env python3
"""Generate tests/golden/patch14/*.npz -- the vectors that pin the oracle on a patch-14 model (patch vector 14*14*3 = 588,
not a multiple of 64; patch row 14*3 = 42, not a multiple of 4).

The same independent implementation as make_golden.py (`transformers.ViTForImageClassification`, built by its `hf_model`,
loaded with this repo's seeded synthetic weights, evaluated in float64 and float32 on seeded synthetic images), the same
npz format.  The fixtures live in a subfolder: the top-level tests/golden/*.npz are looked up in vh_synth.CONFIGS, which
holds no patch-14 model; the configuration is written into the file instead.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_patch14.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import vh_synth as S
from make_golden import hf_model

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
PATCH14_MICRO = dict(image_size=56, patch_size=14, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=40)
CASES = [("patch14_micro", PATCH14_MICRO, 31, 32, 2)]   # (name, config, weight seed, image seed, batch)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "patch14"), exist_ok=True)
    for name, cfg, wseed, iseed, batch in CASES:
        tensors = S.make_tensors(cfg, wseed)
        images = S.make_images(cfg, iseed, batch)            # NHWC fp32
        nchw = torch.from_numpy(images.transpose(0, 3, 1, 2).copy())
        out = {}
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = hf_model(cfg, tensors, dt)
            with torch.no_grad():
                r = m(pixel_values=nchw.to(dt), output_hidden_states=True)
            out[f"logits_{tag}"] = r.logits.to(torch.float64).numpy()
            hs = r.hidden_states
            out[f"hidden_last_{tag}"] = hs[-1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:64]
            out[f"hidden_l1_{tag}"] = hs[1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:64]
            out[f"embed_{tag}"] = hs[0].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:64]
        out["weights_checksum"] = np.array(
            [float(np.float64(v.astype(np.float64).sum())) for v in tensors.values()][:8])
        out["images_checksum"] = np.array([float(images.astype(np.float64).sum())])
        meta = np.array([wseed, iseed, batch], dtype=np.int64)
        config = np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64)
        path = os.path.join(HERE, "patch14", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=meta, config=config,
                            **{k: (v.astype(np.float32) if k.endswith("f32") else v) for k, v in out.items()})
        print(name, "logits f64[0,:4] =", out["logits_f64"][0, :4], "->", os.path.relpath(path, HERE),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
