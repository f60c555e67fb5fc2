#!/usr/bin/env python3
"""Generate tests/golden/headdim/*.npz -- the vectors that pin the oracle on models whose head dim is not 64 (80: dim 320 over
4 heads; 128: dim 256 over 2 heads).

The same independent implementation as make_golden.py (`transformers.ViTForImageClassification`, built by its `hf_model`,
loaded with this repo's seeded synthetic weights, evaluated in float64 and float32 on seeded synthetic images), the same npz
format as make_golden_patch14.py, with the configuration written into the file.  The hidden-state taps keep the first
ROWS[name] rows (fewer than 64 at these widths, to keep each file near the patch-14 fixture's size).

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_headdim.py
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
HD80_MICRO = dict(image_size=64, patch_size=16, channels=3, dim=320, heads=4, mlp_dim=640, layers=2, classes=40)
HD128_MICRO = dict(image_size=64, patch_size=16, channels=3, dim=256, heads=2, mlp_dim=512, layers=2, classes=40)
CASES = [("hd80_micro", HD80_MICRO, 41, 42, 2, 12),     # (name, config, weight seed, image seed, batch, hidden rows)
         ("hd128_micro", HD128_MICRO, 43, 44, 2, 16)]


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "headdim"), exist_ok=True)
    for name, cfg, wseed, iseed, batch, rows in CASES:
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
            out[f"hidden_last_{tag}"] = hs[-1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
            out[f"hidden_l1_{tag}"] = hs[1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
            out[f"embed_{tag}"] = hs[0].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
        out["weights_checksum"] = np.array(
            [float(np.float64(v.astype(np.float64).sum())) for v in tensors.values()][:8])
        out["images_checksum"] = np.array([float(images.astype(np.float64).sum())])
        meta = np.array([wseed, iseed, batch], dtype=np.int64)
        config = np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64)
        path = os.path.join(HERE, "headdim", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=meta, config=config,
                            **{k: (v.astype(np.float32) if k.endswith("f32") else v) for k, v in out.items()})
        print(name, "logits f64[0,:4] =", out["logits_f64"][0, :4], "->", os.path.relpath(path, HERE),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
