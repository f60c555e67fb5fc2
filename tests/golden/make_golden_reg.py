#!/usr/bin/env python3
"""Generate tests/golden/reg/*.npz -- the vectors that pin tests/vit_ref.py (and through it the device) on register tokens.
Two micro cases, each an independent implementation: `transformers`' Dinov2WithRegistersModel, built from a random config (no
download), eager attention, float64, loaded with this repository's seeded tensors (vit_ref.make_tensors) under the Hugging Face
names plus seeded, non-trivial LayerScale vectors (hf_state_dicts.layer_scale: uniform in 0.5 .. 1.5, tensor ids 0x6000 + layer and
0x6100 + layer of the weight seed), evaluated on seeded images, layer_norm_eps = 1e-6:
  reg4_d128   image 56, patch 14, dim 128, heads 2, mlp 256, layers 2, R = 4, batch 3
  reg1_d256   image 32, patch 8,  dim 256, heads 4, mlp 512, layers 2, R = 1, batch 2   (dim 256: the fold and split-residual path)
Each file stores last_hidden_state [batch, T, D] (after the final LayerNorm), every hidden state [layers + 1, batch, T, D]
(hidden_states[0] = the embedded rows) and the meta; weights are regenerated from the seeds and not stored.  The row order is
the model's: class token, R register tokens, patch tokens.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_reg.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel

import hf_state_dicts as H
import vh_synth as S
import vit_ref as R

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-6
CASES = [  # (name, config, registers, weight seed, image seed, batch)
    ("reg4_d128", dict(image_size=56, patch_size=14, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=40), 4, 61, 62, 3),
    ("reg1_d256", dict(image_size=32, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=64), 1, 63, 64, 2),
]


def hf_model(cfg, sd, regs):
    hc = Dinov2WithRegistersConfig(hidden_size=cfg["dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                                   mlp_ratio=cfg["mlp_dim"] // cfg["dim"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                                   num_channels=cfg["channels"], num_register_tokens=regs, layer_norm_eps=EPS, hidden_act="gelu",
                                   qkv_bias=True, use_swiglu_ffn=False, hidden_dropout_prob=0.0,
                                   attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    hc._attn_implementation = "eager"
    m = Dinov2WithRegistersModel(hc).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(torch.float64)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "reg"), exist_ok=True)
    for name, cfg, regs, wseed, iseed, batch in CASES:
        assert cfg["mlp_dim"] % cfg["dim"] == 0
        flags = R.FLAG_REGISTERS(regs)
        tensors = R.make_tensors(cfg, wseed, flags)
        sd = H.dinov2_state_dict(cfg, tensors, wseed)
        images = S.make_images(cfg, iseed, batch)
        m = hf_model(cfg, sd, regs)
        with torch.no_grad():
            r = m(pixel_values=torch.from_numpy(images.transpose(0, 3, 1, 2).copy()).to(torch.float64), output_hidden_states=True)
        last = r.last_hidden_state.numpy()
        hidden = np.stack([h.numpy() for h in r.hidden_states])
        T = R.tokens(cfg, flags)
        assert last.shape == (batch, T, cfg["dim"]) and hidden.shape == (cfg["layers"] + 1, batch, T, cfg["dim"]), (last.shape, hidden.shape)
        # the embedded rows are the ones the row order of vit_ref.assemble states (independent of the LayerScale)
        x0 = R.forward(cfg, R.pack_blob(cfg, tensors, flags, EPS), images, flags, EPS, n_layers=0, want_hidden=True)[1]
        d0 = float(np.abs(x0.reshape(batch, T, -1) - hidden[0]).max())
        assert d0 < 1e-12, (name, d0)
        path = os.path.join(HERE, "reg", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, regs], dtype=np.int64),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(EPS),
                            last_hidden_state=last, hidden_states=hidden,
                            weights_checksum=np.array([float(v.astype(np.float64).sum()) for v in tensors.values()][:8]),
                            images_checksum=np.array([float(images.astype(np.float64).sum())]))
        print(name, "hidden_states[0] vs vit_ref.assemble:", d0, "last[0,0,:3] =", last[0, 0, :3], "->", os.path.relpath(path, HERE),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
