#!/usr/bin/env python3
"""Generate tests/golden/clip/*.npz -- the vectors that pin tests/vit_ref.py (and through it the device) on the two CLIP
switches.  Three micro cases, each an independent implementation from `transformers`, built from a random config (no download),
loaded with this repository's seeded tensors, evaluated in float64 and float32 on seeded images, layer_norm_eps = 1e-5:
  clip_both     CLIPVisionModelWithProjection, hidden_act "quick_gelu"    VH_FLAG_PRE_LN | VH_FLAG_QUICK_GELU
  clip_preln    CLIPVisionModelWithProjection, hidden_act "gelu"          VH_FLAG_PRE_LN
  vit_quick     ViTForImageClassification,     hidden_act "quick_gelu"    VH_FLAG_QUICK_GELU
CLIP has no patch-convolution bias and no projection bias: the CLIP cases use hf_state_dicts.make_clip_tensors (both zero), and
`logits` is the model's image_embeds.  Same npz layout as make_golden_headdim.py plus `ln_eps`, `zero_bias` and the flags in
`meta`.  CLIP's hidden_states[0] is the encoder's input, i.e. the rows AFTER pre_layrnorm: the script checks that against
vit_ref with n_layers = 0 before it writes anything.

Needs torch + transformers (build container only).  Re-run:  python tests/golden/make_golden_clip.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection, ViTConfig, ViTForImageClassification

import hf_state_dicts as H
import vh_synth as S
import vit_ref as R

CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-5
MICRO = dict(image_size=64, patch_size=16, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=40)
MICRO_P8 = dict(image_size=32, patch_size=8, channels=3, dim=192, heads=3, mlp_dim=384, layers=2, classes=64)
PRE, QUICK = R.FLAG_PRE_LN, R.FLAG_QUICK_GELU
CASES = [("clip_both", MICRO, PRE | QUICK, 51, 52, 3, 24),     # (name, config, flags, weight seed, image seed, batch, hidden rows)
         ("clip_preln", MICRO_P8, PRE, 53, 54, 2, 16),
         ("vit_quick", MICRO, QUICK, 55, 56, 3, 24)]


def clip_model(cfg, t, flags, dtype):
    hc = CLIPVisionConfig(hidden_size=cfg["dim"], intermediate_size=cfg["mlp_dim"], projection_dim=cfg["classes"],
                          num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], num_channels=cfg["channels"],
                          image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                          hidden_act="quick_gelu" if flags & QUICK else "gelu", layer_norm_eps=EPS, attention_dropout=0.0)
    hc._attn_implementation = "eager"
    m = CLIPVisionModelWithProjection(hc).eval()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()}
    v, sd = "vision_model.", {}
    sd[v + "embeddings.class_embedding"] = t["cls"]
    sd[v + "embeddings.patch_embedding.weight"] = t["patch.weight"]
    sd[v + "embeddings.position_embedding.weight"] = t["pos"]
    sd[v + "pre_layrnorm.weight"], sd[v + "pre_layrnorm.bias"] = t["pre_ln.weight"], t["pre_ln.bias"]
    for l in range(cfg["layers"]):
        b = f"{v}encoder.layers.{l}."
        for ours, theirs in (("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"), ("v", "self_attn.v_proj"),
                             ("o", "self_attn.out_proj"), ("ln1", "layer_norm1"), ("ln2", "layer_norm2"),
                             ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
    sd[v + "post_layernorm.weight"], sd[v + "post_layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    sd["visual_projection.weight"] = t["head.weight"]
    own = m.state_dict()
    for k in list(own):           # buffers such as position_ids keep the model's own value
        if k not in sd:
            assert "position_ids" in k, k
            sd[k] = own[k]
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def vit_quick_model(cfg, t, dtype):
    from make_golden import hf_model   # the ViT mapping of the other fixtures; only the activation and eps differ
    hc = ViTConfig(hidden_size=cfg["dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                   intermediate_size=cfg["mlp_dim"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                   num_channels=cfg["channels"], layer_norm_eps=EPS, hidden_act="quick_gelu", qkv_bias=True,
                   num_labels=cfg["classes"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hc._attn_implementation = "eager"
    src = hf_model(cfg, t, torch.float32)
    m = ViTForImageClassification(hc).eval()
    m.load_state_dict(src.state_dict(), strict=True)
    return m.to(dtype)


def main():
    torch.set_num_threads(8)
    os.makedirs(os.path.join(HERE, "clip"), exist_ok=True)
    for name, cfg, flags, wseed, iseed, batch, rows in CASES:
        is_clip = bool(flags & PRE)
        tensors = H.make_clip_tensors(cfg, wseed, flags) if is_clip else R.make_tensors(cfg, wseed, flags)
        images = S.make_images(cfg, iseed, batch)
        nchw = torch.from_numpy(images.transpose(0, 3, 1, 2).copy())
        out = {}
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = clip_model(cfg, tensors, flags, dt) if is_clip else vit_quick_model(cfg, tensors, dt)
            with torch.no_grad():
                r = m(pixel_values=nchw.to(dt), output_hidden_states=True)
            out[f"logits_{tag}"] = (r.image_embeds if is_clip else r.logits).to(torch.float64).numpy()
            hs = r.hidden_states
            out[f"hidden_last_{tag}"] = hs[-1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
            out[f"hidden_l1_{tag}"] = hs[1].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
            out[f"embed_{tag}"] = hs[0].to(torch.float64).numpy().reshape(-1, cfg["dim"])[:rows]
        # which hidden state is the post-ln_pre one: hidden_states[0], the encoder's input
        blob = R.pack_blob(cfg, tensors, flags, EPS)
        _, x0 = R.forward(cfg, blob, images, flags, EPS, n_layers=0, want_hidden=True)
        d0 = float(np.abs(x0[:rows] - out["embed_f64"]).max())
        assert d0 < 1e-10, (name, d0)
        if is_clip:
            assert abs(float(out["embed_f64"].mean())) < 0.1 and float(out["embed_f64"].std()) > 0.5   # normalised rows
        out["weights_checksum"] = np.array([float(np.float64(v.astype(np.float64).sum())) for v in tensors.values()][:8])
        out["images_checksum"] = np.array([float(images.astype(np.float64).sum())])
        path = os.path.join(HERE, "clip", f"{name}_s{wseed}_i{iseed}_b{batch}.npz")
        np.savez_compressed(path, meta=np.array([wseed, iseed, batch, flags], dtype=np.int64),
                            config=np.array([cfg[k] for k in CFG_KEYS], dtype=np.int64), ln_eps=np.array(EPS),
                            zero_bias=np.array(int(is_clip)),
                            **{k: (v.astype(np.float32) if k.endswith("f32") else v) for k, v in out.items()})
        print(name, "hidden_states[0] vs vit_ref after ln_pre:", d0, "logits f64[0,:4] =", out["logits_f64"][0, :4], "->",
              os.path.relpath(path, HERE), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
