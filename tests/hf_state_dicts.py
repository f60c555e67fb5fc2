"""Other projects' checkpoint names and the recipes of the `transformers` fixtures (TEST INFRASTRUCTURE): vit_ref's seeded tensors
as the state dicts of numpy arrays that the converters take, so that the CPU tests rebuild a fixture's model without torch or
transformers, and tests/golden/make_golden_{clip,reg,pool}.py load the same tensors into the Hugging Face models."""
from __future__ import annotations

import numpy as np

import vh_synth as S
import vit_ref as R

# The DINOv2 model of a fixture = the seeded tensors + seeded LayerScale vectors with tensor ids of the fixture scripts' own
# (uniform in 0.5 .. 1.5).
TID_LS1, TID_LS2 = 0x6000, 0x6100   # + layer
HF_LAYER_NAMES = (("ln1", "layernorm_before"), ("q", "attention.q_proj"), ("k", "attention.k_proj"), ("v", "attention.v_proj"),
                  ("o", "attention.o_proj"), ("ln2", "layernorm_after"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))


def make_clip_tensors(cfg, seed, flags):
    """The seeded tensors as a CLIP tower holds them: no patch-convolution bias, no projection bias (both zero)."""
    t = R.make_tensors(cfg, seed, flags)
    t["patch.bias"] = np.zeros_like(t["patch.bias"])
    t["head.bias"] = np.zeros_like(t["head.bias"])
    return t


def fixture_tensors(kind, cfg, flags, wseed):
    """The seeded tensors of a tests/golden/pool case.  BEiT has no key bias: there k.bias is zero."""
    t = R.make_tensors(cfg, wseed, flags)
    if kind == "beit":
        for l in range(cfg["layers"]):
            t[f"l{l}.k.bias"] = np.zeros_like(t[f"l{l}.k.bias"])
    return t


def layer_scale(cfg, seed, l):
    D = cfg["dim"]
    return (1.0 + 0.5 * S.fill(D, seed, TID_LS1 + l, 0).astype(np.float64)).astype(np.float32), \
           (1.0 + 0.5 * S.fill(D, seed, TID_LS2 + l, 0).astype(np.float64)).astype(np.float32)


def dinov2_state_dict(cfg, tensors, seed, unit_scale=False):
    """The seeded tensors (make_tensors) as a Hugging Face Dinov2(WithRegisters)Model state dict of numpy arrays."""
    D = cfg["dim"]
    t, sd, e = tensors, {}, "embeddings."
    sd[e + "cls_token"] = t["cls"].reshape(1, 1, D)
    sd[e + "mask_token"] = np.zeros((1, D), np.float32)
    sd[e + "position_embeddings"] = t["pos"].reshape(1, -1, D)
    if "reg" in t:
        sd[e + "register_tokens"] = t["reg"].reshape(1, -1, D)
    sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
    for l in range(cfg["layers"]):
        b = f"encoder.layer.{l}."
        for ours, theirs in (("ln1", "norm1"), ("q", "attention.attention.query"), ("k", "attention.attention.key"),
                             ("v", "attention.attention.value"), ("o", "attention.output.dense"), ("ln2", "norm2"),
                             ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
        l1, l2 = layer_scale(cfg, seed, l)
        sd[b + "layer_scale1.lambda1"] = np.ones_like(l1) if unit_scale else l1
        sd[b + "layer_scale2.lambda1"] = np.ones_like(l2) if unit_scale else l2
    sd["layernorm.weight"], sd["layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    return sd


def dinov2_classifier_state_dict(cfg, tensors, seed, unit_scale=False):
    """Seeded POOL_CLS_AVG tensors as a Dinov2(WithRegisters)ForImageClassification state dict (the backbone's names under
    `dinov2.` / `dinov2_with_registers.`, plus `classifier`)."""
    prefix = "dinov2_with_registers." if "reg" in tensors else "dinov2."
    sd = {prefix + k: v for k, v in dinov2_state_dict(cfg, tensors, seed, unit_scale).items()}
    sd["classifier.weight"], sd["classifier.bias"] = tensors["head.weight"], tensors["head.bias"]
    return sd


def ijepa_state_dict(cfg, tensors):
    """Seeded NO_CLS tensors as a Hugging Face IJepaForImageClassification state dict of numpy arrays."""
    D = cfg["dim"]
    t, sd, e = tensors, {}, "ijepa.embeddings."
    sd[e + "position_embeddings"] = t["pos"].reshape(1, -1, D)
    sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"] = t["patch.weight"], t["patch.bias"]
    for l in range(cfg["layers"]):
        b = f"ijepa.layers.{l}."
        for ours, theirs in HF_LAYER_NAMES:
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
    sd["ijepa.layernorm.weight"], sd["ijepa.layernorm.bias"] = t["lnf.weight"], t["lnf.bias"]
    sd["classifier.weight"], sd["classifier.bias"] = t["head.weight"], t["head.bias"]
    return sd
