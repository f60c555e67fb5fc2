#!/usr/bin/env python3
"""Fingerprint of the forward's launch sequence, for A/B runs of two builds that must compute the same thing the same way.

    tools/forward_fingerprint.py --tree <checkout with a built vit-fpga_amd/libvithip.so> [--context NAME]

For every context below -- the smallest at which each branch of enqueue_forward is taken -- it prints one line: the SHA-256 of the
logits of a seeded batch (init_weights_seeded(0), fill_input_seeded(1, ...)), debug taps 3 and 4 (tiled hidden activation,
head-major q|k|v) and the stages of profile_forward that recorded events, with their counts.  The "readout" contexts add the
SHA-256 of what the read-outs return for listed layers (read_outs below); "inflight" runs four steps of one asynchronous call, so
both activation sets and both compute streams take part.  Two builds agree when the two outputs are the same text.  Every context runs in a child process of its own (VH_GEMM_PP and the other knobs are read
once per process or per context); the first child that fails ends the run.
"""
import argparse
import glob
import hashlib
import os
import subprocess
import sys

import numpy as np

BF16, FP16, FP8 = 0, 1, 2
LN_FOLD_OFF, LN_FOLD_ON, W8_E4M3, CLS_TAIL, PRE_LN, QUICK_GELU = 1, 2, 4, 8, 16, 32
NO_CLS, MAP_HEAD, TANH_GELU, ROPE, SWIGLU = 1 << 15, 1 << 19, 1 << 21, 1 << 23, 1 << 25
POOL_AVG_NORM, POOL_CLS_AVG = 1 << 16, 3 << 16
REGISTERS_4 = 4 << 9
FEAT_NORM, FEAT_RAW = 0, 1   # vh_features.norm: through the final LayerNorm / the residual stream as it is

# name: (dtype, batch, flags, environment, extra)
CONTEXTS = {
    "fp16_b1": (FP16, 1, 0, {}, None),
    "fp16_b128": (FP16, 128, 0, {}, None),
    "fp16_b256": (FP16, 256, 0, {}, None),
    "fp16_b300": (FP16, 300, 0, {}, None),
    "fp16_b300_plain": (FP16, 300, LN_FOLD_OFF, {}, None),
    "fp16_b256_h_tiled_0": (FP16, 256, 0, {"VH_H_TILED": "0"}, None),
    "fp16_b256_att_tiled_0": (FP16, 256, 0, {"VH_ATT_TILED": "0"}, None),
    "fp16_b256_qkv_hm_0": (FP16, 256, 0, {"VH_QKV_HM": "0"}, None),
    "fp16_b256_resid_split_0": (FP16, 256, 0, {"VH_RESID_SPLIT": "0"}, None),
    "fp16_b256_cls_tail": (FP16, 256, CLS_TAIL, {}, None),
    "fp8_b256": (FP8, 256, 0, {}, None),
    "fp8_b256_h_tiled_0": (FP8, 256, 0, {"VH_H_TILED": "0"}, None),
    "fp8_b256_plain": (FP8, 256, LN_FOLD_OFF, {}, None),
    "bf16_b256_clip": (BF16, 256, PRE_LN | QUICK_GELU, {}, None),
    "fp8_b256_clip": (FP8, 256, PRE_LN | QUICK_GELU, {}, None),
    "fp16_hd80_fixture": (FP16, 0, 0, {}, "hd80"),
    "fp16_b300_streams2": (FP16, 300, 0, {}, "streams2"),
    "fp16_b4_graph": (FP16, 4, 0, {}, "graph"),
    "fp16_b256_gemm_pp_5": (FP16, 256, 0, {"VH_GEMM_PP": "5"}, None),
    "fp16_b256_gemm_pp_7": (FP16, 256, 0, {"VH_GEMM_PP": "7"}, None),
    # one context per model family (LN_FOLD_ON: the guard cannot change the path)
    "fp16_b256_swiglu": (FP16, 256, LN_FOLD_ON | SWIGLU, {}, None),
    "fp16_b256_rope": (FP16, 256, LN_FOLD_ON | ROPE, {}, None),
    "fp16_b256_registers_4": (FP16, 256, LN_FOLD_ON | REGISTERS_4, {}, None),
    "fp16_b256_no_cls_avg_norm": (FP16, 256, LN_FOLD_ON | NO_CLS | POOL_AVG_NORM, {}, None),
    "fp16_b256_cls_avg": (FP16, 256, LN_FOLD_ON | POOL_CLS_AVG, {}, None),
    "fp16_b256_map_head": (FP16, 256, LN_FOLD_ON | NO_CLS | MAP_HEAD | TANH_GELU, {}, None),
    "fp16_b256_w8": (FP16, 256, LN_FOLD_ON | W8_E4M3, {}, None),
    "fp16_b32_inflight": (FP16, 32, 0, {}, "inflight"),
    "fp16_b32_readout": (FP16, 32, LN_FOLD_ON, {}, "readout"),
    "fp16_b32_plain_readout": (FP16, 32, LN_FOLD_OFF, {}, "readout"),
    "fp8_b32_readout": (FP8, 32, LN_FOLD_ON, {}, "readout"),
}
VIT_BASE = dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=1000)
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


READOUT_LAYERS = [6, 12]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def read_outs(ctx, batch, cfg):
    """What the read-outs of the last forward return, hashed: the two debug taps, cls / patch / mean of the listed layers (fp32,
    raw and normalised) and their class-token attention."""
    tokens, dim = ctx.features_dims()[1], cfg["dim"]
    out = [f"tap0 {sha(ctx.debug_read(0, batch * tokens * dim))}", f"tap1 {sha(ctx.debug_read(1, batch * dim))}"]
    for k in READOUT_LAYERS:
        for label, norm in (("raw", FEAT_RAW), ("norm", FEAT_NORM)):
            f = ctx.read_layer_features(k, cls=True, patch=True, mean=True, norm=norm)
            out += [f"layer{k}.{label}.{key} {sha(f[key])}" for key in ("cls", "patch", "mean")]
        out.append(f"attention{k} {sha(ctx.read_attention(k)['probs'])}")
    return out


def run_context(tree, name):
    sys.path.insert(0, os.path.join(tree, "vit-fpga_amd", "python"))
    import vithip

    dtype, batch, flags, _, extra = CONTEXTS[name]
    cfg = VIT_BASE
    if extra == "hd80":
        g = np.load(sorted(glob.glob(os.path.join(tree, "tests", "golden", "headdim", "hd80*.npz")))[0])
        cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
        batch = int(g["meta"][2])
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch, device=0, flags=flags)
    ctx.init_weights_seeded(0)
    x = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    y = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, x.ptr)
    if extra == "streams2":
        ctx.set_streams(2)
    if extra == "graph":
        ctx.set_graph(True)
    if extra == "readout":
        ctx.set_feature_layers(READOUT_LAYERS)
        ctx.set_attention_layers(READOUT_LAYERS)
    shas = []
    for _ in range(3 if extra == "graph" else 1):
        if extra == "inflight":
            ctx.forward_device_async(x.ptr, batch, y.ptr, steps=4)
            ctx.synchronize()
        else:
            ctx.forward_device(x.ptr, batch, y.ptr)
        shas.append(sha(y.to_numpy(np.float32, (batch, cfg["classes"]))))
    taps = [int(ctx.debug_read(t, 1)[0]) for t in (3, 4)]
    more = "".join(" " + t for t in read_outs(ctx, batch, cfg)) if extra == "readout" else ""
    prof = ctx.profile_forward(x.ptr, batch, y.ptr)
    slots = " ".join(f"{i}:{prof[s][1]}" for i, s in enumerate(vithip.STAGES) if prof[s][1] or prof[s][0])
    print(f"{name}: batch {batch} logits {' '.join(shas)} taps(3,4) {taps} profile slots(index:events) {slots}{more}", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="checkout to import vithip from (vit-fpga_amd/python, built library beside it)")
    ap.add_argument("--context", help="run this one context in this process")
    a = ap.parse_args()
    if a.context:
        run_context(os.path.abspath(a.tree), a.context)
        return 0
    for name, (_, _, _, env, _) in CONTEXTS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", a.tree, "--context", name], env={**os.environ, **env}, timeout=120)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping here", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
