#!/usr/bin/env python3
"""Fingerprint of the forward's launch sequence, for A/B runs of two builds that must compute the same thing the same way.

    tools/forward_fingerprint.py --tree <checkout with a built vit-fpga_amd/libvithip.so> [--context NAME]

For every context below -- the smallest at which each branch of enqueue_forward is taken -- it prints one line: the SHA-256 of the
logits of a seeded batch (init_weights_seeded(0), fill_input_seeded(1, ...)), debug taps 3 and 4 (tiled hidden activation,
head-major q|k|v) and the stages of profile_forward that recorded events, with their counts.  Two builds agree
when the two outputs are the same text.  Every context runs in a child process of its own (VH_GEMM_PP and the other knobs are read
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
LN_FOLD_OFF, CLS_TAIL, PRE_LN, QUICK_GELU = 1, 8, 16, 32

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
}
VIT_BASE = dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=1000)
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


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
    shas = []
    for _ in range(3 if extra == "graph" else 1):
        ctx.forward_device(x.ptr, batch, y.ptr)
        shas.append(hashlib.sha256(y.to_numpy(np.float32, (batch, cfg["classes"])).tobytes()).hexdigest())
    taps = [int(ctx.debug_read(t, 1)[0]) for t in (3, 4)]
    prof = ctx.profile_forward(x.ptr, batch, y.ptr)
    slots = " ".join(f"{i}:{prof[s][1]}" for i, s in enumerate(vithip.STAGES) if prof[s][1] or prof[s][0])
    print(f"{name}: batch {batch} logits {' '.join(shas)} taps(3,4) {taps} profile slots(index:events) {slots}", flush=True)
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
