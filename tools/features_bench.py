#!/usr/bin/env python3
"""Token-feature measurements (run on the GPU box): what pulling the features of a finished forward costs.

  python tools/features_bench.py [--out profiles] [--passes 7] [--steps 4] [--only NAME]

In ONE process, one context per model: ViT-B/16 bf16 at batch 512 and ViT-L/14 fp16 at batch 256.  `passes` interleaved passes of
  the forward (vh_forward_device_async, `steps` steps, wall time per step), then the synchronous vh_read_features_device of
  patch as fp32, patch as bf16, mean only, cls only (all VH_FEAT_NORM), wall time of each call,
the median pass reported with min and max, beside the bytes each call must move (planes in, results out; the mean re-reads the
planes) and the GB/s that implies.  Then, on the small fp16 model of the feature tests, the parity of the normalised features with
the CPU oracle beside the parity of the hidden state they are made from.  No threshold is asserted: the tool records what it sees.
Written to <out>/features.txt.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

VIT_L14 = dict(image_size=224, patch_size=14, channels=3, dim=1024, heads=16, mlp_dim=4096, layers=24, classes=1000)
MODELS = [("ViT-B/16 bf16 b512", S.CONFIGS["vit_base"], vithip.DTYPE_BF16, 512),
          ("ViT-L/14 fp16 b256", VIT_L14, vithip.DTYPE_FP16, 256)]
VARIANTS = ["patch fp32", "patch bf16", "mean only", "cls only"]


def call_bytes(variant, B, T, D, plane_bytes):
    """Bytes a call must move: the patch rows' planes in (the mean kernel reads them a second time), results out, the row statistics."""
    NP = T - 1
    planes = B * NP * D * plane_bytes
    if variant == "patch fp32":
        return planes + B * NP * D * 4
    if variant == "patch bf16":
        return planes + B * NP * D * 2
    if variant == "mean only":
        return 2 * planes + 2 * B * NP * 8 + B * D * 4
    return B * D * 4 + B * D * 4


def measure(name, cfg, dtype, batch, passes, steps, say):
    T, D = S.tokens(cfg), cfg["dim"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch)
    ctx.init_weights_seeded(0)
    split = ctx.ln_fold()
    plane_bytes = 3 if split else 4
    d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, d_in.ptr)
    bufs = {"patch": vithip.DeviceBuffer(batch * (T - 1) * D * 4), "cls": vithip.DeviceBuffer(batch * D * 4),
            "mean": vithip.DeviceBuffer(batch * D * 4)}
    descs = {"patch fp32": vithip.Features(None, bufs["patch"].ptr, None, vithip.ELEM_F32, vithip.FEAT_NORM),
             "patch bf16": vithip.Features(None, bufs["patch"].ptr, None, vithip.ELEM_BF16, vithip.FEAT_NORM),
             "mean only": vithip.Features(None, None, bufs["mean"].ptr, vithip.ELEM_F32, vithip.FEAT_NORM),
             "cls only": vithip.Features(bufs["cls"].ptr, None, None, vithip.ELEM_F32, vithip.FEAT_NORM)}
    ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=2)   # warm-up: the forward and every feature kernel once
    ctx.synchronize()
    for v in VARIANTS:
        ctx.read_features_device(descs[v])
    step_ms, feat_ms = [], {v: [] for v in VARIANTS}
    for _ in range(passes):
        t0 = time.perf_counter()
        ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=steps)
        ctx.synchronize()
        step_ms.append((time.perf_counter() - t0) * 1e3 / steps)
        for v in VARIANTS:
            t0 = time.perf_counter()
            ctx.read_features_device(descs[v])
            feat_ms[v].append((time.perf_counter() - t0) * 1e3)
    step = statistics.median(step_ms)
    say(f"{name}: T = {T}, D = {D}, residual rows as {'split planes (3 B / element)' if split else 'fp32'}; {passes} interleaved passes")
    say(f"  forward step            {step:9.3f} ms median (min {min(step_ms):.3f}, max {max(step_ms):.3f}; {steps} steps per pass)")
    for v in VARIANTS:
        ms = statistics.median(feat_ms[v])
        nb = call_bytes(v, batch, T, D, plane_bytes)
        say(f"  read {v:<12}       {ms:9.3f} ms median (min {min(feat_ms[v]):.3f}, max {max(feat_ms[v]):.3f})  "
            f"{nb / 1e6:8.1f} MB  {nb / ms / 1e6:7.1f} GB/s  {100 * ms / step:5.2f} % of a step")
    ctx.close()
    for b in (d_in, d_out, *bufs.values()):
        b.free()


def oracle_parity(say):
    import features_ref as R
    import oracle_lib as O
    cfg, seed, eps = R.FEAT_FOLD, 11, 1e-6
    blob, images = S.make_blob(cfg, seed, eps), S.make_images(cfg, 8, 3)
    t = S.make_tensors(cfg, seed)
    T, D = S.tokens(cfg), cfg["dim"]
    _, hidden = O.vit_forward(cfg, blob, images, want_hidden=True, ln_eps=eps)
    hidden = hidden.reshape(3, T, D)
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_FP16, max_batch=3, ln_eps=eps)
    ctx.load_weights(blob)
    ctx.forward(images)
    x = ctx.debug_read(0, 3 * T * D).reshape(3, T, D)
    f = ctx.read_features(cls=True, patch=True, mean=True)
    ctx.close()
    ref = R.layernorm64(hidden, t["lnf.weight"], t["lnf.bias"], eps)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())   # noqa: E731
    say(f"feat_fold (96 / 16, D 256, 2 layers) fp16 b3 against the CPU oracle, rel = max|d| / max|ref|: hidden state {rel(x, hidden):.3e}; "
        f"normalised patch rows {rel(f['patch'], ref[:, 1:, :]):.3e}, cls {rel(f['cls'], ref[:, 0, :]):.3e}, "
        f"mean {rel(f['mean'], ref[:, 1:, :].mean(axis=1)):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("token features: wall time of the synchronous vh_read_features_device beside the forward's step time, same process")
    for name, cfg, dtype, batch in MODELS:
        if not a.only or a.only in name:
            measure(name, cfg, dtype, batch, a.passes, a.steps, say)
    oracle_parity(say)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "features.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
