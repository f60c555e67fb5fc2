#!/usr/bin/env python3
"""Patch-14 measurements (run on the GPU box): models whose patch vector 14*14*3 = 588 is zero-padded to 640 for the patch GEMM.

  python tools/patch14_bench.py [--out profiles] [--steps 20]

  (1) whole forward, ViT-L/14-224 at batch 256 (bf16, fp16, fp8), DINOv2-S/14-518 shape at batch 64 (bf16, fp16) and, as the
      reference point of the same run, ViT-L/16-384 fp16 at batch 256: forward_device_async with step timing (device time per
      step), images/s, algorithmic FLOP/s over the 2.5 PF 16-bit peak;
  (2) the im2col and patch_gemm stages of the same forwards (hip events around their launches): device time, their share
      of the step, and im2col's bytes (fp32 images read + 16-bit padded patch matrix written) over its time against the
      ~6.3 TB/s achievable HBM rate.
The patch-14 models are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

PEAK_16 = 2.5e15   # MI355X dense 16-bit MFMA peak, FLOP/s
HBM = 6.3e12       # achievable HBM rate, bytes/s (MI355X_MICROARCH.md)
DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16, "fp8": vithip.DTYPE_FP8}


def _cfg(image, patch, dim, heads, mlp, layers):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=1000)


RUNS = [  # (model, config, batch, dtypes)
    ("ViT-L/14-224", _cfg(224, 14, 1024, 16, 4096, 24), 256, ("bf16", "fp16", "fp8")),
    ("DINOv2-S/14-518", _cfg(518, 14, 384, 6, 1536, 12), 64, ("bf16", "fp16")),
    ("ViT-L/16-384", _cfg(384, 16, 1024, 16, 4096, 24), 256, ("fp16",)),
]


def stage_ms(ctx, name, din, batch, dout, steps):
    ctx.set_stage_timing(name)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=steps)
    ctx.synchronize()
    avg_ms, min_ms, n = ctx.get_stage_timing()
    ctx.set_stage_timing(None)
    return avg_ms, min_ms, n


def forward_row(model, cfg, batch, dname, steps, log):
    T, P, C = S.tokens(cfg), cfg["patch_size"], cfg["channels"]
    kp = P * P * C
    kpa = -(-kp // 64) * 64
    ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch)
    ctx.init_weights_seeded(0)
    din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * C * 4)
    dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, din.ptr)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=3)   # warm-up
    ctx.synchronize()
    ctx.set_step_timing(True)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=steps)
    ctx.synchronize()
    st = np.array(ctx.get_step_timing())
    ctx.set_step_timing(False)
    im_avg, im_min, im_n = stage_ms(ctx, "im2col", din, batch, dout, max(2, steps // 4))
    pg_avg, pg_min, pg_n = stage_ms(ctx, "patch_gemm", din, batch, dout, max(2, steps // 4))
    logits = dout.to_numpy(np.float32, (batch, cfg["classes"]))
    ctx.close(); din.free(); dout.free()
    step = float(np.median(st))
    flop = S.flops_per_image(cfg) * batch
    im_bytes = batch * cfg["image_size"] ** 2 * C * 4 + batch * (T - 1) * kpa * 2
    r = dict(model=model, tokens=T, patch_vector=kp, patch_vector_padded=kpa, dtype=dname, batch=batch, steps=len(st),
             step_ms_median=step, step_ms_min=float(st.min()), images_per_s=batch / (step * 1e-3),
             gflop_per_image=S.flops_per_image(cfg) / 1e9, flops_per_s=flop / (step * 1e-3),
             peak_fraction=flop / (step * 1e-3) / PEAK_16,
             im2col_us_avg=im_avg * 1e3, im2col_us_min=im_min * 1e3, im2col_launches=im_n, im2col_bytes=im_bytes,
             im2col_bytes_per_s=im_bytes / (im_avg * 1e-3) if im_avg > 0 else None,
             patch_gemm_us_avg=pg_avg * 1e3, patch_gemm_us_min=pg_min * 1e3, patch_gemm_launches=pg_n,
             patch_share_of_step=(im_avg + pg_avg) / step, logits_finite=bool(np.isfinite(logits).all()))
    log(f"forward {model} T={T} {dname} b{batch}: step {step:.3f} ms median ({r['step_ms_min']:.3f} min, {len(st)} steps) = "
        f"{r['images_per_s']:.0f} images/s = {r['flops_per_s'] / 1e15:.3f} PF/s = {r['peak_fraction']:.3f} of {PEAK_16 / 1e15:.1f} PF "
        f"({r['gflop_per_image']:.1f} GFLOP/image)")
    bw = f"{r['im2col_bytes_per_s'] / 1e12:.2f} TB/s = {r['im2col_bytes_per_s'] / HBM:.2f} of {HBM / 1e12:.1f} TB/s" \
        if r["im2col_bytes_per_s"] else "not timed"
    log(f"  stages: im2col {r['im2col_us_avg']:.1f} us avg ({im_n} launches; {im_bytes / 1e6:.1f} MB read + written: {bw}), "
        f"patch_gemm {r['patch_gemm_us_avg']:.1f} us avg ({pg_n} launches, K = {kpa}); together {100 * r['patch_share_of_step']:.2f} % "
        f"of the step")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="patch14")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def log(msg):
        print(msg, flush=True)
        lines.append(msg)

    rows = [forward_row(model, cfg, batch, dname, a.steps, log) for model, cfg, batch, dts in RUNS for dname in dts]
    l14 = next(r for r in rows if r["model"] == "ViT-L/14-224" and r["dtype"] == "fp16")
    l16 = next(r for r in rows if r["model"] == "ViT-L/16-384" and r["dtype"] == "fp16")
    summary = dict(l14_over_l16_flops_fp16=l14["flops_per_s"] / l16["flops_per_s"],
                   l14_patch_share_max=max(r["patch_share_of_step"] for r in rows if r["model"] == "ViT-L/14-224"))
    log(f"ViT-L/14-224 fp16 FLOP/s over ViT-L/16-384 fp16 FLOP/s (same run): {summary['l14_over_l16_flops_fp16']:.3f}; "
        f"im2col + patch_gemm of the ViT-L/14-224 step, worst dtype: {100 * summary['l14_patch_share_max']:.2f} %")
    with open(os.path.join(a.out, f"{a.tag}_bench.json"), "w") as f:
        json.dump(dict(forward=rows, summary=summary), f, indent=1)
    with open(os.path.join(a.out, f"{a.tag}_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
