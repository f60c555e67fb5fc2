#!/usr/bin/env python3
"""Head-dim measurements (run on the GPU box): models whose head dim is not 64 run their attention in kernels_attn_hd.hip.

  python tools/headdim_bench.py [--out profiles] [--steps 20] [--skip-forward]

  (1) whole forward, ViT-H/14-224 (head dim 80) at batch 128 in bf16, fp16 and fp8 and, as the head-dim-64 reference point of
      the same run, ViT-L/14-224 fp16 at batch 128: forward_device_async with step timing (device time per step), images/s,
      algorithmic FLOP/s over the 2.5 PF 16-bit peak;
  (2) the attention stage of the same forwards (hip events around its launches): device time per step, its FLOP/s (QK^T + PV,
      4 T^2 D per image and layer) and its share of the step;
  (3) the attention kernel alone at T = 257 and 1025: vh_op_attention_hd at head dims 64, 80 and 128 at equal
      batch x heads x T, bf16, in attention FLOP/s and relative to head dim 64 (host wall clock around `reps` back-to-back
      calls; each call ends with a stream synchronisation, whose few microseconds are included).
The ViT-H/14 and ViT-L/14 models are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

PEAK_16 = 2.5e15   # MI355X dense 16-bit MFMA peak, FLOP/s
DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16, "fp8": vithip.DTYPE_FP8}


def _cfg(image, patch, dim, heads, mlp, layers):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=1000)


RUNS = [  # (model, config, batch, dtypes)
    ("ViT-H/14-224", _cfg(224, 14, 1280, 16, 5120, 32), 128, ("bf16", "fp16", "fp8")),
    ("ViT-L/14-224", _cfg(224, 14, 1024, 16, 4096, 24), 128, ("fp16",)),
]
# (tokens, batch x heads): equal for every head dim at one T
TAP = [(257, 8192), (1025, 1024)]


def stage_ms(ctx, name, din, batch, dout, steps):
    ctx.set_stage_timing(name)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=steps)
    ctx.synchronize()
    avg_ms, min_ms, n = ctx.get_stage_timing()
    ctx.set_stage_timing(None)
    return avg_ms, min_ms, n


def forward_row(model, cfg, batch, dname, steps, log):
    T, D, L = S.tokens(cfg), cfg["dim"], cfg["layers"]
    ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch)
    ctx.init_weights_seeded(0)
    din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, din.ptr)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=3)   # warm-up
    ctx.synchronize()
    ctx.set_step_timing(True)
    ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=steps)
    ctx.synchronize()
    st = np.array(ctx.get_step_timing())
    ctx.set_step_timing(False)
    at_avg, at_min, at_n = stage_ms(ctx, "attention", din, batch, dout, max(2, steps // 4))
    logits = dout.to_numpy(np.float32, (batch, cfg["classes"]))
    ctx.close(); din.free(); dout.free()
    step = float(np.median(st))
    flop = S.flops_per_image(cfg) * batch
    att_step_ms = at_avg * L                      # one launch per layer
    att_flop = 4.0 * T * T * D * L * batch        # QK^T + PV
    r = dict(model=model, tokens=T, head_dim=D // cfg["heads"], dtype=dname, batch=batch, steps=len(st),
             step_ms_median=step, step_ms_min=float(st.min()), images_per_s=batch / (step * 1e-3),
             gflop_per_image=S.flops_per_image(cfg) / 1e9, flops_per_s=flop / (step * 1e-3),
             peak_fraction=flop / (step * 1e-3) / PEAK_16,
             attention_us_per_launch_avg=at_avg * 1e3, attention_us_per_launch_min=at_min * 1e3, attention_launches=at_n,
             attention_ms_per_step=att_step_ms, attention_flops_per_s=att_flop / (att_step_ms * 1e-3),
             attention_peak_fraction=att_flop / (att_step_ms * 1e-3) / PEAK_16, attention_share_of_step=att_step_ms / step,
             logits_finite=bool(np.isfinite(logits).all()))
    log(f"forward {model} T={T} hd={r['head_dim']} {dname} b{batch}: step {step:.3f} ms median ({r['step_ms_min']:.3f} min, "
        f"{len(st)} steps) = {r['images_per_s']:.0f} images/s = {r['flops_per_s'] / 1e15:.3f} PF/s = {r['peak_fraction']:.3f} of "
        f"{PEAK_16 / 1e15:.1f} PF ({r['gflop_per_image']:.1f} GFLOP/image)")
    log(f"  attention: {at_avg * 1e3:.1f} us per launch ({at_n} launches), {att_step_ms:.3f} ms per step = "
        f"{100 * r['attention_share_of_step']:.1f} % of the step, {r['attention_flops_per_s'] / 1e15:.3f} PF/s = "
        f"{r['attention_peak_fraction']:.3f} of peak")
    return r


def tap_rows(log, reps=10):
    rows = []
    for T, bh in TAP:
        for hd in (64, 80, 128):
            heads = 16
            batch = bh // heads
            D = heads * hd
            n = batch * T * 3 * D
            f32 = vithip.DeviceBuffer(n * 4)
            vithip.op_fill(f32.ptr, n, 7, 1, 0)   # uniform [-1, 1): scores stay small without a q scale
            qkv = vithip.DeviceBuffer(n * 2)
            vithip.op_cast(f32.ptr, qkv.ptr, n, vithip.DTYPE_BF16)
            f32.free()
            out = vithip.DeviceBuffer(batch * T * D * 2)
            call = lambda: vithip.op_attention_hd(qkv.ptr, batch, T, heads, hd, out.ptr, vithip.DTYPE_BF16)
            call()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            us = (time.perf_counter() - t0) * 1e6 / reps
            flop = 4.0 * T * T * hd * bh
            got = vithip.from16(out.to_numpy(np.uint16, (batch * T, D))[:64], vithip.DTYPE_BF16)
            r = dict(kernel="hd", tokens=T, head_dim=hd, batch_heads=bh, us_per_call=us, flops_per_s=flop / (us * 1e-6),
                     finite=bool(np.isfinite(got).all()))
            rows.append(r)
            log(f"tap T={T} batch*heads={bh} hd={hd}: {us:.1f} us per call = {r['flops_per_s'] / 1e15:.3f} PF/s")
            qkv.free(); out.free()
    for T, _ in TAP:
        ref = next(r for r in rows if r["tokens"] == T and r["head_dim"] == 64)
        for r in rows:
            if r["tokens"] == T:
                r["over_hd64"] = r["flops_per_s"] / ref["flops_per_s"]
        log(f"tap T={T}: FLOP/s over head dim 64: " +
            ", ".join(f"hd{r['head_dim']} {r['over_hd64']:.3f}" for r in rows if r["tokens"] == T and r["head_dim"] != 64))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="headdim")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-forward", action="store_true", help="tap rows only")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def log(msg):
        print(msg, flush=True)
        lines.append(msg)

    rows = [] if a.skip_forward else [forward_row(model, cfg, batch, dname, a.steps, log) for model, cfg, batch, dts in RUNS for dname in dts]
    taps = tap_rows(log)
    summary = dict(tap_over_hd64={f"T{r['tokens']}_hd{r['head_dim']}": r["over_hd64"] for r in taps})
    if rows:
        h = next(r for r in rows if r["model"] == "ViT-H/14-224" and r["dtype"] == "fp16")
        l14 = next(r for r in rows if r["model"] == "ViT-L/14-224" and r["dtype"] == "fp16")
        summary.update(h14_over_l14_flops_fp16=h["flops_per_s"] / l14["flops_per_s"],
                       h14_over_l14_attention_flops_fp16=h["attention_flops_per_s"] / l14["attention_flops_per_s"])
        log(f"ViT-H/14-224 fp16 FLOP/s over ViT-L/14-224 fp16 FLOP/s (same run): {summary['h14_over_l14_flops_fp16']:.3f} "
            f"(target >= 0.95); attention stage: {summary['h14_over_l14_attention_flops_fp16']:.3f}")
    with open(os.path.join(a.out, f"{a.tag}_bench.json"), "w") as f:
        json.dump(dict(forward=rows, tap=taps, summary=summary), f, indent=1)
    with open(os.path.join(a.out, f"{a.tag}_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
