#!/usr/bin/env python3
"""Pooled-head measurements (run on the GPU box): the one-pass pool kernel against the two-kernel mean it replaces inside the
forward, and what each VH_FLAG_POOL mode and VH_FLAG_NO_CLS cost per step.

  python tools/pool_bench.py [--out profiles] [--passes 7] [--steps 4] [--only NAME]

In ONE process, at the shapes of profiles/features.txt (ViT-B/16 bf16 at batch 512, ViT-L/14 fp16 at batch 256), `passes` interleaved
passes, medians with min and max:
  1. the kernel: wall time of the synchronous vh_op_pool_rows (VH_FEAT_NORM) on synthetic split planes [batch * T][D], beside
     vh_op_token_features2 writing the same normalised mean from the same planes (feat_rows_kernel for the statistics +
     feat_mean_kernel: the planes twice; that tap also allocates and frees its statistics scratch inside the call), and beside the
     synchronous vh_read_features_device(mean) of a live VH_POOL_CLS context of the shape (the same two kernels on the context's own
     scratch: no allocation).  The outputs of the first two are compared for bits.
  2. the step: vh_forward_device_async (`steps` steps, wall time per step) of a context per pooling mode and of a NO_CLS context,
     all holding seeded weights, as ratios to the VH_POOL_CLS context of the same model.
No threshold is asserted: the tool records what it sees.  Written to <out>/pool_bench.txt.
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
POOL, NO_CLS = vithip.FLAG_POOL, vithip.FLAG_NO_CLS
MODES = [("POOL_CLS", 0), ("POOL_AVG_NORM", POOL(vithip.POOL_AVG_NORM)), ("POOL_AVG_FCNORM", POOL(vithip.POOL_AVG_FCNORM)),
         ("POOL_CLS_AVG", POOL(vithip.POOL_CLS_AVG)), ("NO_CLS | POOL_AVG_NORM", NO_CLS | POOL(vithip.POOL_AVG_NORM))]


def med(v):
    return f"{statistics.median(v):9.3f} ms median (min {min(v):.3f}, max {max(v):.3f})"


def kernel_alone(name, cfg, dtype, batch, passes, ctx_cls, say):
    T, D = S.tokens(cfg), cfg["dim"]
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((T, D)) + rng.uniform(-0.8, 0.8, (T, 1))).astype(np.float32)   # one image's rows, repeated
    hi = vithip.to16(x, dtype)
    lo = vithip.to_lo8(x - vithip.from16(hi, dtype), dtype)
    d_hi = vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(hi, (batch, T, D))))
    d_lo = vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(lo, (batch, T, D))))
    d_g = vithip.DeviceBuffer.from_numpy((1.0 + 0.05 * rng.standard_normal(D)).astype(np.float32))
    d_b = vithip.DeviceBuffer.from_numpy((0.02 * rng.standard_normal(D)).astype(np.float32))
    d_one, d_two, d_ctx = (vithip.DeviceBuffer(batch * D * 4) for _ in range(3))
    desc = vithip.Features(None, None, d_ctx.ptr, vithip.ELEM_F32, vithip.FEAT_NORM)

    def one():
        vithip.op_pool_rows(d_hi.ptr, d_lo.ptr, dtype, batch, T, 1, D, d_g.ptr, d_b.ptr, 1e-6, vithip.FEAT_NORM, d_one.ptr)

    def two():
        vithip.op_token_features2(d_hi.ptr, d_lo.ptr, dtype, batch, T, 1, D, d_g.ptr, d_b.ptr, 1e-6, vithip.ELEM_F32, vithip.FEAT_NORM, None,
                                  vithip.FEAT_ROWS, d_two.ptr, None)

    def live():
        ctx_cls.read_features_device(desc)

    runs = [("one pass   (vh_op_pool_rows)", one), ("two kernels (vh_op_token_features2)", two), ("two kernels (live context, read mean)", live)]
    for _, fn in runs:
        fn()
        fn()
    same = np.array_equal(d_one.to_numpy(np.uint32, (batch, D)), d_two.to_numpy(np.uint32, (batch, D)))
    ms = {k: [] for k, _ in runs}
    for _ in range(passes):
        for k, fn in runs:
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    planes = batch * (T - 1) * D * 3
    say(f"{name}: pool kernel alone, T = {T}, D = {D}, split planes (3 B / element), {planes / 1e6:.1f} MB of patch rows; {passes} interleaved passes")
    for k, _ in runs:
        m = statistics.median(ms[k])
        nb = planes * (1 if k.startswith("one") else 2)
        say(f"  {k:<40} {med(ms[k])}  {nb / 1e6:7.1f} MB  {nb / m / 1e6:7.1f} GB/s")
    a, b, c = (statistics.median(ms[k]) for k, _ in runs)
    say(f"  one pass / two kernels = {a / b:.3f} (tap against tap), {a / c:.3f} (tap against the live context's read); "
        f"the two taps' outputs are {'bit-identical' if same else 'DIFFERENT'}")
    for buf in (d_hi, d_lo, d_g, d_b, d_one, d_two, d_ctx):
        buf.free()


def measure(name, cfg, dtype, batch, passes, steps, say):
    ctxs = []
    for label, flags in MODES:
        ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch, flags=flags)
        ctx.init_weights_seeded(0)
        ctxs.append((label, ctx))
    d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctxs[0][1].fill_input_seeded(1, batch, d_in.ptr)
    for _, ctx in ctxs:   # warm-up
        ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=2)
        ctx.synchronize()
    kernel_alone(name, cfg, dtype, batch, passes, ctxs[0][1], say)
    step_ms = {label: [] for label, _ in ctxs}
    for _ in range(passes):
        for label, ctx in ctxs:
            t0 = time.perf_counter()
            ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=steps)
            ctx.synchronize()
            step_ms[label].append((time.perf_counter() - t0) * 1e3 / steps)
    base = statistics.median(step_ms["POOL_CLS"])
    say(f"{name}: step time per mode, fold {ctxs[0][1].ln_fold()}; {passes} interleaved passes, {steps} steps per pass")
    for label, _ in ctxs:
        m = statistics.median(step_ms[label])
        say(f"  {label:<24} {med(step_ms[label])}  {m / base:.4f} of POOL_CLS ({100 * (m / base - 1):+.2f} %)")
    for _, ctx in ctxs:
        ctx.close()
    d_in.free()
    d_out.free()


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

    say("pooled heads: the one-pass pool kernel against the two-kernel mean, and the forward's step time per pooling mode, same process")
    for name, cfg, dtype, batch in MODELS:
        if not a.only or a.only in name:
            measure(name, cfg, dtype, batch, a.passes, a.steps, say)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "pool_bench.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
