#!/usr/bin/env python3
"""Attention-rollout measurements (run on the GPU box): what chaining every layer costs beside the forward.

  python tools/rollout_bench.py [--out profiles] [--passes 7]

In ONE process, one context per model, seeded weights and images: ViT-B/16 bf16 at batch 512, ViT-L/14 fp16 at batch 256.  `passes`
interleaved passes, the median reported with min and max, of
  step       one synchronous forward (device buffers) with no rollout set, wall time;
  step+roll  the same with vh_set_rollout(1, -1, mean): one launch per layer more.  The set call is outside the timed region;
  launch     one synchronous vh_op_rollout on q|k|v of the model's shape (random values, scores of deviation 3) with an R_prev: the
             kernel alone, beside its multiply-add count (2 H hd + T) T^2 per image (scores twice, then the fp32 product).
No threshold is asserted: the tool records what it sees.  Not here: the FLOP floor at the fc2 GEMM's rate; the default bench line
against a build of the parent commit is profiles/rollout_default_ab.txt.  Written to <out>/rollout_bench.txt.
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
MODELS = [("ViT-B/16 bf16", S.CONFIGS["vit_base"], vithip.DTYPE_BF16, 512), ("ViT-L/14 fp16", VIT_L14, vithip.DTYPE_FP16, 256)]


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return f"{statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("rollout_bench: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"attention rollout, {a.passes} interleaved passes, median [min .. max] in ms")
    for name, cfg, dt, batch in MODELS:
        T, H, hd, L = S.tokens(cfg), cfg["heads"], cfg["dim"] // cfg["heads"], cfg["layers"]
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
        ctx.init_weights_seeded(0)
        d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
        d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        ctx.fill_input_seeded(1, batch, d_in.ptr)
        rng = np.random.default_rng(0)
        qkv = rng.standard_normal((batch * T, 3 * cfg["dim"])).astype(np.float32)
        qkv[:, :cfg["dim"]] *= np.float32(3.0 / np.sqrt(hd))
        d_qkv = vithip.DeviceBuffer.from_numpy(vithip.to16(qkv, dt))
        d_r = [vithip.DeviceBuffer.from_numpy(np.full((batch, T, T), 1.0 / T, dtype=np.float32)), vithip.DeviceBuffer(batch * T * T * 4)]
        step, roll, launch = [], [], []
        forward = lambda: ctx.forward_device(d_in.ptr, batch, d_out.ptr)
        for p in range(a.passes + 1):   # pass 0 warms up and is dropped
            ctx.set_rollout(0)
            forward()
            t_step = wall_ms(forward)
            ctx.set_rollout(1, -1, vithip.ROLLOUT_MEAN)
            forward()
            t_roll = wall_ms(forward)
            t_launch = wall_ms(lambda: vithip.op_rollout(d_qkv.ptr, batch, T, H, hd, dt, vithip.ROLLOUT_MEAN, d_r[0].ptr, d_r[1].ptr))
            if p:
                step.append(t_step); roll.append(t_roll); launch.append(t_launch)
        macs = (2.0 * H * hd + T) * T * T * batch
        ms, mr, ml = (statistics.median(v) for v in (step, roll, launch))
        say(f"{name} b{batch}, {T} tokens, {L} layers chained:")
        say(f"  step       {med(step)}")
        say(f"  step+roll  {med(roll)}   (+{100 * (mr / ms - 1):.1f} %, {1e3 * (mr - ms) / L:.0f} us per layer)")
        say(f"  launch     {med(launch)}   ({macs / 1e9:.1f} G multiply-adds: {2 * macs / ml / 1e9:.1f} TFLOP/s)")
        for b in (d_in, d_out, d_qkv, *d_r):
            b.free()
        ctx.close()
    with open(os.path.join(a.out, "rollout_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
