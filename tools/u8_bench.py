#!/usr/bin/env python3
"""8-bit input measurements (run on the GPU box): what taking u8 NHWC images instead of fp32 is worth on the host path.

  python tools/u8_bench.py [--out profiles] [--steps 30] [--passes 3] [--only NAME]

In ONE process, for ViT-B/16 bf16 at batch 512, ViT-B/16 fp8 at batch 512 and CLIP ViT-B/32 bf16 at batch 256:
  (1) images/s through the submit/collect ring (3 slots, pinned host memory -> logits in host memory) with fp32 slots and
      with u8 slots, and the HBM-resident rate (forward_device_async / forward_device_u8_async on the same buffers, step
      timing, median step) -- the four modes interleaved, `passes` times, the median pass reported with min and max;
  (2) the im2col stage of both kinds, hip events around its launches (vh_set_stage_timing), two interleaved passes.
The two kinds see the same images: the fp32 arrays are the u8 images normalised on the host (ImageNet mean / std), so
both rings compute the same logits, which is checked.  Written to <out>/u8_host_path.txt and .json.
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

DT = {"bf16": vithip.DTYPE_BF16, "fp8": vithip.DTYPE_FP8}
CLIP_B32 = dict(image_size=224, patch_size=32, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=512)
RUNS = [("ViT-B/16 bf16 b512", "vit_b16_bf16", S.CONFIGS["vit_base"], "bf16", 512, 0, 1e-6),
        ("ViT-B/16 fp8 b512", "vit_b16_fp8", S.CONFIGS["vit_base"], "fp8", 512, 0, 1e-6),
        ("CLIP ViT-B/32 bf16 b256", "clip_b32_bf16", CLIP_B32, "bf16", 256, vithip.FLAG_PRE_LN | vithip.FLAG_QUICK_GELU, 1e-5)]
SLOTS = 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Side:
    """One context with one ring (fp32 or u8 slots) and the matching HBM-resident input."""

    def __init__(self, cfg, dname, batch, flags, eps, u8_images, scale, shift, u8):
        self.cfg, self.batch, self.u8 = cfg, batch, u8
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        host = u8_images if u8 else (u8_images.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
        self.din = vithip.DeviceBuffer.from_numpy(host)
        self.dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        self.ctx.ring_create(SLOTS, batch, u8=u8)
        for _ in range(SLOTS):   # fill every slot's pinned staging buffer once (a producer writes there in place); warms up too
            (self.ctx.ring_input_u8 if u8 else self.ctx.ring_input)(batch)[...] = host
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]
        self.fwd(5)
        self.ctx.synchronize()

    def submit(self):
        (self.ctx.ring_submit_u8 if self.u8 else self.ctx.ring_submit)(None, self.batch)

    def fwd(self, steps):
        (self.ctx.forward_device_u8_async if self.u8 else self.ctx.forward_device_async)(self.din.ptr, self.batch, self.dout.ptr, steps)

    def ring_rate(self, steps):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        inflight = 0
        for _ in range(steps):
            if inflight == SLOTS:
                self.ctx.ring_collect(); inflight -= 1
            self.submit(); inflight += 1
        while inflight:
            self.ctx.ring_collect(); inflight -= 1
        return self.batch * steps / (time.perf_counter() - t0)

    def resident_rate(self, steps):
        self.ctx.set_step_timing(True)
        self.fwd(steps)
        self.ctx.synchronize()
        st = np.array(self.ctx.get_step_timing())
        self.ctx.set_step_timing(False)
        return self.batch / (float(np.median(st)) * 1e-3)

    def im2col(self, steps):
        self.ctx.set_stage_timing("im2col")
        self.fwd(steps)
        self.ctx.synchronize()
        avg_ms, min_ms, launches = self.ctx.get_stage_timing()
        self.ctx.set_stage_timing(None)
        return avg_ms * 1e3, min_ms * 1e3, launches

    def close(self):
        self.ctx.close(); self.din.free(); self.dout.free()


def mid(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    log(f"u8_bench: ring of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (fp32 ring, u8 ring, fp32 resident, "
        f"u8 resident); median pass [min .. max]; images/s")
    for title, key, cfg, dname, batch, flags, eps in RUNS:
        if a.only and a.only != key:
            continue
        rng = np.random.default_rng(3)
        u8 = rng.integers(0, 256, size=(batch, cfg["image_size"], cfg["image_size"], cfg["channels"]), dtype=np.uint8)
        F = Side(cfg, dname, batch, flags, eps, u8, scale, shift, u8=False)
        U = Side(cfg, dname, batch, flags, eps, u8, scale, shift, u8=True)
        same = bool(np.array_equal(F.first.view(np.uint32), U.first.view(np.uint32)) and np.isfinite(F.first).all())
        rf, ru, sf, su = [], [], [], []
        for _ in range(a.passes):
            rf.append(F.ring_rate(a.steps)); ru.append(U.ring_rate(a.steps))
            sf.append(F.resident_rate(a.steps)); su.append(U.resident_rate(a.steps))
        i1 = [F.im2col(8), U.im2col(8), F.im2col(8), U.im2col(8)]
        px = batch * cfg["image_size"] ** 2 * cfg["channels"]
        r = dict(config=key, title=title, batch=batch, dtype=dname, ring_logits_bit_identical=same,
                 ring_fp32=mid(rf), ring_u8=mid(ru), resident_fp32=mid(sf), resident_u8=mid(su),
                 h2d_MB_per_step_fp32=px * 4 / 1e6, h2d_MB_per_step_u8=px / 1e6,
                 im2col_fp32_us_avg=[i1[0][0], i1[2][0]], im2col_u8_us_avg=[i1[1][0], i1[3][0]],
                 im2col_fp32_us_min=min(i1[0][1], i1[2][1]), im2col_u8_us_min=min(i1[1][1], i1[3][1]), im2col_launches=i1[0][2])
        rows.append(r)
        res = r["resident_fp32"][0]
        log(f"{title}: logits of both rings bit-identical: {same}")
        for name, k in (("ring, fp32 slots", "ring_fp32"), ("ring, u8 slots  ", "ring_u8"), ("resident, fp32  ", "resident_fp32"),
                        ("resident, u8    ", "resident_u8")):
            m, lo, hi = r[k]
            log(f"    {name}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / res:6.2f} % of the fp32-resident rate")
        log(f"    upload per step: fp32 {r['h2d_MB_per_step_fp32']:.1f} MB = {r['h2d_MB_per_step_fp32'] * 1e-3 * r['ring_fp32'][0] / batch:.1f} GB/s at the ring rate | "
            f"u8 {r['h2d_MB_per_step_u8']:.1f} MB = {r['h2d_MB_per_step_u8'] * 1e-3 * r['ring_u8'][0] / batch:.1f} GB/s")
        f_us, u_us = float(np.mean(r["im2col_fp32_us_avg"])), float(np.mean(r["im2col_u8_us_avg"]))
        log(f"    im2col per launch: fp32 {f_us:.1f} us avg ({r['im2col_fp32_us_min']:.1f} min) | u8 {u_us:.1f} us avg ({r['im2col_u8_us_min']:.1f} min) | "
            f"u8 / fp32 = {u_us / f_us:.3f} | passes {r['im2col_fp32_us_avg'][0]:.1f} {r['im2col_fp32_us_avg'][1]:.1f} / "
            f"{r['im2col_u8_us_avg'][0]:.1f} {r['im2col_u8_us_avg'][1]:.1f}")
        F.close(); U.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "u8_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "u8_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
