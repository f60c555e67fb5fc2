#!/usr/bin/env python3
"""CLIP measurements (run on the GPU box): what the two switches VH_FLAG_PRE_LN and VH_FLAG_QUICK_GELU cost.

  python tools/clip_bench.py [--out profiles] [--steps 20] [--batch 256]

For the CLIP ViT-B/32, ViT-B/16 and ViT-L/14 towers at 224 x 224 in bf16, fp16 and fp8, in ONE process and interleaved
(A, B, A, B per shape and dtype, so that both see the same box and clock):
  (1) whole forward with both flags and with neither: forward_device_async with step timing, median and min step, images/s;
  (2) the fc1 stage of both (hip events around its launches): QuickGELU against erf GELU in the same kernel, per launch;
  (3) the pre_layernorm stage of the flagged context, per launch (one launch per forward).
The towers are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
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

DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16, "fp8": vithip.DTYPE_FP8}
CLIP_FLAGS = vithip.FLAG_PRE_LN | vithip.FLAG_QUICK_GELU


def _cfg(patch, dim, heads, mlp, layers, classes):
    return dict(image_size=224, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


RUNS = [("CLIP ViT-B/32", _cfg(32, 768, 12, 3072, 12, 512)), ("CLIP ViT-B/16", _cfg(16, 768, 12, 3072, 12, 512)),
        ("CLIP ViT-L/14", _cfg(14, 1024, 16, 4096, 24, 768))]


class Run:
    def __init__(self, cfg, dname, batch, flags):
        self.cfg, self.batch = cfg, batch
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=1e-5)
        self.ctx.init_weights_seeded(0)
        self.din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
        self.dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        self.ctx.fill_input_seeded(1, batch, self.din.ptr)
        self.ctx.forward_device_async(self.din.ptr, batch, self.dout.ptr, steps=5)   # warm-up
        self.ctx.synchronize()

    def steps(self, n):
        self.ctx.set_step_timing(True)
        self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps=n)
        self.ctx.synchronize()
        st = np.array(self.ctx.get_step_timing())
        self.ctx.set_step_timing(False)
        return st

    def stage(self, name, n):
        self.ctx.set_stage_timing(name)
        self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps=n)
        self.ctx.synchronize()
        avg_ms, min_ms, launches = self.ctx.get_stage_timing()
        self.ctx.set_stage_timing(None)
        return avg_ms, min_ms, launches

    def close(self):
        finite = bool(np.isfinite(self.dout.to_numpy(np.float32, (self.batch, self.cfg["classes"]))).all())
        self.ctx.close(); self.din.free(); self.dout.free()
        return finite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,fp16,fp8")
    a = ap.parse_args()
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"clip_bench: batch {a.batch}, {a.steps} timed steps per pass, two interleaved passes per context (A B A B)")
    for model, cfg in RUNS:
        for dname in a.dtypes.split(","):
            A, B = Run(cfg, dname, a.batch, CLIP_FLAGS), Run(cfg, dname, a.batch, 0)
            sa, sb = [], []
            for _ in range(2):
                sa.append(A.steps(a.steps)); sb.append(B.steps(a.steps))
            sa, sb = np.concatenate(sa), np.concatenate(sb)
            fa, fb = A.stage("fc1_gemm", 4), B.stage("fc1_gemm", 4)
            fa2, fb2 = A.stage("fc1_gemm", 4), B.stage("fc1_gemm", 4)
            pl = A.stage("pre_layernorm", 8)
            r = dict(model=model, tokens=S.tokens(cfg), dtype=dname, batch=a.batch,
                     clip_step_ms_median=float(np.median(sa)), clip_step_ms_min=float(sa.min()),
                     plain_step_ms_median=float(np.median(sb)), plain_step_ms_min=float(sb.min()),
                     clip_images_per_s=a.batch / (float(np.median(sa)) * 1e-3), plain_images_per_s=a.batch / (float(np.median(sb)) * 1e-3),
                     fc1_qgelu_us_avg=[fa[0] * 1e3, fa2[0] * 1e3], fc1_gelu_us_avg=[fb[0] * 1e3, fb2[0] * 1e3],
                     fc1_qgelu_us_min=min(fa[1], fa2[1]) * 1e3, fc1_gelu_us_min=min(fb[1], fb2[1]) * 1e3, fc1_launches=fa[2],
                     pre_layernorm_us_avg=pl[0] * 1e3, pre_layernorm_us_min=pl[1] * 1e3, pre_layernorm_launches=pl[2])
            r["logits_finite"] = A.close() and B.close()
            rows.append(r)
            q, g = float(np.mean(r["fc1_qgelu_us_avg"])), float(np.mean(r["fc1_gelu_us_avg"]))
            log(f"{model} T={r['tokens']} {dname}: CLIP flags {r['clip_step_ms_median']:.3f} ms median ({r['clip_step_ms_min']:.3f} min) = "
                f"{r['clip_images_per_s']:.0f} images/s | no flag {r['plain_step_ms_median']:.3f} ms ({r['plain_step_ms_min']:.3f} min) = "
                f"{r['plain_images_per_s']:.0f} images/s | ratio {r['clip_step_ms_median'] / r['plain_step_ms_median']:.4f}")
            log(f"    fc1 per launch: QuickGELU {q:.1f} us avg ({r['fc1_qgelu_us_min']:.1f} min) | erf GELU {g:.1f} us avg "
                f"({r['fc1_gelu_us_min']:.1f} min) | ratio {q / g:.4f} | passes {r['fc1_qgelu_us_avg'][0]:.1f} {r['fc1_qgelu_us_avg'][1]:.1f} / "
                f"{r['fc1_gelu_us_avg'][0]:.1f} {r['fc1_gelu_us_avg'][1]:.1f}")
            log(f"    pre_layernorm: {r['pre_layernorm_us_avg']:.1f} us per launch ({r['pre_layernorm_us_min']:.1f} min, one per forward) = "
                f"{100 * r['pre_layernorm_us_avg'] * 1e-3 / r['clip_step_ms_median']:.2f} % of the step; "
                f"{a.batch * r['tokens'] * cfg['dim'] * 4 / 1e6:.0f} MB read")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "clip_bench.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "clip_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
