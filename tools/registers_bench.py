#!/usr/bin/env python3
"""Register-token measurements (run on the GPU box): what R = 4 register tokens cost against the same model with R = 0.

  python tools/registers_bench.py [--out profiles] [--steps 20] [--passes 3]

ViT-B/14 and ViT-L/14 at 224 x 224 (257 -> 261 tokens, batch 256) and DINOv2-S/14 at 518 x 518 (1 370 -> 1 374 tokens, batch 64) in
bf16, fp16 and fp8, in ONE process and interleaved (A, B, A, B, ... per shape and dtype, so that both see the same box and clock):
  (1) whole forward with R = 4 and with R = 0: forward_device_async with step timing; median and min step, images/s, the ratio
      of the medians beside the row ratio T(4) / T(0) that arithmetic predicts, and the 256-row tile rounds of both;
  (2) the lead-row kernel (stage "cls_rows": the class-token row and the R register rows of every image), hip events per launch;
  (3) the layer stages of both (q|k|v, attention, out-projection, fc1, fc2; hip events around their launches), per launch: where a
      step ratio away from the row ratio comes from.
Writes registers_bench.txt and registers_bench.json.  The towers are defined here: vh_synth.CONFIGS is shared by the test suite
and bench.py.
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
REGS = 4
LAYER_STAGES = ["qkv_gemm", "attention", "proj_gemm", "fc1_gemm", "fc2_gemm"]


def _cfg(image, dim, heads, mlp, layers):
    return dict(image_size=image, patch_size=14, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=1000)


RUNS = [("ViT-B/14-224", _cfg(224, 768, 12, 3072, 12), 256), ("ViT-L/14-224", _cfg(224, 1024, 16, 4096, 24), 256),
        ("DINOv2-S/14-518", _cfg(518, 384, 6, 1536, 12), 64)]


class Run:
    def __init__(self, cfg, dname, batch, regs):
        self.cfg, self.batch = cfg, batch
        self.ctx = vithip.VitContext(dict(cfg, registers=regs), dtype=DT[dname], max_batch=batch)
        self.ctx.init_weights_seeded(0)
        self.tokens = self.ctx.features_dims()[1]
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
        fold = self.ctx.ln_fold()
        self.ctx.close(); self.din.free(); self.dout.free()
        return finite, fold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp16,fp8")
    ap.add_argument("--models", default=",".join(r[0] for r in RUNS))
    a = ap.parse_args()
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"registers_bench: R = {REGS} against R = 0, {a.steps} timed steps per pass, {a.passes} interleaved passes per context (A B A B ...)")
    for model, cfg, batch in RUNS:
        if model not in a.models.split(","):
            continue
        for dname in a.dtypes.split(","):
            A, B = Run(cfg, dname, batch, REGS), Run(cfg, dname, batch, 0)
            sa, sb = [], []
            for _ in range(a.passes):
                sa.append(A.steps(a.steps)); sb.append(B.steps(a.steps))
            pass_ratio = [float(np.median(x) / np.median(y)) for x, y in zip(sa, sb)]
            sa, sb = np.concatenate(sa), np.concatenate(sb)
            la, lb = A.stage("cls_rows", 8), B.stage("cls_rows", 8)
            st = {name: (A.stage(name, 4)[0] * 1e3, B.stage(name, 4)[0] * 1e3) for name in LAYER_STAGES}
            ta, tb = A.tokens, B.tokens
            tiles = lambda t: -(-batch * t // 256)
            r = dict(model=model, dtype=dname, batch=batch, tokens_reg=ta, tokens_plain=tb, row_ratio=ta / tb,
                     row_tiles_reg=tiles(ta), row_tiles_plain=tiles(tb),
                     reg_step_ms_median=float(np.median(sa)), reg_step_ms_min=float(sa.min()),
                     plain_step_ms_median=float(np.median(sb)), plain_step_ms_min=float(sb.min()),
                     step_ratio=float(np.median(sa) / np.median(sb)), step_ratio_per_pass=pass_ratio,
                     reg_images_per_s=batch / (float(np.median(sa)) * 1e-3), plain_images_per_s=batch / (float(np.median(sb)) * 1e-3),
                     lead_rows_us_avg_reg=la[0] * 1e3, lead_rows_us_min_reg=la[1] * 1e3, lead_rows_us_avg_plain=lb[0] * 1e3,
                     lead_rows_us_min_plain=lb[1] * 1e3, lead_rows_launches=la[2], stage_us_avg_reg_plain=st)
            (fa, fold_a), (fb, fold_b) = A.close(), B.close()
            r["logits_finite"], r["ln_fold"] = fa and fb, [fold_a, fold_b]
            rows.append(r)
            log(f"{model} b{batch} {dname}: R={REGS} T={ta} {r['reg_step_ms_median']:.3f} ms median ({r['reg_step_ms_min']:.3f} min) = "
                f"{r['reg_images_per_s']:.0f} images/s | R=0 T={tb} {r['plain_step_ms_median']:.3f} ms ({r['plain_step_ms_min']:.3f} min) = "
                f"{r['plain_images_per_s']:.0f} images/s | step ratio {r['step_ratio']:.4f} (per pass {' '.join(f'{x:.4f}' for x in pass_ratio)}), "
                f"row ratio {ta / tb:.4f}, 256-row tiles {r['row_tiles_reg']} / {r['row_tiles_plain']} = {r['row_tiles_reg'] / r['row_tiles_plain']:.4f}")
            log(f"    lead-row kernel per launch: R={REGS} {r['lead_rows_us_avg_reg']:.1f} us avg ({r['lead_rows_us_min_reg']:.1f} min) | R=0 "
                f"{r['lead_rows_us_avg_plain']:.1f} us avg ({r['lead_rows_us_min_plain']:.1f} min) | one launch per forward = "
                f"{100 * r['lead_rows_us_avg_reg'] * 1e-3 / r['reg_step_ms_median']:.3f} % of the step | fold {fold_a}/{fold_b}, finite {r['logits_finite']}")
            log("    layer stages, us per launch R=4 / R=0 (ratio): " +
                ", ".join(f"{n} {x:.1f} / {y:.1f} ({x / y:.4f})" for n, (x, y) in st.items()))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "registers_bench.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "registers_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
