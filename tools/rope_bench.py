#!/usr/bin/env python3
"""Rotary-embedding measurements (run on the GPU box): what VH_FLAG_ROPE costs against the same model with the flag cleared.

  python tools/rope_bench.py [--out profiles] [--steps 20] [--passes 3]

DINOv3 ViT-S/16, ViT-B/16 and ViT-L/16 at 224 x 224 with 4 register tokens (201 tokens, batch 256) in bf16, fp16 and fp8, in ONE process
and interleaved (A, B, A, B, ... per model and dtype, so that both see the same box and clock); A = FLAG_ROPE | REGISTERS(4), B =
REGISTERS(4):
  (1) whole forward of both: forward_device_async with step timing; median and min step, images/s, the ratio of the medians (per pass
      too), and the difference per layer -- the rotation IN PLACE, with whatever it does to the attention kernel behind it;
  (2) the rotation launch ON ITS OWN through the tap vh_op_rope on a q|k|v buffer of the model's shape, in both layouts where head dim
      64 has both: host time per synchronous call, minus the same call on ONE image (launch + synchronisation), beside
      bytes / 4.33 TB/s, the rate the feature read-out reaches, with their ratio.  bytes = q and k of the patch rows read and written
      once: batch * 196 * 2 * dim * 2 B * 2.  (fp8 contexts keep q|k|v in bf16: the bf16 figure is theirs.)
  (3) the attention and q|k|v stages of both (hip events around their launches), per launch: whether the pass changes its neighbours.
Neither number is a threshold: they decide whether fusing the rotation into the projection's epilogue is worth its risk.
Writes rope_bench.txt and rope_bench.json.  The towers are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
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

import vithip  # noqa: E402

DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16, "fp8": vithip.DTYPE_FP8}
REGS, BATCH, RATE = 4, 256, 4.33e12
STAGES = ["qkv_gemm", "attention"]


def _cfg(dim, heads, mlp, layers):
    return dict(image_size=224, patch_size=16, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=1000)


RUNS = [("DINOv3-S/16", _cfg(384, 6, 1536, 12)), ("DINOv3-B/16", _cfg(768, 12, 3072, 12)), ("DINOv3-L/16", _cfg(1024, 16, 4096, 24))]


class Run:
    def __init__(self, cfg, dname, batch, flags):
        self.cfg, self.batch = cfg, batch
        self.ctx = vithip.VitContext(dict(cfg, registers=REGS), dtype=DT[dname], max_batch=batch, flags=flags)
        self.ctx.init_weights_seeded(0)
        self.din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
        self.dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        self.ctx.fill_input_seeded(1, batch, self.din.ptr)
        self.ctx.forward_device_async(self.din.ptr, batch, self.dout.ptr, steps=5)   # warm-up
        self.ctx.synchronize()
        self.hm = int(self.ctx.debug_read(4, 1)[0])

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


def tap(cfg, dname, batch, calls):
    """us per synchronous vh_op_rope call on a q|k|v of the model's shape, per layout: (layout, whole batch, one image)."""
    D, H = cfg["dim"], cfg["heads"]
    hd, NP = D // H, (cfg["image_size"] // cfg["patch_size"]) ** 2
    T = NP + 1 + REGS
    rows = batch * T
    hm_rows = -(-rows // 256) * 256
    buf = vithip.DeviceBuffer.from_numpy(np.full(3 * D * hm_rows, 0x3C00, np.uint16))   # a finite value in both 16-bit types
    a = np.linspace(-3.0, 3.0, NP * hd // 2, dtype=np.float64)
    cos, sin = (vithip.DeviceBuffer.from_numpy(f(a).astype(np.float32)) for f in (np.cos, np.sin))
    out = []
    for layout, hm in (("row-major", 0),) + ((("head-major", hm_rows),) if hd == 64 else ()):
        res = []
        for b in (batch, 1):
            t = []
            for i in range(calls + 3):
                t0 = time.perf_counter()
                vithip.op_rope(buf.ptr, DT[dname], b, T, H, hd, 1 + REGS, hm, cos.ptr, sin.ptr)
                t.append((time.perf_counter() - t0) * 1e6)
            res.append((float(np.median(t[3:])), float(np.min(t[3:]))))
        out.append((layout, res[0], res[1]))
    buf.free(); cos.free(); sin.free()
    return out


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

    log(f"rope_bench: FLAG_ROPE against the flag cleared, R = {REGS}, batch {BATCH}, {a.steps} timed steps per pass, {a.passes} interleaved passes per "
        f"context (A B A B ...)")
    for model, cfg in RUNS:
        if model not in a.models.split(","):
            continue
        nbytes = BATCH * (cfg["image_size"] // cfg["patch_size"]) ** 2 * 2 * cfg["dim"] * 2 * 2
        for dname in a.dtypes.split(","):
            A, B = Run(cfg, dname, BATCH, vithip.FLAG_ROPE), Run(cfg, dname, BATCH, 0)
            sa, sb = [], []
            for _ in range(a.passes):
                sa.append(A.steps(a.steps)); sb.append(B.steps(a.steps))
            pass_ratio = [float(np.median(x) / np.median(y)) for x, y in zip(sa, sb)]
            sa, sb = np.concatenate(sa), np.concatenate(sb)
            st = {name: (A.stage(name, 4)[0] * 1e3, B.stage(name, 4)[0] * 1e3) for name in STAGES}
            hm = (A.hm, B.hm)
            (fa, fold_a), (fb, fold_b) = A.close(), B.close()
            ma, mb = float(np.median(sa)), float(np.median(sb))
            per_layer_us = (ma - mb) * 1e3 / cfg["layers"]
            r = dict(model=model, dtype=dname, batch=BATCH, rope_step_ms_median=ma, rope_step_ms_min=float(sa.min()), plain_step_ms_median=mb,
                     plain_step_ms_min=float(sb.min()), step_ratio=ma / mb, step_ratio_per_pass=pass_ratio, rope_images_per_s=BATCH / (ma * 1e-3),
                     plain_images_per_s=BATCH / (mb * 1e-3), in_place_us_per_layer=per_layer_us, bytes_per_layer=nbytes,
                     bytes_over_rate_us=nbytes / RATE * 1e6, stage_us_avg_rope_plain=st, head_major=hm, logits_finite=fa and fb, ln_fold=[fold_a, fold_b])
            log(f"{model} b{BATCH} {dname}: ROPE {ma:.3f} ms median ({r['rope_step_ms_min']:.3f} min) = {r['rope_images_per_s']:.0f} images/s | cleared "
                f"{mb:.3f} ms ({r['plain_step_ms_min']:.3f} min) = {r['plain_images_per_s']:.0f} images/s | step ratio {r['step_ratio']:.4f} (per pass "
                f"{' '.join(f'{x:.4f}' for x in pass_ratio)}) | difference {per_layer_us:.1f} us per layer; {nbytes / 1e6:.1f} MB per layer / 4.33 TB/s = "
                f"{r['bytes_over_rate_us']:.1f} us, ratio {per_layer_us / r['bytes_over_rate_us']:.2f} | q|k|v head-major {hm[0]}/{hm[1]}, fold {fold_a}/{fold_b}, "
                f"finite {r['logits_finite']}")
            log("    neighbouring stages, us per launch ROPE / cleared (ratio): " + ", ".join(f"{n} {x:.1f} / {y:.1f} ({x / y:.4f})" for n, (x, y) in st.items()))
            if dname != "fp8":
                r["tap"] = []
                for layout, (med, mn), (med1, mn1) in tap(cfg, dname, BATCH, 40):
                    net = med - med1
                    r["tap"].append(dict(layout=layout, us_median=med, us_min=mn, one_image_us_median=med1, one_image_us_min=mn1, net_us=net,
                                         ratio_to_bytes_over_rate=net / r["bytes_over_rate_us"]))
                    log(f"    the launch on its own (tap, {layout}, 40 synchronous calls, host time): {med:.1f} us median ({mn:.1f} min) | one image "
                        f"{med1:.1f} us ({mn1:.1f} min) | net {net:.1f} us = {nbytes / net / 1e6:.2f} TB/s, {net / r['bytes_over_rate_us']:.2f} x bytes / 4.33 TB/s")
            rows.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rope_bench.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "rope_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
