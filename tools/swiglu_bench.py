#!/usr/bin/env python3
"""SwiGLU gate-pass measurements (run on the GPU box): what the pass behind fc1 costs, in place and on its own.

  python tools/swiglu_bench.py [--out profiles] [--steps 10] [--passes 3]

DINOv2-g/14 at 224 x 224 (dim 1536, 24 heads, 40 layers, M 4096, 257 tokens) and DINOv3 ViT-H+/16 (dim 1280, 20 heads, 32 layers, M 5120,
4 registers, rotary), batch 128, in bf16 and fp16, seeded weights, in ONE process and interleaved (A, B, C, A, B, C, ... per model and
dtype, so that all see the same box and clock):
  A = the FLAG_SWIGLU context as it runs (h tiled where fc2 takes the persistent form);
  B = the same context created under VH_SWIGLU_SKIP=1: every launch but the gate pass (fc2 reads whatever h16 holds: timing only);
  C = the same context created under VH_H_TILED=0: the row-major pass in front of the row-major fc2.
  (1) whole forward of each: forward_device_async with step timing; median and min step, images/s; (A - B) / layers = the pass per
      launch IN PLACE; C / A = what the tiled form is worth;
  (2) the pass ON ITS OWN through the tap vh_op_swiglu on buffers of the model's shape, both layouts: host time per synchronous call minus
      the same call on 16 rows (launch + synchronisation);
  each beside rows * 3 M * 2 bytes / 4.33 TB/s, the HBM rate the README uses, with the ratio.
No number here is a threshold: the ratios are what fusing the gate into fc1's epilogue will be judged against.
Writes swiglu_bench.txt and swiglu_bench.json.  The towers are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
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

DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16}
BATCH, RATE = 128, 4.33e12
RUNS = [("DINOv2-g/14", dict(image_size=224, patch_size=14, channels=3, dim=1536, heads=24, mlp_dim=4096, layers=40, classes=1000), 0, 0),
        ("DINOv3-H+/16", dict(image_size=224, patch_size=16, channels=3, dim=1280, heads=20, mlp_dim=5120, layers=32, classes=1000), 4, vithip.FLAG_ROPE)]


class Run:
    def __init__(self, cfg, regs, dname, batch, flags, env=None):
        self.cfg, self.batch = cfg, batch
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:   # the switches are read when the context is created
            self.ctx = vithip.VitContext(dict(cfg, registers=regs), dtype=DT[dname], max_batch=batch, flags=flags)
        finally:
            for k in env or {}:
                del os.environ[k]
        self.ctx.init_weights_seeded(0)
        self.din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
        self.dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        self.ctx.fill_input_seeded(1, batch, self.din.ptr)
        self.ctx.forward_device_async(self.din.ptr, batch, self.dout.ptr, steps=3)   # warm-up
        self.ctx.synchronize()
        self.tiled = int(self.ctx.debug_read(3, 1)[0])

    def steps(self, n):
        self.ctx.set_step_timing(True)
        self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps=n)
        self.ctx.synchronize()
        st = np.array(self.ctx.get_step_timing())
        self.ctx.set_step_timing(False)
        return st

    def close(self):
        finite = bool(np.isfinite(self.dout.to_numpy(np.float32, (self.batch, self.cfg["classes"]))).all())
        self.ctx.close(); self.din.free(); self.dout.free()
        return finite


def tap(rows, M, dname, calls):
    """us per synchronous vh_op_swiglu call on gu [rows][2 M], per layout: (layout, whole buffer, 16 rows)."""
    gu = vithip.DeviceBuffer.from_numpy(np.full(rows * 2 * M, 0x3C00, np.uint16))   # a finite value in both 16-bit types
    h = vithip.DeviceBuffer(rows * M * 2)
    out = []
    for layout, tiled in (("row-major", False), ("tiled", True)):
        res = []
        for r in (rows, 16):
            t = []
            for i in range(calls + 3):
                t0 = time.perf_counter()
                vithip.op_swiglu(gu.ptr, DT[dname], r, M, h.ptr, tiled)
                t.append((time.perf_counter() - t0) * 1e6)
            res.append((float(np.median(t[3:])), float(np.min(t[3:]))))
        out.append((layout, res[0], res[1]))
    gu.free(); h.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--models", default=",".join(r[0] for r in RUNS))
    a = ap.parse_args()
    lines, rows_out = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"swiglu_bench: FLAG_SWIGLU as it runs (A), with the gate pass left out (B: VH_SWIGLU_SKIP=1) and with the row-major h (C: VH_H_TILED=0); "
        f"batch {BATCH}, {a.steps} timed steps per pass, {a.passes} interleaved passes per context (A B C A B C ...)")
    for model, cfg, regs, more in RUNS:
        if model not in a.models.split(","):
            continue
        M, layers = cfg["mlp_dim"], cfg["layers"]
        T = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1 + regs
        rows = BATCH * T
        for dname in a.dtypes.split(","):
            flags = vithip.FLAG_SWIGLU | more
            ctxs = [Run(cfg, regs, dname, BATCH, flags), Run(cfg, regs, dname, BATCH, flags, {"VH_SWIGLU_SKIP": "1"}),
                    Run(cfg, regs, dname, BATCH, flags, {"VH_H_TILED": "0"})]
            # the folded loop pads its GEMM rows to whole 256-row tiles only from two rounds of tiles on; a tiled h tells that it did
            rows_g = -(-rows // 256) * 256 if ctxs[0].tiled else rows
            floor_us = rows_g * 3 * M * 2 / RATE * 1e6
            st = [[], [], []]
            for _ in range(a.passes):
                for i, c in enumerate(ctxs):
                    st[i].append(c.steps(a.steps))
            per_pass = [[float(np.median(x)) for x in s] for s in st]
            st = [np.concatenate(s) for s in st]
            tiled = [c.tiled for c in ctxs]
            finite = [c.close() for c in ctxs]
            ma, mb, mc = (float(np.median(s)) for s in st)
            in_place = (ma - mb) * 1e3 / layers
            in_place_rm = (mc - mb) * 1e3 / layers
            r = dict(model=model, dtype=dname, batch=BATCH, tokens=T, rows=rows, rows_gemm=rows_g, step_ms_median=dict(A=ma, B=mb, C=mc),
                     step_ms_min=dict(A=float(st[0].min()), B=float(st[1].min()), C=float(st[2].min())), step_ms_median_per_pass=per_pass,
                     images_per_s=BATCH / (ma * 1e-3), images_per_s_row_major=BATCH / (mc * 1e-3), in_place_us_per_layer=in_place,
                     in_place_row_major_us_per_layer=in_place_rm, bytes_per_layer=rows_g * 3 * M * 2, bytes_over_rate_us=floor_us,
                     h_tiled=tiled, logits_finite_A_C=[finite[0], finite[2]])
            log(f"{model} b{BATCH} {dname} ({T} tokens, {rows_g} GEMM rows): A {ma:.3f} ms median ({r['step_ms_min']['A']:.3f} min) = {r['images_per_s']:.0f} images/s | "
                f"B (no pass) {mb:.3f} ms ({r['step_ms_min']['B']:.3f} min) | C (row-major h) {mc:.3f} ms ({r['step_ms_min']['C']:.3f} min) = "
                f"{r['images_per_s_row_major']:.0f} images/s, C / A = {mc / ma:.4f} | h tiled A/B/C {tiled}, finite A/C {finite[0]}/{finite[2]}")
            log(f"    the pass in place: (A - B) / {layers} layers = {in_place:.1f} us per launch (tiled out), (C - B) / {layers} = {in_place_rm:.1f} us (row-major out, "
                f"with what the row-major fc2 costs) | {r['bytes_per_layer'] / 1e6:.1f} MB per layer / 4.33 TB/s = {floor_us:.1f} us, ratio {in_place / floor_us:.2f} (tiled)")
            log("    per pass, ms median A / B / C: " + "; ".join(f"{x:.3f} / {y:.3f} / {z:.3f}" for x, y, z in zip(*per_pass)))
            r["tap"] = []
            for layout, (med, mn), (med1, mn1) in tap(rows_g, M, dname, 30):
                net = med - med1
                r["tap"].append(dict(layout=layout, us_median=med, us_min=mn, rows16_us_median=med1, rows16_us_min=mn1, net_us=net, ratio_to_bytes_over_rate=net / floor_us))
                log(f"    the launch on its own (tap, {layout}, 30 synchronous calls, host time): {med:.1f} us median ({mn:.1f} min) | 16 rows {med1:.1f} us "
                    f"({mn1:.1f} min) | net {net:.1f} us = {r['bytes_per_layer'] / net / 1e6:.2f} TB/s, {net / floor_us:.2f} x bytes / 4.33 TB/s")
            rows_out.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "swiglu_bench.json"), "w") as f:
        json.dump(rows_out, f, indent=1)
    with open(os.path.join(a.out, "swiglu_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
