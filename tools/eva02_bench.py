#!/usr/bin/env python3
"""EVA-02 measurements (run on the GPU box): what the gate pass with the inner LayerNorm (FLAG_SUB_LN) costs in place, beside the plain
gate pass of the same shape in the same run.

  python tools/eva02_bench.py [--out profiles] [--steps 10] [--passes 3]

EVA-02-B/14 at 224 x 224 (dim 768, 12 heads, 12 layers, M 2048, 257 tokens, batch 256) and EVA-02-L/14 (dim 1024, 16 heads, 24 layers, gated
width n 2730 inside M 2816, batch 128), rotary, bf16 and fp16, seeded weights, in ONE process and interleaved (A, P, B, A, P, B, ...):
  A = the FLAG_ROPE | FLAG_SWIGLU | FLAG_SUB_LN context as it runs (EVA-02-L: the seeded blob reloaded with subln.width = 2730);
  P = the same shape with FLAG_SUB_LN cleared: the plain gate pass, the yardstick;
  B = A created under VH_SWIGLU_SKIP=1: every launch but the pass (fc2 reads whatever h16 holds: timing only).
Reported: median and min step of each, images/s of A, the pass per layer (A - B) / layers and (P - B) / layers, their ratio, each beside
rows * 3 M * 2 bytes / 4.33 TB/s.  No number here is a threshold.  Writes eva02_bench.txt.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))

import vithip  # noqa: E402

DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16}
RATE = 4.33e12
BASE = dict(image_size=224, patch_size=14, channels=3, classes=1000)
RUNS = [("EVA-02-B/14", dict(BASE, dim=768, heads=12, mlp_dim=2048, layers=12), 2048, 256),
        ("EVA-02-L/14", dict(BASE, dim=1024, heads=16, mlp_dim=2816, layers=24), 2730, 128)]
FULL = vithip.FLAG_ROPE | vithip.FLAG_SWIGLU | vithip.FLAG_SUB_LN


class Run:
    def __init__(self, cfg, dname, batch, flags, width=None, skip=False):
        self.cfg, self.batch = cfg, batch
        if skip:
            os.environ["VH_SWIGLU_SKIP"] = "1"
        try:   # the switch is read when the context is created
            self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags)
        finally:
            os.environ.pop("VH_SWIGLU_SKIP", None)
        self.ctx.init_weights_seeded(0)
        if width is not None and width != cfg["mlp_dim"]:   # the true width of a padded model: the word in front of the two subln tensors
            blob = self.ctx.export_weights()
            at = blob.size - 4 * (1 + 2 * cfg["layers"] * cfg["mlp_dim"])
            blob[at:at + 4] = np.array([width], np.float32).view(np.uint8)
            self.ctx.load_weights(blob)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp16")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"eva02_bench: FLAG_SUB_LN as it runs (A), the same shape with the plain gate pass (P: the flag cleared) and without the pass (B: "
        f"VH_SWIGLU_SKIP=1); {a.steps} timed steps per pass, {a.passes} interleaved passes per context (A P B A P B ...)")
    for model, cfg, width, batch in RUNS:
        M, layers = cfg["mlp_dim"], cfg["layers"]
        T = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
        for dname in a.dtypes.split(","):
            ctxs = [Run(cfg, dname, batch, FULL, width), Run(cfg, dname, batch, FULL & ~vithip.FLAG_SUB_LN), Run(cfg, dname, batch, FULL, width, skip=True)]
            rows_g = -(-batch * T // 256) * 256 if ctxs[0].tiled else batch * T   # (the folded loop pads its GEMM rows: swiglu_bench.py)
            floor_us = rows_g * 3 * M * 2 / RATE * 1e6
            st = [[], [], []]
            for _ in range(a.passes):
                for i, c in enumerate(ctxs):
                    st[i].append(c.steps(a.steps))
            per_pass = [[float(np.median(x)) for x in s] for s in st]
            st = [np.concatenate(s) for s in st]
            tiled, finite = [c.tiled for c in ctxs], [c.close() for c in ctxs]
            ma, mp, mb = (float(np.median(s)) for s in st)
            sub, plain = (ma - mb) * 1e3 / layers, (mp - mb) * 1e3 / layers
            log(f"{model} b{batch} {dname} ({T} tokens, {rows_g} GEMM rows, M {M}, n {width}): A {ma:.3f} ms median ({st[0].min():.3f} min) = "
                f"{batch / (ma * 1e-3):.0f} images/s | P (plain gate) {mp:.3f} ms ({st[1].min():.3f} min) | B (no pass) {mb:.3f} ms ({st[2].min():.3f} min) | "
                f"A / P = {ma / mp:.4f} | h tiled A/P/B {tiled}, finite A/P {finite[0]}/{finite[1]}")
            log(f"    the pass per layer: with the LayerNorm (A - B) / {layers} = {sub:.1f} us, plain (P - B) / {layers} = {plain:.1f} us, ratio {sub / plain:.2f} | "
                f"{rows_g * 3 * M * 2 / 1e6:.1f} MB per layer / 4.33 TB/s = {floor_us:.1f} us: {sub / floor_us:.2f} x and {plain / floor_us:.2f} x")
            log("    per pass, ms median A / P / B: " + "; ".join(f"{x:.3f} / {y:.3f} / {z:.3f}" for x, y, z in zip(*per_pass)))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "eva02_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
