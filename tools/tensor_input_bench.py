#!/usr/bin/env python3
"""Image-tensor input measurements (run on the GPU box): what each (element type, layout) costs against the NHWC fp32 entry point.

  python tools/tensor_input_bench.py [--out profiles] [--steps 20] [--passes 5] [--batch 512]

In ONE process and ONE context, ViT-B/16 bf16 at batch 512, HBM-resident inputs: NHWC fp32 through vh_forward_device_async
(today's entry point) and every (elem, layout) through vh_forward_device_tensor_async, interleaved, `passes` times.
  (1) step time: step timing on, `steps` forwards, the median step of the pass; per format the median over the passes [min .. max];
  (2) the "im2col" stage: hip events around its launches (vh_set_stage_timing), 8 forwards per pass, the average per launch; per
      format the median over the passes.
Every format holds the same images (u8 pixels; the float tensors are those pixels normalised on the host with ImageNet mean /
std, then narrowed), and the u8 and fp32 formats must give the logits of the NHWC fp32 run, bit for bit, which is checked.
CONDITION: the median step time of every format <= the NHWC fp32 median x (1 + s), s = (max - min) / median of the NHWC fp32
passes of this run.  Written to <out>/tensor_input.txt.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ELEM_NAME = {vithip.ELEM_F32: "f32", vithip.ELEM_F16: "f16", vithip.ELEM_BF16: "bf16", vithip.ELEM_U8: "u8"}
LAYOUT_NAME = {vithip.LAYOUT_NHWC: "NHWC", vithip.LAYOUT_NCHW: "NCHW"}


def host_tensor(u8, x32, elem, layout):
    a = {vithip.ELEM_F32: lambda: x32, vithip.ELEM_F16: lambda: x32.astype(np.float16),
         vithip.ELEM_BF16: lambda: vithip.to_bf16_bits(x32), vithip.ELEM_U8: lambda: u8}[elem]()
    return np.ascontiguousarray(a if layout == vithip.LAYOUT_NHWC else a.transpose(0, 3, 1, 2))


class Format:
    def __init__(self, ctx, name, batch, dout, host, elem=None, layout=None):
        self.ctx, self.name, self.batch, self.dout, self.elem, self.layout = ctx, name, batch, dout, elem, layout
        self.din = vithip.DeviceBuffer.from_numpy(host)
        self.mbytes = host.nbytes / 1e6
        self.steps_ms, self.im2col_us = [], []

    def fwd(self, steps):
        if self.elem is None:
            self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps)
        else:
            self.ctx.forward_device_tensor_async(self.din.ptr, self.elem, self.layout, self.batch, self.dout.ptr, steps)

    def logits(self):
        self.fwd(1)
        self.ctx.synchronize()
        return self.dout.to_numpy(np.float32, (self.batch, self.ctx.cfg["classes"]))

    def step_pass(self, steps):
        self.ctx.set_step_timing(True)
        self.fwd(steps)
        self.ctx.synchronize()
        st = np.array(self.ctx.get_step_timing())
        self.ctx.set_step_timing(False)
        self.steps_ms.append(float(np.median(st)))

    def im2col_pass(self, steps):
        self.ctx.set_stage_timing("im2col")
        self.fwd(steps)
        self.ctx.synchronize()
        avg_ms, _, _ = self.ctx.get_stage_timing()
        self.ctx.set_stage_timing(None)
        self.im2col_us.append(avg_ms * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    cfg, batch = S.CONFIGS["vit_base"], a.batch
    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    rng = np.random.default_rng(3)
    unit = min(batch, 32)                    # 32 distinct images, repeated: the gather's time does not depend on the pixel values
    u8 = np.tile(rng.integers(0, 256, size=(unit, cfg["image_size"], cfg["image_size"], cfg["channels"]), dtype=np.uint8),
                 ((batch + unit - 1) // unit, 1, 1, 1))[:batch]
    x32 = (u8.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=batch)
    ctx.init_weights_seeded(0)
    ctx.set_input_norm(scale, shift)
    dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    base = Format(ctx, "NHWC f32 (vh_forward_device_async)", batch, dout, x32)
    formats = [base]
    for layout in (vithip.LAYOUT_NHWC, vithip.LAYOUT_NCHW):
        for elem in (vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16, vithip.ELEM_U8):
            formats.append(Format(ctx, f"{LAYOUT_NAME[layout]} {ELEM_NAME[elem]}", batch, dout, host_tensor(u8, x32, elem, layout), elem, layout))
    ref = base.logits()
    exact = {f.name: bool(np.array_equal(f.logits().view(np.uint32), ref.view(np.uint32)))
             for f in formats if f.elem in (None, vithip.ELEM_F32, vithip.ELEM_U8)}
    for f in formats:                         # warm-up
        f.fwd(2)
    ctx.synchronize()
    for _ in range(a.passes):
        for f in formats:
            f.step_pass(a.steps)
    for _ in range(a.passes):
        for f in formats:
            f.im2col_pass(8)
    log(f"tensor_input_bench: ViT-B/16 bf16 batch {batch}, HBM-resident inputs, one context; {a.passes} interleaved passes of {a.steps} "
        f"steps (median step per pass) and of 8 forwards with the im2col stage timed")
    log(f"logits bit-identical to the NHWC fp32 run (fp32 and u8 formats; finite: {bool(np.isfinite(ref).all())}): {exact}")
    b_med, b_min, b_max = float(np.median(base.steps_ms)), min(base.steps_ms), max(base.steps_ms)
    s = (b_max - b_min) / b_med
    bound = b_med * (1 + s)
    log(f"NHWC fp32 passes: median {b_med:.4f} ms, min {b_min:.4f}, max {b_max:.4f}: spread s = {100 * s:.3f} %, bound = {bound:.4f} ms")
    log(f"{'format':36s} {'input MB':>9s} {'step ms median [min .. max]':>34s} {'vs fp32':>9s} {'<= bound':>9s} {'im2col us median [min .. max]':>34s}")
    missed = []
    for f in formats:
        m, lo, hi = float(np.median(f.steps_ms)), min(f.steps_ms), max(f.steps_ms)
        im, ilo, ihi = float(np.median(f.im2col_us)), min(f.im2col_us), max(f.im2col_us)
        ok = m <= bound
        if not ok:
            missed.append(f.name)
        log(f"{f.name:36s} {f.mbytes:9.1f} {m:12.4f} [{lo:8.4f} .. {hi:8.4f}] {100 * (m / b_med - 1):+8.3f}% {'yes' if ok else 'NO':>9s} "
            f"{im:12.1f} [{ilo:8.1f} .. {ihi:8.1f}]")
    log("CONDITION (every format's median step <= NHWC fp32 median x (1 + s)): " + ("met" if not missed else "MISSED by " + ", ".join(missed)))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor_input.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
