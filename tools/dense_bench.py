#!/usr/bin/env python3
"""Dense-head measurements (run on the GPU box): what the per-patch logits and the class map of a finished forward cost.

  python tools/dense_bench.py [--out profiles] [--passes 7] [--steps 4] [--map 224]

In ONE process, one context per model: ViT-B/16 bf16 at batch 512 and ViT-L/14 fp16 at batch 256, a seeded head of C = 21 and of
C = 150 classes (VH_FEAT_NORM).  `passes` interleaved passes of
  the forward with no head set and with the head set (vh_forward_device_async, `steps` steps, wall time per step: the default line),
  the synchronous vh_read_dense_logits_device (fp32) and vh_read_dense_map_device (map x map, with scores), wall time of each call,
the median pass reported with min and max.  The logits call IS the head launch; the map call is the head launch plus the upsample +
argmax launch, so the second launch is reported as their difference.  Each kernel stands beside its byte floor at 4.33 TB/s, the
copy rate this project measures: the head's floor is the rows' planes in + the logits out, the map's the logits in + classes and
scores out.  The default line is also what to hold against the parent commit's `python bench.py` on the same box.  No threshold is
asserted: the tool records what it sees.  Written to <out>/dense_bench.txt.
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
CLASSES = (21, 150)
HBM_BYTES_PER_S = 4.33e12


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(name, cfg, dtype, batch, passes, steps, side, say):
    D, g = cfg["dim"], cfg["image_size"] // cfg["patch_size"]
    NP = g * g
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch)
    ctx.init_weights_seeded(0)
    plane_bytes = 3 if ctx.ln_fold() else 4
    d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, d_in.ptr)
    d_logits = vithip.DeviceBuffer(batch * max(CLASSES) * NP * 4)
    d_cls, d_score = vithip.DeviceBuffer(batch * side * side), vithip.DeviceBuffer(batch * side * side * 4)
    L = vithip.lib()

    def step():
        ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=steps)
        ctx.synchronize()

    rng = np.random.default_rng(0)
    heads = {c: ((0.05 * rng.standard_normal((c, D))).astype(np.float32), np.zeros(c, np.float32)) for c in CLASSES}
    keys = ["step, no head"] + [f"{k}, C={c}" for c in CLASSES for k in ("step, head set", "logits fp32", f"map {side}x{side}")]
    t = {k: [] for k in keys}
    step()
    for _ in range(passes):
        ctx.set_dense_head(None)
        t["step, no head"].append(wall_ms(step) / steps)
        for c in CLASSES:
            ctx.set_dense_head(*heads[c], norm=True)
            t[f"step, head set, C={c}"].append(wall_ms(step) / steps)
            t[f"logits fp32, C={c}"].append(wall_ms(lambda: vithip._check(L.vh_read_dense_logits_device(ctx.h, batch, d_logits.ptr, vithip.ELEM_F32), ctx.h)))
            t[f"map {side}x{side}, C={c}"].append(wall_ms(lambda: vithip._check(L.vh_read_dense_map_device(ctx.h, batch, side, side, d_cls.ptr, d_score.ptr), ctx.h)))
    say(f"{name}: dim {D}, {NP} patches, residual rows {plane_bytes} B per element, {passes} passes, median [min .. max] ms")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in keys:
        say(f"  {k:24s} {med[k]:9.3f}  [{min(t[k]):.3f} .. {max(t[k]):.3f}]")
    for c in CLASSES:
        head_floor = (batch * NP * D * plane_bytes + batch * NP * c * 4) / HBM_BYTES_PER_S * 1e3
        map_floor = (batch * NP * c * 4 + batch * side * side * 5) / HBM_BYTES_PER_S * 1e3
        head_ms = med[f"logits fp32, C={c}"]
        map_ms = med[f"map {side}x{side}, C={c}"] - head_ms
        say(f"  C={c}: head launch {head_ms:.3f} ms = {head_ms / head_floor:.1f} x its byte floor {head_floor:.3f} ms;  upsample + argmax "
            f"{map_ms:.3f} ms = {map_ms / map_floor:.1f} x its byte floor {map_floor:.3f} ms  (wall times of synchronous calls: launch and "
            "synchronisation overhead included)")
    for d in (d_in, d_out, d_logits, d_cls, d_score):
        d.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--map", type=int, default=224)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, cfg, dtype, batch in MODELS:
        if a.only is None or a.only in name:
            measure(name, cfg, dtype, batch, a.passes, a.steps, a.map, say)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "dense_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
