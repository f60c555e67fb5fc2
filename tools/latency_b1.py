#!/usr/bin/env python3
"""Batch-1 latency of one build, graph off, for A/B runs of the host path.

    tools/latency_b1.py --tree <checkout with a built vit-fpga_amd/libvithip.so> --label NAME

tools/forward_fingerprint.py's fp16_b1 context (ViT-B/16 fp16, max_batch 1, no flags): 50 synchronous forwards of warm-up, then
three passes of 200.  Per pass it prints the median, minimum and maximum of last_kernel_ms -- the time between the stream events
around the forward; at batch 1 the forward is launch-bound, so the host's enqueue pace is inside it -- and the median and
minimum wall time of the call.
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True, help="checkout to import vithip from (vit-fpga_amd/python, built library beside it)")
ap.add_argument("--label", required=True, help="name of the build in the printed lines")
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "vit-fpga_amd", "python"))
import vithip  # noqa: E402

cfg = dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=1000)
ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_FP16, max_batch=1, device=0, flags=0)
ctx.init_weights_seeded(0)
x = vithip.DeviceBuffer(224 * 224 * 3 * 4)
y = vithip.DeviceBuffer(1000 * 4)
ctx.fill_input_seeded(1, 1, x.ptr)
for _ in range(50):
    ctx.forward_device(x.ptr, 1, y.ptr)
for p in range(3):
    ms, wall = [], []
    for _ in range(200):
        t0 = time.perf_counter()
        ctx.forward_device(x.ptr, 1, y.ptr)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_kernel_ms())
    print(f"b1 {a.label} pass {p}: last_kernel_ms median {np.median(ms):.4f} min {min(ms):.4f} max {max(ms):.4f}   "
          f"wall ms median {np.median(wall):.4f} min {min(wall):.4f}", flush=True)
ctx.close()
