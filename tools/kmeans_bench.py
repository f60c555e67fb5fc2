#!/usr/bin/env python3
"""Patch-clustering measurements (run on the GPU box): what k-means of the patches of every image costs beside the forward.

  python tools/kmeans_bench.py [--out profiles] [--passes 7]

In ONE process, one context per model, synthetic weights and images: ViT-B/16 bf16 at batch 512 and ViT-L/14 fp16 at batch 256, all
images, K = 8 and 32, 10 iterations, spherical k-means, the stride init.  `passes` interleaved passes, the median with min and max, of
  step     one synchronous forward (device buffers), wall time;
  call     one synchronous vh_cluster_patches_device: the prepare pass, the clustering and the widening pass, wall time;
  launch   the synchronous vh_op_kmeans on unit rows of the same shape;
beside two floors measured in the same passes:
  flops    per image 2 (iters + 1) NP K D for the assignments and 2 iters NP K D for the updates (the kernel's second COSINE update pass
           is overhead against this floor) at the rate of the forward's fc2 GEMM (vh_bench_gemm, the better of variants 5 and 6);
  bytes    the rate of a streaming cast (vh_op_cast over 2^28 elements, 6 bytes per element), reported for reference.
No threshold is asserted: the tool records what it sees.  Written to <out>/kmeans_bench.txt.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402
from match_bench import CAST_ELEMS, FC2, MODELS, med, wall_ms  # noqa: E402

KS, ITERS = (8, 32), 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("kmeans_bench: no HIP device visible")
    runs = []
    for name, cfg, dt, batch, _ in MODELS:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
        ctx.load_weights(S.make_blob(cfg, 0))
        npatch, dim = (cfg["image_size"] // cfg["patch_size"]) ** 2, cfg["dim"]
        d_in = vithip.DeviceBuffer.from_numpy(S.make_images(cfg, 1, batch))
        d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        d_img = vithip.DeviceBuffer.from_numpy(np.arange(batch, dtype=np.int32))
        d_lab, d_cnt = vithip.DeviceBuffer(batch * npatch * 4), vithip.DeviceBuffer(batch * max(KS) * 4)
        d_c32, d_c16 = vithip.DeviceBuffer(batch * max(KS) * dim * 4), vithip.DeviceBuffer(batch * max(KS) * dim * 2)
        x = np.random.default_rng(0).standard_normal((batch * npatch, dim)).astype(np.float32)
        d_rows = vithip.DeviceBuffer.from_numpy(vithip.to16(x / np.linalg.norm(x, axis=1, keepdims=True), dt))
        fns = {"step": lambda c=ctx, i=d_in, o=d_out, b=batch: c.forward_device(i.ptr, b, o.ptr)}
        for k in KS:
            desc = vithip.KmeansDesc(vithip.FEAT_NORM, -1, vithip.KMEANS_COSINE, k, ITERS, vithip.KMEANS_INIT_STRIDE, batch, 0)
            fns[f"call{k}"] = lambda c=ctx, d=desc, i=d_img, l=d_lab, c32=d_c32, n=d_cnt: c.cluster_patches_device(d, i.ptr, None, l.ptr, c32.ptr, n.ptr)
            fns[f"launch{k}"] = lambda r=d_rows, dt=dt, b=batch, p=npatch, w=dim, k=k, l=d_lab, c16=d_c16, n=d_cnt: vithip.op_kmeans(
                r.ptr, dt, b, p, w, k, ITERS, vithip.KMEANS_COSINE, None, l.ptr, c16.ptr, n.ptr)
        runs.append((name, batch, npatch, dim, fns, {k: [] for k in fns}))
    c_in, c_out = vithip.DeviceBuffer(CAST_ELEMS * 4), vithip.DeviceBuffer(CAST_ELEMS * 2)

    def cast():
        vithip._check(vithip.lib().vh_op_cast(c_in.ptr, c_out.ptr, CAST_ELEMS, vithip.DTYPE_BF16, None))

    for r in runs:   # warm-up: code objects, the dynamic-LDS attribute, the scratches
        for fn in r[4].values():
            fn()
    cast()
    t_cast, t_fc2 = [], []
    for _ in range(a.passes):
        for r in runs:
            for k, fn in r[4].items():
                r[5][k].append(wall_ms(fn))
        t_cast.append(wall_ms(cast))
        t_fc2.append(min(vithip.bench_gemm(*FC2, vithip.EPI_BIAS_RESID, vithip.DTYPE_BF16, v, 10) for v in (5, 6)))
    rate_b = CAST_ELEMS * 6 / (statistics.median(t_cast) * 1e-3)
    rate_f = 2.0 * FC2[0] * FC2[1] * FC2[2] / (statistics.median(t_fc2) * 1e-3)
    lines = [f"kmeans_bench: {a.passes} interleaved passes, median [min .. max] ms; {ITERS} iterations, cosine, stride init; streaming rate "
             f"{rate_b / 1e12:.2f} TB/s (cast, median {statistics.median(t_cast):.3f} ms), fc2 rate {rate_f / 1e12:.0f} TFLOP/s "
             f"(median {statistics.median(t_fc2):.3f} ms)"]
    for name, batch, npatch, dim, _, t in runs:
        m = {k: statistics.median(v) for k, v in t.items()}
        lines += [f"  {name} b{batch}, all {batch} images, NP {npatch}, D {dim}:", f"    step      {med(t['step'])}"]
        for k in KS:
            ff = batch * (2.0 * (ITERS + 1) + 2.0 * ITERS) * npatch * k * dim / rate_f * 1e3
            lines += [f"    K {k:2d} call   {med(t[f'call{k}'])}   = {100 * m[f'call{k}'] / m['step']:.2f} % of a step",
                      f"    K {k:2d} launch {med(t[f'launch{k}'])}   flop floor {ff:.4f} ({m[f'launch{k}'] / ff:.1f} x)"]
    print("\n".join(lines), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "kmeans_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
