#!/usr/bin/env python3
"""Feature-moments measurements (run on the GPU box): what the column sums and X^T X of all patch rows of a batch cost.

  python tools/moments_bench.py [--out profiles] [--passes 7]

In ONE process, one context per model, synthetic weights and images: ViT-B/16 bf16 at batch 512 (R = 100 352 rows, W = 768) and ViT-L/14
fp16 at batch 256 (R = 65 536, W = 1024), all images.  `passes` interleaved passes, the median with min and max, of
  step     one synchronous forward (device buffers), wall time;
  call     one synchronous vh_patch_moments_device: the prepare pass, the list pass, the moments and the merge, wall time;
  launch   the synchronous vh_op_moments on unit rows of the same shape;
  torch    x.T @ x of the same rows (only where torch is importable and sees the device), synchronised;
beside two floors measured in the same passes:
  flops    R W (W + 128) multiply-adds (the upper triangle in 128-column tiles), 2 flops each, at the rate of the forward's fc2 GEMM
           (vh_bench_gemm, the better of variants 5 and 6);
  bytes    reading the R W 16-bit rows once at the rate of a streaming cast (vh_op_cast over 2^28 elements, 6 bytes per element).
No threshold is asserted: the tool records what it sees.  Written to <out>/moments_bench.txt.
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


def torch_gram(x16, dt):
    """A closure timing x.T @ x of the rows on the device with torch, or None."""
    try:
        import torch
        if not torch.cuda.is_available():
            return None
        t = torch.from_numpy(vithip.from16(x16, dt).astype(np.float32)).to("cuda").to(torch.bfloat16 if dt == vithip.DTYPE_BF16 else torch.float16)

        def run():
            (t.T @ t).sum().item()
        return run
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("moments_bench: no HIP device visible")
    runs = []
    for name, cfg, dt, batch, _ in MODELS:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
        ctx.load_weights(S.make_blob(cfg, 0))
        npatch, dim = (cfg["image_size"] // cfg["patch_size"]) ** 2, cfg["dim"]
        rows = batch * npatch
        d_in = vithip.DeviceBuffer.from_numpy(S.make_images(cfg, 1, batch))
        d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        d_img = vithip.DeviceBuffer.from_numpy(np.arange(batch, dtype=np.int32))
        d_sum, d_gram, d_cnt = vithip.DeviceBuffer(dim * 4), vithip.DeviceBuffer(dim * dim * 4), vithip.DeviceBuffer(16)
        d_ws = vithip.DeviceBuffer(vithip.op_moments_workspace_bytes(rows, dim))
        x = np.random.default_rng(0).standard_normal((rows, dim)).astype(np.float32)
        x16 = vithip.to16(x / np.linalg.norm(x, axis=1, keepdims=True), dt)
        d_rows = vithip.DeviceBuffer.from_numpy(x16)
        desc = vithip.MomentsDesc(vithip.FEAT_NORM, -1, 0, batch)
        fns = {"step": lambda c=ctx, i=d_in, o=d_out, b=batch: c.forward_device(i.ptr, b, o.ptr),
               "call": lambda c=ctx, d=desc, i=d_img, s=d_sum, g=d_gram, n=d_cnt: c.patch_moments_device(d, i.ptr, s.ptr, g.ptr, n.ptr),
               "launch": lambda r=d_rows, dt=dt, R=rows, w=dim, s=d_sum, g=d_gram, n=d_cnt, ws=d_ws: vithip.op_moments(
                   r.ptr, dt, R, w, 0, s.ptr, g.ptr, n.ptr, ws.ptr)}
        tg = torch_gram(x16, dt)
        if tg:
            fns["torch"] = tg
        runs.append((name, batch, rows, dim, fns, {k: [] for k in fns}))
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
    lines = [f"moments_bench: {a.passes} interleaved passes, median [min .. max] ms; streaming rate {rate_b / 1e12:.2f} TB/s (cast, median "
             f"{statistics.median(t_cast):.3f} ms), fc2 rate {rate_f / 1e12:.0f} TFLOP/s (median {statistics.median(t_fc2):.3f} ms)"]
    for name, batch, rows, dim, _, t in runs:
        m = {k: statistics.median(v) for k, v in t.items()}
        ff, bf = 2.0 * rows * dim * (dim + 128) / rate_f * 1e3, rows * dim * 2 / rate_b * 1e3
        lines += [f"  {name} b{batch}, all {batch} images, R {rows}, W {dim}, {vithip.op_moments_slabs(rows, dim)} slabs:",
                  f"    step   {med(t['step'])}",
                  f"    call   {med(t['call'])}   = {100 * m['call'] / m['step']:.2f} % of a step",
                  f"    launch {med(t['launch'])}   flop floor {ff:.4f} ({m['launch'] / ff:.1f} x), byte floor {bf:.4f} ({m['launch'] / bf:.1f} x)"]
        if "torch" in t:
            lines.append(f"    torch  {med(t['torch'])}   x.T @ x of the same rows ({m['launch'] / m['torch']:.2f} x of it)")
    print("\n".join(lines), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "moments_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
