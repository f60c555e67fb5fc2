#!/usr/bin/env python3
"""Label-propagation measurements (run on the GPU box): what the top-k neighbours of several source frames and their label vote cost
beside the forward and beside the match, the only way to the top-1 before it.

  python tools/propagate_bench.py [--out profiles] [--passes 7]

In ONE process, one context per model, synthetic weights and images: ViT-B/16 bf16 at batch 512, ViT-L/14 fp16 at batch 256.  64 items,
item i = frame i + 7 with its seven predecessors as sources (S = 7), k = 5, tau 0.1, 8 classes, at radius 0 and at radius 4.  `passes`
interleaved passes, the median reported with min and max, of
  step     one synchronous forward (device buffers), wall time;
  call     one synchronous vh_propagate_labels_device (cosine, normalised rows): the prepare pass and the launch, wall time;
  launch   the synchronous vh_op_propagate on operand rows of the same shape;
  match    one synchronous vh_match_patches_device on the same 64 x 7 (target, source) pairs: the yardstick, which keeps the top-1 only;
beside the FLOP floor measured in the same passes: 2 D flops per admitted (query, key) pair at the rate of the forward's fc2 GEMM
(vh_bench_gemm, ViT-B/16 at batch 512, the better of variants 5 and 6).  No threshold is asserted: the tool records what it sees.
Written to <out>/propagate_bench.txt.
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

FC2 = (512 * 197, 768, 3072)   # M, N, K
VIT_L14 = dict(image_size=224, patch_size=14, channels=3, dim=1024, heads=16, mlp_dim=4096, layers=24, classes=1000)
MODELS = [("ViT-B/16 bf16", S.CONFIGS["vit_base"], vithip.DTYPE_BF16, 512), ("ViT-L/14 fp16", VIT_L14, vithip.DTYPE_FP16, 256)]
NITEMS, NSRC, K, TAU, CLASSES, RADII = 64, 7, 5, 0.1, 8, (0, 4)


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return f"{statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]"


def admitted(g, radius):
    """The (query, key) pairs of one g x g source the window admits."""
    if radius == 0:
        return g ** 4
    y = np.arange(g)
    return int((np.minimum(y + radius, g - 1) - np.maximum(y - radius, 0) + 1).sum()) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("propagate_bench: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    items = np.array([[i + NSRC] + list(range(i, i + NSRC)) for i in range(NITEMS)], dtype=np.int32)
    pairs = np.array([[it[0], s] for it in items for s in it[1:]], dtype=np.int32)
    images = int(items.max()) + 1
    runs = []
    for name, cfg, dt, batch in MODELS:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
        ctx.load_weights(S.make_blob(cfg, 0))
        g, dim = cfg["image_size"] // cfg["patch_size"], cfg["dim"]
        npatch = g * g
        rng = np.random.default_rng(0)
        d_in = vithip.DeviceBuffer.from_numpy(S.make_images(cfg, 1, batch))
        d_logits = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        d_items, d_pairs = vithip.DeviceBuffer.from_numpy(items), vithip.DeviceBuffer.from_numpy(pairs)
        d_labels = vithip.DeviceBuffer.from_numpy(rng.random((batch, npatch, CLASSES), dtype=np.float32))
        d_out = vithip.DeviceBuffer(NITEMS * npatch * CLASSES * 4)
        d_idx, d_score = vithip.DeviceBuffer(len(pairs) * npatch * 4), vithip.DeviceBuffer(len(pairs) * npatch * 4)
        d_rows = vithip.DeviceBuffer.from_numpy(vithip.to16(rng.standard_normal((images * npatch, dim)).astype(np.float32) / np.sqrt(dim), dt))
        mdesc = vithip.MatchDesc(vithip.FEAT_NORM, -1, vithip.MATCH_COSINE, len(pairs))
        fns = {"step": lambda c=ctx, i=d_in, o=d_logits, b=batch: c.forward_device(i.ptr, b, o.ptr),
               "match": lambda c=ctx, d=mdesc, p=d_pairs, i=d_idx, s=d_score: c.match_patches_device(d, p.ptr, i.ptr, s.ptr)}
        for r in RADII:
            pdesc = vithip.PropagateDesc(vithip.FEAT_NORM, -1, vithip.MATCH_COSINE, NITEMS, NSRC, K, r, CLASSES, TAU, 0)
            fns[f"call r{r}"] = lambda c=ctx, d=pdesc, it=d_items, la=d_labels, o=d_out: c.propagate_labels_device(d, it.ptr, la.ptr, o.ptr)
            fns[f"launch r{r}"] = (lambda r=r, rows=d_rows, dt=dt, g=g, dim=dim, it=d_items, la=d_labels, o=d_out:
                                   vithip.op_propagate(rows.ptr, dt, images, g, g, dim, it.ptr, NITEMS, NSRC, K, r, TAU, la.ptr, CLASSES, o.ptr))
        runs.append((name, batch, g, dim, fns, {k: [] for k in fns}))
    for r in runs:   # warm-up: code objects, the dynamic-LDS attribute, the operand scratch
        for fn in r[4].values():
            fn()
    t_fc2 = []
    for _ in range(a.passes):
        for r in runs:
            for k, fn in r[4].items():
                r[5][k].append(wall_ms(fn))
        t_fc2.append(min(vithip.bench_gemm(*FC2, vithip.EPI_BIAS_RESID, vithip.DTYPE_BF16, v, 10) for v in (5, 6)))
    rate_f = 2.0 * FC2[0] * FC2[1] * FC2[2] / (statistics.median(t_fc2) * 1e-3)
    say(f"propagate_bench: {a.passes} interleaved passes, median [min .. max] ms; fc2 rate {rate_f / 1e12:.0f} TFLOP/s (median "
        f"{statistics.median(t_fc2):.3f} ms); {NITEMS} items, S {NSRC}, k {K}, tau {TAU}, {CLASSES} classes")
    for name, batch, g, dim, _, t in runs:
        m = {k: statistics.median(v) for k, v in t.items()}
        say(f"  {name} b{batch}, NP {g * g}, D {dim}:")
        say(f"    step       {med(t['step'])}")
        say(f"    match      {med(t['match'])}   {NITEMS * NSRC} pairs, top-1 only: the yardstick")
        for r in RADII:
            ff = 2.0 * NITEMS * NSRC * admitted(g, r) * dim / rate_f * 1e3
            say(f"    call r{r}    {med(t[f'call r{r}'])}   = {100 * m[f'call r{r}'] / m['step']:.2f} % of a step, {m[f'call r{r}'] / m['match']:.2f} x the match")
            say(f"    launch r{r}  {med(t[f'launch r{r}'])}   flop floor {ff:.4f} ({m[f'launch r{r}'] / ff:.1f} x)")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "propagate_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
