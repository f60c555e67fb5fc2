#!/usr/bin/env python3
"""Dense-correspondence measurements (run on the GPU box): what matching the patches of image pairs costs beside the forward.

  python tools/match_bench.py [--out profiles] [--passes 7]

In ONE process, one context per model, synthetic weights and images: ViT-B/16 bf16 at batch 512 with 256 pairs, ViT-L/14 fp16 at batch
256 with 128 pairs (pair p = images 2 p and 2 p + 1).  `passes` interleaved passes, the median reported with min and max, of
  step     one synchronous forward (device buffers), wall time;
  call     one synchronous vh_match_patches_device (cosine, normalised rows): the prepare pass and the match launch, wall time, launch
           and synchronisation overhead included;
  launch   the synchronous vh_op_match on operand rows of the same shape, with 64 and with 128 query rows per workgroup (VH_MATCH_QB);
           the prepare pass is reported as call - the launch the call's own choice makes;
beside two floors measured in the same passes:
  flops    2 npairs NP^2 D at the rate of the forward's fc2 GEMM (vh_bench_gemm, ViT-B/16 at batch 512, the better of variants 5 and 6);
  bytes    the prepare pass's bytes (batch NP D elements: the residual's bytes in, 2 out) at the streaming rate of this run -- vh_op_cast
           over 2^28 elements, 4 bytes in and 2 out per element.
No threshold is asserted: the tool records what it sees.  Written to <out>/match_bench.txt.
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

CAST_ELEMS = 1 << 28
FC2 = (512 * 197, 768, 3072)   # M, N, K
VIT_L14 = dict(image_size=224, patch_size=14, channels=3, dim=1024, heads=16, mlp_dim=4096, layers=24, classes=1000)
MODELS = [("ViT-B/16 bf16", S.CONFIGS["vit_base"], vithip.DTYPE_BF16, 512, 256), ("ViT-L/14 fp16", VIT_L14, vithip.DTYPE_FP16, 256, 128)]


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return f"{statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("match_bench: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    runs = []
    for name, cfg, dt, batch, npairs in MODELS:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
        ctx.load_weights(S.make_blob(cfg, 0))
        npatch, dim = (cfg["image_size"] // cfg["patch_size"]) ** 2, cfg["dim"]
        d_in = vithip.DeviceBuffer.from_numpy(S.make_images(cfg, 1, batch))
        d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        d_pairs = vithip.DeviceBuffer.from_numpy(np.arange(2 * npairs, dtype=np.int32))
        d_idx, d_score = vithip.DeviceBuffer(npairs * npatch * 4), vithip.DeviceBuffer(npairs * npatch * 4)
        rows = vithip.to16(np.random.default_rng(0).standard_normal((2 * npairs * npatch, dim)).astype(np.float32) / np.sqrt(dim), dt)
        d_rows = vithip.DeviceBuffer.from_numpy(rows)
        desc = vithip.MatchDesc(vithip.FEAT_NORM, -1, vithip.MATCH_COSINE, npairs)
        half = npairs * npatch * dim * 2   # bytes: the A rows, then the B rows

        def launch(qb, r=d_rows, half=half, dt=dt, npairs=npairs, npatch=npatch, dim=dim, i=d_idx, s=d_score):
            os.environ["VH_MATCH_QB"] = str(qb)
            vithip.op_match(r.ptr, r.ptr + half, dt, npairs, npatch, npatch, dim, vithip.MATCH_COSINE, i.ptr, s.ptr)
            del os.environ["VH_MATCH_QB"]
        fns = {"step": lambda c=ctx, i=d_in, o=d_out, b=batch: c.forward_device(i.ptr, b, o.ptr),
               "call": lambda c=ctx, d=desc, p=d_pairs, i=d_idx, s=d_score: c.match_patches_device(d, p.ptr, i.ptr, s.ptr),
               "launch64": lambda f=launch: f(64), "launch128": lambda f=launch: f(128)}
        runs.append((name, cfg, batch, npairs, npatch, dim, fns, {k: [] for k in fns}, ctx.ln_fold()))
    c_in, c_out = vithip.DeviceBuffer(CAST_ELEMS * 4), vithip.DeviceBuffer(CAST_ELEMS * 2)

    def cast():
        vithip._check(vithip.lib().vh_op_cast(c_in.ptr, c_out.ptr, CAST_ELEMS, vithip.DTYPE_BF16, None))

    for r in runs:   # warm-up: code objects, the dynamic-LDS attribute, the operand scratch
        for fn in r[6].values():
            fn()
    cast()
    t_cast, t_fc2 = [], []
    for _ in range(a.passes):
        for r in runs:
            for k, fn in r[6].items():
                r[7][k].append(wall_ms(fn))
        t_cast.append(wall_ms(cast))
        t_fc2.append(min(vithip.bench_gemm(*FC2, vithip.EPI_BIAS_RESID, vithip.DTYPE_BF16, v, 10) for v in (5, 6)))
    rate_b = CAST_ELEMS * 6 / (statistics.median(t_cast) * 1e-3)
    rate_f = 2.0 * FC2[0] * FC2[1] * FC2[2] / (statistics.median(t_fc2) * 1e-3)
    say(f"match_bench: {a.passes} interleaved passes, median [min .. max] ms; streaming rate {rate_b / 1e12:.2f} TB/s (cast, median "
        f"{statistics.median(t_cast):.3f} ms), fc2 rate {rate_f / 1e12:.0f} TFLOP/s (median {statistics.median(t_fc2):.3f} ms)")
    for name, cfg, batch, npairs, npatch, dim, _, t, fold in runs:
        qb = 128 if npairs * ((npatch + 127) // 128) >= 256 and npatch > 64 else 64   # match_query_rows (kernels_match.hip)
        m = {k: statistics.median(v) for k, v in t.items()}
        ff = 2.0 * npairs * npatch * npatch * dim / rate_f * 1e3
        fb = batch * npatch * dim * ((3 if fold else 4) + 2) / rate_b * 1e3
        prep = m["call"] - m[f"launch{qb}"]
        say(f"  {name} b{batch}, {npairs} pairs, NP {npatch}, D {dim} ({'split planes' if fold else 'fp32 rows'}):")
        say(f"    step      {med(t['step'])}")
        say(f"    call      {med(t['call'])}   = {100 * m['call'] / m['step']:.2f} % of a step")
        say(f"    launch64  {med(t['launch64'])}   flop floor {ff:.4f} ({m['launch64'] / ff:.1f} x)")
        say(f"    launch128 {med(t['launch128'])}   flop floor {ff:.4f} ({m['launch128'] / ff:.1f} x)   the launcher picks {qb}")
        say(f"    prepare   {prep:8.3f} (call - launch{qb})   byte floor {fb:.4f} ({prep / fb:.1f} x)")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "match_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
