#!/usr/bin/env python3
"""Layer-feature measurements (run on the GPU box): what tapping four layers costs a forward, and what the channels-first read-out
costs beside the rows read-out followed by a permute pass.

  python tools/layer_features_bench.py [--out profiles] [--passes 7] [--steps 4] [--only NAME]

In ONE process, one context per model: ViT-B/16 bf16 at batch 512 (taps 3, 6, 9, 12) and ViT-L/14 fp16 at batch 256 (taps 5, 12, 18,
24).  `passes` interleaved passes of
  the forward with no list and with the list set (vh_forward_device_async, `steps` steps, wall time per step; the list is switched
  between the two, which drops no graph here: the forwards are eager),
  then, with the list set, the synchronous vh_read_layer_features_device of the normalised patch rows of an intermediate layer as
  bf16: VH_FEAT_ROWS, VH_FEAT_NCHW, and VH_FEAT_ROWS followed by torch's permute(0, 2, 1).contiguous() of the same tensor -- the
  pair the channels-first call replaces,
the median pass reported with min and max.  No threshold is asserted: the tool records what it sees.  Written to
<out>/layer_features.txt.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

VIT_L14 = dict(image_size=224, patch_size=14, channels=3, dim=1024, heads=16, mlp_dim=4096, layers=24, classes=1000)
MODELS = [("ViT-B/16 bf16 b512", S.CONFIGS["vit_base"], vithip.DTYPE_BF16, 512, [3, 6, 9, 12]),
          ("ViT-L/14 fp16 b256", VIT_L14, vithip.DTYPE_FP16, 256, [5, 12, 18, 24])]
READS = ["rows", "nchw", "rows + torch permute"]


def measure(name, cfg, dtype, batch, taps, passes, steps, say):
    import torch
    T, D = S.tokens(cfg), cfg["dim"]
    NP = T - 1
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch)
    ctx.init_weights_seeded(0)
    split = ctx.ln_fold()
    d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, d_in.ptr)
    rows_t = torch.empty((batch, NP, D), dtype=torch.bfloat16, device="cuda")
    nchw_t = torch.empty((batch, D, NP), dtype=torch.bfloat16, device="cuda")
    layer = taps[1]

    def desc(ptr, layout):
        return vithip.LayerFeatures(None, ptr, None, None, vithip.ELEM_BF16, vithip.FEAT_NORM, layer, layout)

    d_rows, d_nchw = desc(rows_t.data_ptr(), vithip.FEAT_ROWS), desc(nchw_t.data_ptr(), vithip.FEAT_NCHW)

    def step_ms():
        t0 = time.perf_counter()
        ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=steps)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def read(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "nchw":
            ctx.read_layer_features_device(d_nchw)
        else:
            ctx.read_layer_features_device(d_rows)
            if which != "rows":
                out = rows_t.permute(0, 2, 1).contiguous()
                torch.cuda.synchronize()
                del out
        return (time.perf_counter() - t0) * 1e3

    ctx.set_feature_layers(taps)
    step_ms()   # warm-up: the forward, the capture copy and every read-out once
    for r in READS:
        read(r)
    same = bool(torch.equal(rows_t.permute(0, 2, 1).contiguous(), nchw_t))
    plain, tapped, reads = [], [], {r: [] for r in READS}
    for _ in range(passes):
        ctx.set_feature_layers([])
        plain.append(step_ms())
        ctx.set_feature_layers(taps)
        tapped.append(step_ms())
        for r in READS:
            reads[r].append(read(r))
    med = statistics.median
    per_layer = batch * T * D * (3 if split else 4)
    say(f"{name}: T = {T}, D = {D}, residual rows as {'split planes (3 B / element)' if split else 'fp32'}; taps {taps}, "
        f"{per_layer / 1e6:.0f} MB per captured layer; {passes} interleaved passes, {steps} steps per pass")
    say(f"  forward step, no list   {med(plain):9.3f} ms median (min {min(plain):.3f}, max {max(plain):.3f})")
    say(f"  forward step, taps set  {med(tapped):9.3f} ms median (min {min(tapped):.3f}, max {max(tapped):.3f})  "
        f"{100 * (med(tapped) / med(plain) - 1):+5.2f} % of a step")
    for r in READS:
        say(f"  read layer {layer} patch bf16, {r:<22} {med(reads[r]):9.3f} ms median (min {min(reads[r]):.3f}, max {max(reads[r]):.3f})")
    say(f"  nchw == permute(rows): {same}")
    ctx.close()
    d_in.free()
    d_out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("layer features: wall time of a forward step with and without four tapped layers, and of the patch read-outs, same process")
    for name, cfg, dtype, batch, taps in MODELS:
        if not a.only or a.only in name:
            measure(name, cfg, dtype, batch, taps, a.passes, a.steps, say)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "layer_features.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
