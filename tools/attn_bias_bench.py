#!/usr/bin/env python3
"""Attention with an additive per-head bias (VH_FLAG_ATTN_BIAS) measured on one MI355X -> profiles/attn_bias_bench.txt.

One process, interleaved passes, medians:
  1. the step of BEiT-B/16-224 (batch 256) and BEiT-L/16-224 (batch 128), bf16 and fp16, with the flag against the same context shape
     without it (seeded weights; images/s of vh_forward_device_async steps);
  2. the biased kernel per launch against vh_op_attention_hd at equal shape, with the bytes of bias image a launch reads;
  3. the two grid orders of the biased launcher (VH_ATTN_BIAS_ORDER, read at each launch) at 197 and 1025 tokens.
Usage: python tools/attn_bias_bench.py [--passes 7] [--quick]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
import vithip  # noqa: E402

BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
NAME = {BF16: "bf16", FP16: "fp16"}
MODELS = {"BEiT-B/16-224": (dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=1000), 256),
          "BEiT-L/16-224": (dict(image_size=224, patch_size=16, channels=3, dim=1024, heads=16, mlp_dim=4096, layers=24, classes=1000), 128)}


def timed(fn, reps):
    vithip.lib().vh_device_synchronize(0)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    vithip.lib().vh_device_synchronize(0)
    return (time.perf_counter() - t0) / reps


def interleaved(fns, passes, reps):
    """median seconds per call of every fn, the fns taking turns inside each pass"""
    for fn in fns:
        timed(fn, 3)
    t = [[] for _ in fns]
    for _ in range(passes):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, reps))
    return [statistics.median(x) for x in t]


def model_steps(out, passes):
    pool = vithip.FLAG_POOL(vithip.POOL_AVG_FCNORM)
    for name, (cfg, batch) in MODELS.items():
        for dt in (BF16, FP16):
            ctxs = []
            for flags in (pool | vithip.FLAG_ATTN_BIAS, pool):
                c = vithip.VitContext(cfg, dtype=dt, max_batch=batch, flags=flags)
                c.init_weights_seeded(1)
                ctxs.append(c)
            images = np.zeros((batch, cfg["image_size"], cfg["image_size"], 3), np.float32)
            x = vithip.DeviceBuffer.from_numpy(images)
            y = vithip.DeviceBuffer.from_numpy(np.zeros((batch, cfg["classes"]), np.float32))
            fns = [lambda c=c: c.forward_device(x.ptr, batch, y.ptr) for c in ctxs]
            on, off = interleaved(fns, passes, 5)
            out(f"{name} {NAME[dt]} b{batch}: with the flag {batch / on:9.1f} images/s, without {batch / off:9.1f} images/s (ratio {off / on:.3f})")
            for c in ctxs:
                c.close()


def kernel_launches(out, passes):
    for tokens, batch, heads, hd in ((197, 256, 12, 64), (197, 128, 16, 64), (1025, 8, 16, 64), (197, 128, 16, 80), (1025, 8, 16, 128)):
        for dt in (BF16, FP16):
            D = heads * hd
            qkv = vithip.DeviceBuffer.from_numpy(vithip.to16((np.random.default_rng(0).standard_normal((batch * tokens, 3 * D)) * 0.5).astype(np.float32), dt))
            o = vithip.DeviceBuffer.from_numpy(np.zeros((batch * tokens, D), np.uint16))
            bias = vithip.DeviceBuffer.from_numpy(np.random.default_rng(1).standard_normal((heads, tokens, tokens)).astype(np.float32))
            nbytes = vithip.attention_bias_image_bytes(heads, tokens)
            img = vithip.DeviceBuffer.from_numpy(np.zeros(nbytes, np.uint8))
            vithip.op_attention_bias_image(bias.ptr, heads, tokens, img.ptr)

            def biased(order):
                def f():
                    os.environ["VH_ATTN_BIAS_ORDER"] = order
                    vithip.op_attention_bias(qkv.ptr, batch, tokens, heads, hd, img.ptr, o.ptr, dt)
                return f
            plain = lambda: vithip.op_attention_hd(qkv.ptr, batch, tokens, heads, hd, o.ptr, dt)
            t1, t0, tp = interleaved([biased("1"), biased("0"), plain], passes, 10)
            io = batch * tokens * 4 * D * 2
            out(f"T {tokens:4d} b{batch:3d} H{heads} hd{hd:3d} {NAME[dt]}: biased {t1 * 1e6:7.1f} us (images of a head neighbours) / {t0 * 1e6:7.1f} us (unbiased order), "
                f"vh_op_attention_hd {tp * 1e6:7.1f} us; ratio {t1 / tp:.3f}; bias image {nbytes / 2**20:.1f} MiB beside {io / 2**20:.1f} MiB of q|k|v + out")
    os.environ.pop("VH_ATTN_BIAS_ORDER", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="kernel launches only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_bias_bench.txt"))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("Attention bias on one MI355X: medians of interleaved passes in one process (tools/attn_bias_bench.py; the taps synchronise, so a")
    out("launch's time includes one host round trip, the same for both kernels).")
    kernel_launches(out, a.passes)
    if not a.quick:
        model_steps(out, a.passes)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
