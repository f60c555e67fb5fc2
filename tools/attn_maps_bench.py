#!/usr/bin/env python3
"""Attention-map measurements (run on the GPU box): what keeping the class token's softmax rows costs a forward, what the capture
launch costs on its own beside its memory floor, one read-out, and the accuracy of the hardware exp2 as seen through the tap.

  python tools/attn_maps_bench.py [--out profiles] [--passes 7] [--steps 4] [--only NAME]

In ONE process, one context per model: ViT-B/16 bf16 at batch 512 and ViT-L/14 fp16 at batch 256.  `passes` interleaved passes of
  the forward with no list, with the last layer listed and with every layer listed (VH_ATTN_Q_CLS; vh_forward_device_async, `steps`
  steps, wall time per step; the forwards are eager, so switching the list drops no graph),
  the capture kernel alone through vh_op_attention_probs on a q|k|v buffer of the model's shape, between two events on the stream,
  beside the floor of reading the K third of q|k|v once at 4.33 TB/s (the rate profiles/features.txt records for a feature read),
  one synchronous vh_read_attention_device of the last layer (fp32, all keys),
the median pass reported with min and max.  No threshold is asserted: the tool records what it sees.

exp2: tokens = 2, one head of 32 columns, Q = 1.  Key 0 scores 0, key 1 scores x = -i / 32, i = 0 .. 4032 (x = -(i // 32) - (i % 32) / 32
from two exact products), so p[1] / p[0] = exp2(x) up to the two divisions' roundings; the largest |p[1] / p[0] - 2^x| / 2^x against
float64 is recorded.  tests/test_gpu_attention_maps.py uses twice that value.  Written to <out>/attn_maps.txt.
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
FLOOR_TBS = 4.33


def exp2_sweep(say):
    n = 4033
    i = np.arange(n)
    qkv = np.zeros((n, 2, 3, 32), dtype=np.float32)
    qkv[:, 0, 0, 0], qkv[:, 0, 0, 1] = -1.0, -1.0 / 32
    qkv[:, 1, 1, 0], qkv[:, 1, 1, 1] = i // 32, i % 32
    x = -(i // 32) - (i % 32) / 32.0
    src = vithip.DeviceBuffer.from_numpy(vithip.to16(qkv.reshape(n * 2, 96), vithip.DTYPE_FP16))
    dst = vithip.DeviceBuffer(n * 2 * 4)
    vithip.op_attention_probs(src.ptr, n, 2, 1, 32, 1, vithip.DTYPE_FP16, dst.ptr)
    p = dst.to_numpy(np.float32, (n, 2)).astype(np.float64)
    rel = np.abs(p[:, 1] / p[:, 0] - np.exp2(x)) / np.exp2(x)
    w = int(np.argmax(rel))
    say(f"exp2 through the tap: {n} arguments -i/32 in [{x.min():.0f}, 0]: max |p1/p0 - 2^x| / 2^x = {rel.max():.3e} = 2^{np.log2(rel.max()):.2f} "
        f"at x = {float(x[w])!r} (the quotient's two division roundings included); exact at {int((rel == 0).sum())} arguments")
    src.free()
    dst.free()


def measure(name, cfg, dtype, batch, passes, steps, say):
    import torch
    T, D, H, L = S.tokens(cfg), cfg["dim"], cfg["heads"], cfg["layers"]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=batch)
    ctx.init_weights_seeded(0)
    d_in = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    d_out = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, batch, d_in.ptr)
    qkv_t = (torch.randn((batch * T, 3 * D), device="cuda") * 0.5).to(torch.bfloat16 if dtype == vithip.DTYPE_BF16 else torch.float16)
    probs_t = torch.empty((batch, H, 1, T), dtype=torch.float32, device="cuda")
    out_t = torch.empty((batch, H, 1, T), dtype=torch.float32, device="cuda")
    desc = vithip.AttentionMaps(out_t.data_ptr(), None, vithip.ELEM_F32, -1, vithip.ATTN_KEYS_ALL, 0)
    lists = {"no list": [], "last layer": [L], "all layers": list(range(1, L + 1))}

    def step_ms():
        t0 = time.perf_counter()
        ctx.forward_device_async(d_in.ptr, batch, d_out.ptr, steps=steps)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def capture_us():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        vithip.op_attention_probs(qkv_t.data_ptr(), batch, T, H, D // H, 1, dtype, probs_t.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def read_ms():
        t0 = time.perf_counter()
        ctx.read_attention_device(desc)
        return (time.perf_counter() - t0) * 1e3

    ctx.set_attention_layers(lists["all layers"])
    step_ms()   # warm-up: the forward, the capture, the read-out and the tap once
    read_ms()
    capture_us()
    step, cap, rd = {k: [] for k in lists}, [], []
    for _ in range(passes):
        for k, lst in lists.items():
            ctx.set_attention_layers(lst)
            step[k].append(step_ms())
        rd.append(read_ms())   # (every layer is listed here)
        cap.append(capture_us())
    med = statistics.median
    kbytes = batch * T * D * 2
    floor = kbytes / (FLOOR_TBS * 1e12) * 1e6
    say(f"{name}: T = {T}, D = {D}, {H} heads, {L} layers; store {batch * H * T * 4 / 1e6:.1f} MB per listed layer (Q = 1); "
        f"{passes} interleaved passes, {steps} steps per pass")
    base = med(step["no list"])
    for k in lists:
        extra = "" if k == "no list" else f"  {100 * (med(step[k]) / base - 1):+5.2f} % of a step, {(med(step[k]) - base) * 1e3 / len(lists[k]):+7.1f} us per listed layer"
        say(f"  forward step, {k:<11} {med(step[k]):9.3f} ms median (min {min(step[k]):.3f}, max {max(step[k]):.3f}){extra}")
    say(f"  capture launch alone (tap, events) {med(cap):8.1f} us median (min {min(cap):.1f}, max {max(cap):.1f}); K is {kbytes / 1e6:.0f} MB: "
        f"floor {floor:.1f} us at {FLOOR_TBS} TB/s, so {kbytes / med(cap) / 1e6:.2f} TB/s of K")
    say(f"  read last layer, fp32, all keys    {med(rd):8.3f} ms median (min {min(rd):.3f}, max {max(rd):.3f})")
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

    say("attention maps: wall time of a forward step with no, one and all layers listed, the capture launch alone, one read-out; same process")
    for name, cfg, dtype, batch in MODELS:
        if not a.only or a.only in name:
            measure(name, cfg, dtype, batch, a.passes, a.steps, say)
    if not a.only or a.only == "exp2":
        exp2_sweep(say)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "attn_maps.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
