#!/usr/bin/env python3
"""Long-sequence measurements (run on the GPU box): models beyond 640 tokens, where attention runs the K/V-streaming kernel.

  python tools/long_seq_bench.py [--out profiles] [--steps 20] [--pairs 10] [--parity 16] [--skip-forward] [--skip-tap]

  (1) whole forward, ViT-B/16 at 448x448 (785 tokens) and 512x512 (1025), bf16 and fp16, batch 64: forward_device_async
      with step timing (device time per step), images/s;
  (2) the attention stage of the same forwards (hip events around every attention launch), and its share of the 2.5 PF
      16-bit peak for the algorithmic 4 T^2 D FLOP per image and layer;
  (3) the streaming tap against the resident ring at 577 tokens on the ViT-L/16-384 shape (fp16, batch 256, 16 heads), in
      interleaved pairs, host clock around each synchronising call (kernel-only times: run this part under
      rocprofv3 --kernel-trace --stats);
  (4) --parity N: ViT-B/16-512 fp16 on N seeded images against the CPU oracle, per-image max|d| / max|ref|.
The long-sequence models are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vh_synth as S  # noqa: E402
import vithip  # noqa: E402

PEAK_16 = 2.5e15   # MI355X dense 16-bit MFMA peak, FLOP/s


def vit_b16(image):
    return dict(image_size=image, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=1000)


def forward_rows(steps, batch, log):
    rows = []
    for image in (448, 512):
        cfg = vit_b16(image)
        T, D = S.tokens(cfg), cfg["dim"]
        for dname, dt in (("bf16", vithip.DTYPE_BF16), ("fp16", vithip.DTYPE_FP16)):
            ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch)
            ctx.init_weights_seeded(0)
            din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
            dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
            ctx.fill_input_seeded(1, batch, din.ptr)
            ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=3)   # warm-up
            ctx.synchronize()
            ctx.set_step_timing(True)
            ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=steps)
            ctx.synchronize()
            st = np.array(ctx.get_step_timing())
            ctx.set_step_timing(False)
            ctx.set_stage_timing("attention")
            ctx.forward_device_async(din.ptr, batch, dout.ptr, steps=max(2, steps // 4))
            ctx.synchronize()
            avg_ms, min_ms, n = ctx.get_stage_timing()
            ctx.set_stage_timing(None)
            logits = dout.to_numpy(np.float32, (batch, cfg["classes"]))
            ctx.close(); din.free(); dout.free()
            flop = 4.0 * T * T * D * batch
            r = dict(model=f"ViT-B/16-{image}", tokens=T, dtype=dname, batch=batch, steps=len(st),
                     step_ms_median=float(np.median(st)), step_ms_min=float(st.min()),
                     images_per_s=batch / (float(np.median(st)) * 1e-3),
                     attention_us_avg=avg_ms * 1e3, attention_us_min=min_ms * 1e3, attention_launches=n,
                     attention_peak_fraction=flop / (avg_ms * 1e-3) / PEAK_16, logits_finite=bool(np.isfinite(logits).all()))
            rows.append(r)
            log(f"forward {r['model']} T={T} {dname} b{batch}: step {r['step_ms_median']:.3f} ms median ({r['step_ms_min']:.3f} min, "
                f"{len(st)} steps) = {r['images_per_s']:.0f} images/s; attention {r['attention_us_avg']:.1f} us avg "
                f"({r['attention_us_min']:.1f} min, {n} launches) = {r['attention_peak_fraction']:.3f} of {PEAK_16 / 1e15:.1f} PF")
    return rows


def tap_pairs(pairs, log):
    batch, T, H, dt = 256, 577, 16, vithip.DTYPE_FP16
    D = H * 64
    n_el = batch * T * 3 * D
    f32 = vithip.DeviceBuffer(n_el * 4)
    vithip.op_fill(f32.ptr, n_el, 7, 1, 0, 1.0)   # uniform [-1, 1): exp2-domain scores of a few units, as in a ViT
    qkv = vithip.DeviceBuffer(n_el * 2)
    vithip.op_cast(f32.ptr, qkv.ptr, n_el, dt)
    f32.free()
    out_r, out_s = vithip.DeviceBuffer(batch * T * D * 2), vithip.DeviceBuffer(batch * T * D * 2)

    def timed(fn, out):   # host clock around one synchronising call
        t0 = time.perf_counter()
        fn(qkv.ptr, batch, T, H, out.ptr, dt)
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):   # warm-up (first launches set kernel attributes)
        timed(vithip.op_attention, out_r); timed(vithip.op_attention_stream, out_s)
    ring, stream = [], []
    for i in range(pairs):   # interleaved, alternating which goes first
        if i % 2 == 0:
            ring.append(timed(vithip.op_attention, out_r)); stream.append(timed(vithip.op_attention_stream, out_s))
        else:
            stream.append(timed(vithip.op_attention_stream, out_s)); ring.append(timed(vithip.op_attention, out_r))
    a = vithip.from16(out_r.to_numpy(np.uint16, (batch * T, D)), dt)
    b = vithip.from16(out_s.to_numpy(np.uint16, (batch * T, D)), dt)
    diff = float(np.abs(a - b).max() / np.abs(a).max())
    qkv.free(); out_r.free(); out_s.free()
    ring, stream = np.array(ring), np.array(stream)
    flop = 4.0 * T * T * D * batch
    r = dict(shape=f"ViT-L/16-384 attention: batch {batch}, {T} tokens, {H} heads, fp16", pairs=pairs, clock="host, per synchronising call",
             ring_us_median=float(np.median(ring)), ring_us_min=float(ring.min()),
             stream_us_median=float(np.median(stream)), stream_us_min=float(stream.min()),
             ratio_median=float(np.median(stream / ring)),
             ring_peak_fraction=flop / (np.median(ring) * 1e-6) / PEAK_16,
             stream_peak_fraction=flop / (np.median(stream) * 1e-6) / PEAK_16, max_rel_diff=diff)
    log(f"tap T={T} b{batch} H={H} fp16, {pairs} interleaved pairs, host clock per call (kernel + launch + synchronisation; the "
        f"resident tap also allocates and zeroes its counter): resident ring {r['ring_us_median']:.1f} us median "
        f"({r['ring_us_min']:.1f} min, {r['ring_peak_fraction']:.3f} of peak), stream {r['stream_us_median']:.1f} us median "
        f"({r['stream_us_min']:.1f} min, {r['stream_peak_fraction']:.3f} of peak); stream / ring {r['ratio_median']:.3f} "
        f"(median of the pair ratios); outputs differ by {diff:.2e} (max|d| / max|ring|)")
    return r


def parity(n, log):
    import oracle_lib as O
    cfg = vit_b16(512)
    blob, images = S.make_blob(cfg, 0), S.make_images(cfg, 1, n)
    t = time.time()
    ref = O.vit_forward(cfg, blob, images)
    t_ref = time.time() - t
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_FP16, max_batch=n)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    ctx.close()
    per = np.abs(got - ref).max(1) / np.abs(ref).max()
    r = dict(model="ViT-B/16-512", dtype="fp16", images=n, seeds="make_blob(cfg, 0), make_images(cfg, 1, n)",
             per_image=[float(x) for x in per], median=float(np.median(per)), worst=float(per.max()),
             inside_1e3=int((per <= 1e-3).sum()), first4_worst=float(per[:4].max()), first4_median=float(np.median(per[:4])))
    log(f"parity ViT-B/16-512 fp16, {n} images vs the CPU oracle ({t_ref:.0f} s): median {r['median']:.3e}, worst {r['worst']:.3e}, "
        f"{r['inside_1e3']} of {n} inside 1e-3; the first 4 (the test's images): median {r['first4_median']:.3e}, worst {r['first4_worst']:.3e}")
    log("per image: " + " ".join(f"{x:.3e}" for x in per))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="long_seq")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--parity", type=int, default=0, help="images of the ViT-B/16-512 fp16 parity sample (0: skip)")
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-tap", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def log(msg):
        print(msg, flush=True)
        lines.append(msg)

    res = {}
    if not a.skip_forward:
        res["forward"] = forward_rows(a.steps, a.batch, log)
    if not a.skip_tap:
        res["tap_577"] = tap_pairs(a.pairs, log)
    if a.parity:
        res["parity"] = parity(a.parity, log)
        with open(os.path.join(a.out, "long_seq_vit_b16_512_parity.txt"), "w") as f:
            f.write("\n".join(l for l in lines if l.startswith("parity") or l.startswith("per image")) + "\n")
    with open(os.path.join(a.out, f"{a.tag}_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, f"{a.tag}_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
