#!/usr/bin/env python3
"""SigLIP measurements (run on the GPU box): what VH_FLAG_TANH_GELU and VH_FLAG_MAP_HEAD cost.

  python tools/siglip_bench.py [--out profiles] [--steps 20]

For SigLIP-B/16-224 (196 tokens, D 768, H 12, M 3072) at batch 512 and the L/16-256 shape (256 tokens, D 1024, H 16, M 4096) at batch
256, in bf16, fp16 and fp8, in ONE process with interleaved passes (A, B, A, B, so that both see the same box and clock) and medians:
  (1) the step: A = NO_CLS | MAP_HEAD | TANH_GELU (SiglipVisionModel) against B = NO_CLS | POOL(AVG_NORM) with erf GELU, the same
      backbone with the mean-pooled head (forward_device_async with step timing);
  (2) fc1 per launch, tanh against erf (hip events around the stage's launches);
  (3) the final-LayerNorm stage of a profiled forward: for A the MAP head's total (map_pool_kernel + the six [batch]-row launches), for
      B pool_rows_kernel alone;
  (4) map_pool_kernel against pool_rows_kernel on the same planes through their taps: host time of `calls` synchronous calls each,
      interleaved, median per call -- both carry the same launch + synchronise overhead, so the DIFFERENCE is the kernels'.
The shapes are defined here: vh_synth.CONFIGS is shared by the test suite and bench.py.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vithip  # noqa: E402

DT = {"bf16": vithip.DTYPE_BF16, "fp16": vithip.DTYPE_FP16, "fp8": vithip.DTYPE_FP8}
SIGLIP = vithip.FLAG_NO_CLS | vithip.FLAG_MAP_HEAD | vithip.FLAG_TANH_GELU
BASE = vithip.FLAG_NO_CLS | vithip.FLAG_POOL(vithip.POOL_AVG_NORM)


def _cfg(image, dim, heads, mlp, layers):
    return dict(image_size=image, patch_size=16, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=dim)


RUNS = [("SigLIP-B/16-224", _cfg(224, 768, 12, 3072, 12), 512), ("SigLIP-L/16-256", _cfg(256, 1024, 16, 4096, 24), 256)]


class Run:
    def __init__(self, cfg, dname, batch, flags):
        self.cfg, self.batch = cfg, batch
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=1e-6)
        self.ctx.init_weights_seeded(0)
        self.din = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4)
        self.dout = vithip.DeviceBuffer(batch * cfg["classes"] * 4)
        self.ctx.fill_input_seeded(1, batch, self.din.ptr)
        self.ctx.forward_device_async(self.din.ptr, batch, self.dout.ptr, steps=5)   # warm-up
        self.ctx.synchronize()

    def steps(self, n):
        self.ctx.set_step_timing(True)
        self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps=n)
        self.ctx.synchronize()
        st = np.array(self.ctx.get_step_timing())
        self.ctx.set_step_timing(False)
        return st

    def stage(self, name, n):
        self.ctx.set_stage_timing(name)
        self.ctx.forward_device_async(self.din.ptr, self.batch, self.dout.ptr, steps=n)
        self.ctx.synchronize()
        avg_ms, min_ms, launches = self.ctx.get_stage_timing()
        self.ctx.set_stage_timing(None)
        return avg_ms, min_ms, launches

    def head_ms(self):
        return self.ctx.profile_forward(self.din.ptr, self.batch, self.dout.ptr)["final_layernorm"][0]

    def close(self):
        finite = bool(np.isfinite(self.dout.to_numpy(np.float32, (self.batch, self.cfg["classes"]))).all())
        self.ctx.close(); self.din.free(); self.dout.free()
        return finite


def taps(cfg, batch, dname, calls, log):
    """map_pool_kernel against pool_rows_kernel on the same planes (the form the dtype's split path keeps), through the taps."""
    D, H = cfg["dim"], cfg["heads"]
    T = (cfg["image_size"] // cfg["patch_size"]) ** 2
    rng = np.random.default_rng(0)
    form = DT[dname]
    hi_b, lo_b = (1, 2) if dname == "fp8" else (2, 1)
    n = batch * T * D
    hi = vithip.DeviceBuffer.from_numpy(rng.integers(0x30, 0x3F, n * hi_b, dtype=np.uint8))     # (finite, moderate values in every form)
    lo = vithip.DeviceBuffer.from_numpy(rng.integers(0x30, 0x3F, n * lo_b, dtype=np.uint8))
    gamma = vithip.DeviceBuffer.from_numpy(np.ones(D, np.float32))
    beta = vithip.DeviceBuffer.from_numpy(np.zeros(D, np.float32))
    qk = vithip.DeviceBuffer.from_numpy((rng.standard_normal((H, D)) * (2.0 / np.sqrt(D))).astype(np.float32))
    z, mean = vithip.DeviceBuffer(batch * H * D * 4), vithip.DeviceBuffer(batch * D * 4)
    f_map = lambda: vithip.op_map_pool(hi.ptr, lo.ptr, form, batch, T, 0, D, gamma.ptr, beta.ptr, 1e-6, qk.ptr, H, z.ptr)
    f_pool = lambda: vithip.op_pool_rows(hi.ptr, lo.ptr, form, batch, T, 0, D, gamma.ptr, beta.ptr, 1e-6, vithip.FEAT_NORM, mean.ptr)
    for f in (f_map, f_pool, f_map, f_pool):
        f()
    tm, tp = [], []
    for _ in range(calls):
        for f, acc in ((f_map, tm), (f_pool, tp)):
            t0 = time.perf_counter()
            f()
            acc.append((time.perf_counter() - t0) * 1e3)
    finite = bool(np.isfinite(z.to_numpy(np.float32, (batch * H * D,))).all())
    for b in (hi, lo, gamma, beta, qk, z, mean):
        b.free()
    m, p = float(np.median(tm)), float(np.median(tp))
    mb = n * 3 / 1e6
    log(f"    taps, {mb:.0f} MB of planes, {calls} calls each, host time per synchronous call: map_pool {m:.3f} ms median ({min(tm):.3f} min) | "
        f"pool_rows {p:.3f} ms ({min(tp):.3f} min) | difference {m - p:+.3f} ms | z finite {finite}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--dtypes", default="bf16,fp16,fp8")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"siglip_bench: {a.steps} timed steps per pass, two interleaved passes per context (A B A B); A = NO_CLS | MAP_HEAD | TANH_GELU, "
        "B = NO_CLS | POOL(AVG_NORM), erf GELU")
    for model, cfg, batch in RUNS:
        for dname in a.dtypes.split(","):
            A, B = Run(cfg, dname, batch, SIGLIP), Run(cfg, dname, batch, BASE)
            sa, sb = [], []
            for _ in range(2):
                sa.append(A.steps(a.steps)); sb.append(B.steps(a.steps))
            sa, sb = np.concatenate(sa), np.concatenate(sb)
            f1 = [(A.stage("fc1_gemm", 4), B.stage("fc1_gemm", 4)) for _ in range(2)]
            ha, hb = [], []
            for _ in range(5):
                ha.append(A.head_ms()); hb.append(B.head_ms())
            ma, mb = float(np.median(sa)), float(np.median(sb))
            ok = A.close() and B.close()
            T = (cfg["image_size"] // 16) ** 2
            log(f"{model} T={T} b{batch} {dname}: SigLIP {ma:.3f} ms median ({sa.min():.3f} min) = {batch / ma * 1e3:.0f} images/s | mean-pool + erf "
                f"{mb:.3f} ms ({sb.min():.3f} min) = {batch / mb * 1e3:.0f} images/s | ratio {ma / mb:.4f} | logits finite {ok}")
            t_us = [p[0][0] * 1e3 for p in f1]
            e_us = [p[1][0] * 1e3 for p in f1]
            log(f"    fc1 per launch ({f1[0][0][2]} launches): tanh {np.mean(t_us):.1f} us avg ({min(p[0][1] for p in f1) * 1e3:.1f} min) | erf "
                f"{np.mean(e_us):.1f} us avg ({min(p[1][1] for p in f1) * 1e3:.1f} min) | ratio {np.mean(t_us) / np.mean(e_us):.4f} | passes "
                f"{t_us[0]:.1f} {t_us[1]:.1f} / {e_us[0]:.1f} {e_us[1]:.1f}")
            log(f"    final-LayerNorm stage of a profiled forward, median of 5: MAP head total {np.median(ha):.3f} ms ({min(ha):.3f} min) | "
                f"pool_rows {np.median(hb):.3f} ms ({min(hb):.3f} min) | MAP head = {100 * np.median(ha) / ma:.2f} % of its step")
            taps(cfg, batch, dname, a.calls, log)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "siglip_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
