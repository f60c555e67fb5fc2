#!/usr/bin/env python3
"""Embedding-search measurements (run on the GPU box): what the k best of a device-resident bank cost.

  python tools/search_bench.py [--out profiles] [--passes 7] [--rows 1281167]

In ONE process, bf16: a seeded bank of `rows` x 768 (ImageNet-train's size; integer-valued elements, generated and uploaded in chunks)
searched for the 20 best with 512 and with 16 query rows, and a zero-shot bank of 1 000 x 512 searched for the 5 best with 512 query
rows.  `passes` interleaved passes of the synchronous vh_op_search (the query image, the scan and the slab merge: three launches, wall
time of the call, launch and synchronisation overhead included), the median reported with min and max, beside two floors measured
in the same passes:
  bytes   the bank's bytes at the streaming rate of this run -- vh_op_cast over 2^28 elements, 4 bytes in and 2 out per element;
  flops   2 nq n W at the rate of the forward's fc2 GEMM (vh_bench_gemm, ViT-B/16 at batch 512, the better of variants 5 and 6).
No threshold is asserted: the tool records what it sees.  Written to <out>/search_bench.txt.
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

import vithip  # noqa: E402

DT = vithip.DTYPE_BF16
CAST_ELEMS = 1 << 28
FC2 = (512 * 197, 768, 3072)   # M, N, K


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def make_bank(n, w, seed):
    """[n][w] bf16 on the device: integers in -127 .. 127 (exact in bf16), uploaded 65 536 rows at a time."""
    rng = np.random.default_rng(seed)
    buf = vithip.DeviceBuffer(n * w * 2)
    for r0 in range(0, n, 65536):
        rows = min(65536, n - r0)
        bits = vithip.to16(rng.integers(-127, 128, (rows, w), dtype=np.int8).astype(np.float32), DT)
        vithip._check(vithip.lib().vh_memcpy_h2d(0, buf.ptr + r0 * w * 2, bits.ctypes.data, bits.nbytes))
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1281167)
    a = ap.parse_args()
    if vithip.device_count() < 1:
        raise SystemExit("search_bench: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    banks = {(a.rows, 768): make_bank(a.rows, 768, 1), (1000, 512): make_bank(1000, 512, 2)}
    shapes = [(a.rows, 768, 20, 512), (a.rows, 768, 20, 16), (1000, 512, 5, 512)]
    runs = []
    for n, w, k, nq in shapes:
        bufs = [vithip.DeviceBuffer.from_numpy(rng.standard_normal((nq, w)).astype(np.float32)),
                vithip.DeviceBuffer(vithip.op_search_workspace_bytes(nq, n, k)), vithip.DeviceBuffer(nq * k * 4), vithip.DeviceBuffer(nq * k * 4)]
        runs.append(((n, w, k, nq), bufs, lambda b=bufs, n=n, w=w, k=k, nq=nq: vithip.op_search(
            b[0].ptr, nq, w, 1, banks[(n, w)].ptr, n, DT, k, b[1].ptr, b[2].ptr, b[3].ptr)))
    c_in, c_out = vithip.DeviceBuffer(CAST_ELEMS * 4), vithip.DeviceBuffer(CAST_ELEMS * 2)

    def cast():
        vithip._check(vithip.lib().vh_op_cast(c_in.ptr, c_out.ptr, CAST_ELEMS, DT, None))

    t = {key: [] for key, _, _ in runs}
    t_cast, t_fc2 = [], []
    for _, _, fn in runs:   # warm-up: code objects, the dynamic-LDS attribute
        fn()
    cast()
    for _ in range(a.passes):
        for key, _, fn in runs:
            t[key].append(wall_ms(fn))
        t_cast.append(wall_ms(cast))
        t_fc2.append(min(vithip.bench_gemm(*FC2, vithip.EPI_BIAS_RESID, DT, v, 10) for v in (5, 6)))
    rate_b = CAST_ELEMS * 6 / (statistics.median(t_cast) * 1e-3)
    rate_f = 2.0 * FC2[0] * FC2[1] * FC2[2] / (statistics.median(t_fc2) * 1e-3)
    say(f"search_bench: bf16, {a.passes} interleaved passes, median [min .. max] ms; streaming rate {rate_b / 1e12:.2f} TB/s "
        f"(cast, median {statistics.median(t_cast):.3f} ms), fc2 rate {rate_f / 1e12:.0f} TFLOP/s (median {statistics.median(t_fc2):.3f} ms)")
    for n, w, k, nq in shapes:
        v = t[(n, w, k, nq)]
        med, fb, ff = statistics.median(v), n * w * 2 / rate_b * 1e3, 2.0 * nq * n * w / rate_f * 1e3
        say(f"  n {n:8d} W {w:4d} k {k:2d} nq {nq:4d} ({vithip.op_search_slabs(nq, n):3d} slabs): search {med:9.3f}  [{min(v):.3f} .. {max(v):.3f}]"
            f"  byte floor {fb:.3f} ({med / fb:.1f} x)  flop floor {ff:.3f} ({med / ff:.1f} x)")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "search_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
