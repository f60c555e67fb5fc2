#!/usr/bin/env python3
"""Generate tests/golden/attn_stream/stream64_parent.npz -- the stored bytes of the 64-wide K/V-streaming attention kernel as it
stood in its own source file, before head dim 64 became an instantiation of the kernel of kernels_attn_hd.hip.  The merged
kernel has to reproduce them bit for bit (test_gpu_head_dim.py).

Run on the GPU with the library of the commit before the merge:

    VITHIP_LIB=<that commit's libvithip.so> python tests/golden/make_golden_attn_stream.py [--out DIR]

Inputs are test_gpu_head_dim.make_qkv(batch, tokens, heads, 64, dtype, SEED); outputs are what vh_op_attention_stream stored for
bf16, fp16 and bf16 -> e4m3 ("fp8").  Each case (tokens, batch, heads) is the smallest that reaches one code path:

    (1, 2, 3)      one tile that is both first and tail; one wave
    (33, 2, 3)     two tiles; two waves share the four DMA pieces
    (97, 2, 3)     four tiles: the three-slot ring wraps; four DMA waves
    (289, 1, 2)    ten query blocks: two slabs
    (641, 1, 2)    the first count the dispatcher streams
    (1025, 1, 2)   many slabs                    (SHA-256 of the output only)
    (4097, 1, 2)   the longest sequence          (SHA-256 of the output only)

The file keeps, per dtype and case, the SHA-256 of the converted input bytes (a drifting generator is noticed before any output
is compared) and of the output bytes, and the output arrays of the first five cases.
"""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import vithip
from test_gpu_head_dim import make_qkv

SEED = 34
CASES = [(1, 2, 3), (33, 2, 3), (97, 2, 3), (289, 1, 2), (641, 1, 2), (1025, 1, 2), (4097, 1, 2)]   # (tokens, batch, heads)
STORED = 5                                                                                            # the first cases keep their arrays
DTYPES = [("bf16", vithip.DTYPE_BF16, vithip.DTYPE_BF16), ("fp16", vithip.DTYPE_FP16, vithip.DTYPE_FP16),
          ("fp8", vithip.DTYPE_BF16, vithip.DTYPE_FP8)]                                               # (name, input, launch dtype)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "attn_stream"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    out = dict(seed=np.array([SEED], dtype=np.int64), cases=np.array(CASES, dtype=np.int64), stored=np.array([STORED], dtype=np.int64))
    for name, din, dt in DTYPES:
        in_sha, out_sha = [], []
        for i, (tokens, batch, heads) in enumerate(CASES):
            pre, _ = make_qkv(batch, tokens, heads, 64, din, SEED)
            bits = vithip.to16(pre, din)
            qkv = vithip.DeviceBuffer.from_numpy(bits)
            n = batch * tokens * heads * 64
            width = 1 if dt == vithip.DTYPE_FP8 else 2
            o = vithip.DeviceBuffer.from_numpy(np.full(n * width, 0xFF, dtype=np.uint8))
            vithip.op_attention_stream(qkv.ptr, batch, tokens, heads, o.ptr, dt)
            got = o.to_numpy(np.uint8 if width == 1 else np.uint16, (batch * tokens, heads * 64))
            qkv.free(); o.free()
            in_sha.append(sha(bits))
            out_sha.append(sha(got))
            if i < STORED:
                out[f"out_{name}_{tokens}"] = got
            print(name, (tokens, batch, heads), "in", in_sha[-1][:16], "out", out_sha[-1][:16])
        out[f"in_sha256_{name}"] = np.array(in_sha)
        out[f"out_sha256_{name}"] = np.array(out_sha)
    path = os.path.join(a.out, "stream64_parent.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
