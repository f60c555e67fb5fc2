#!/usr/bin/env python3
"""LDS bank arithmetic of gather_nchw_kernel (vit-fpga_amd/csrc/kernels_gather.hip), on the host: no device needed.

The build phase reads one source element per lane and instruction (ds_read_u8 / u16 / b32): 32 banks of one dword, two groups
of 32 lanes per wave, lanes of a group that hit one bank at DIFFERENT dword addresses serialise (the same dword is one access).
For every read instruction of a strip this prints the worst and the mean number of LDS cycles per 32-lane group (1 = free of
conflicts) for the row pitch the launch chooses (16 mod 32 bytes) and, beside it, for the unpadded pitch.

    tools/gather_lds_banks.py [--image 224 --patch 16 --channels 3 --kpad 768]
"""
import argparse
from collections import defaultdict

BUDGET, THREADS = 32 * 1024, 256


def strip_pitch(npx, patch, esz, padded=True):
    w = (npx * patch * esz + 15) // 16 * 16
    return w + 16 if padded and w % 32 == 0 else w


def choose_npx(image, patch, ch, esz):
    g, npx = image // patch, image // patch
    while npx > 1 and patch * ch * strip_pitch(npx, patch, esz) > BUDGET:
        npx = (npx + 1) // 2
    return npx


def build_cycles(image, patch, ch, kpad, esz, pitch, npx):
    """(worst, mean) LDS cycles per 32-lane group and read instruction over one strip of npx patches."""
    pc, kp, cpr = patch * ch, patch * patch * ch, kpad // 8
    worst, total, count = 0, 0, 0
    for first in range(0, npx * cpr, THREADS):          # one pass of the block's chunk loop
        for lane0 in range(first, min(first + THREADS, npx * cpr), 32):
            for i in range(8):                          # the i-th element of every lane's chunk: one read instruction
                banks = defaultdict(set)
                for f in range(lane0, min(lane0 + 32, npx * cpr)):
                    pxl, k = divmod(f, cpr)
                    k = k * 8 + i
                    if k >= kp:
                        continue
                    ky, r = divmod(k, pc)
                    kx, c = divmod(r, ch)
                    dword = ((ky * ch + c) * pitch + (pxl * patch + kx) * esz) // 4
                    banks[dword % 32].add(dword)
                if banks:
                    cyc = max(len(v) for v in banks.values())
                    worst, total, count = max(worst, cyc), total + cyc, count + 1
    return worst, total / max(count, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--kpad", type=int, default=0, help="default: patch^2 * channels rounded up to 64")
    a = ap.parse_args()
    kpad = a.kpad or (a.patch * a.patch * a.channels + 63) // 64 * 64
    print(f"image {a.image} patch {a.patch} channels {a.channels} kpad {kpad}: LDS cycles per 32-lane group and read (worst, mean)")
    for name, esz in (("f32", 4), ("f16/bf16", 2), ("u8", 1)):
        npx = choose_npx(a.image, a.patch, a.channels, esz)
        padded, plain = strip_pitch(npx, a.patch, esz), strip_pitch(npx, a.patch, esz, padded=False)
        wp, mp = build_cycles(a.image, a.patch, a.channels, kpad, esz, padded, npx)
        wu, mu = build_cycles(a.image, a.patch, a.channels, kpad, esz, plain, npx)
        print(f"  {name:9s} npx {npx:3d}  LDS {a.patch * a.channels * padded:6d} B  pitch {padded:5d} B: worst {wp} mean {mp:.2f}"
              f"   | unpadded pitch {plain:5d} B: worst {wu} mean {mu:.2f}")


if __name__ == "__main__":
    main()
