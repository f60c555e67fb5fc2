"""Host-side check of the planar YUV resize: builds tools/yuv_host_check (the planner and the kernel body of
kernels_resize_nv12.hip as host code under AddressSanitizer and UBSan, one thread per work-item, exact-size heap blocks), runs it over
the operator cases of tests/test_yuv_planar.py at every sub-sampling, odd layouts, left-sited boxes that reach or overhang the last
chroma column, a mixed batch, 40 small frames, one 1080 x 1920 frame and the two frames either side of the 4:4:4 planner boundary,
and compares each output with the fp32 emulation of tests/yuv_ref.py byte for byte.  Then the 16-bit instantiations:
the same operator cases with real 10 / 12 / 16-bit planes, all-0xFFFF words, even offsets and strides that are no multiple of 4
(UBSan's alignment check on every uint16_t and uint32_t load is what shows that the planner's even-offset rule suffices), both pair-load
paths of P016, a mixed batch, 40 small frames, one 1080 x 1920 P010 frame and the 4:4:4 planner boundary.  Then the packed 4:2:2
instantiations: every layout of YUY2 and Y210 over the cases of tests/test_packed422.py, v210 at every width mod 6
with bits 30-31 set, every offset, stride padding and base alignment either side of the one-load-per-macropixel rule, a mixed batch,
40 small frames and one 1080 x 1920 UYVY and v210 frame, each compared with the emulation of the DE-INTERLEAVED planes.  With
--packed444 the packed 4:4:4 body instead (the modes above are unchanged and do not run it): every 8-bit layout, Y416
and AYUV64, Y410 and V410 with their ignored bits set over the cases of tests/test_packed444.py, every offset, row padding and base
residue either side of the one-load-per-pixel rule, 3-byte and 4-byte pixels that end an exact-size heap block, mixed batches, 40
small frames, one 1080 x 1920 BGRA and Y410 frame and the 4:4:4 planner boundary, each compared with the emulation of the
de-interleaved planes (RGB layouts: under the pass-through matrix, which the body does not read).  CPU only; no device is touched.

    python tools/yuv_host_check.py               (needs libvithip.so: make -C vit-fpga_amd)
    python tools/yuv_host_check.py --packed      (the packed 4:2:2 cases alone)
    python tools/yuv_host_check.py --packed444   (the packed 4:4:4 cases)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-fpga_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nv12_ref as N  # noqa: E402
import vithip  # noqa: E402
import yuv_ref as Y  # noqa: E402
from test_gpu_nv12 import lay_out as lay_out_nv12  # noqa: E402
from test_gpu_yuv16 import lay_out16, lay_out_p016, pairs_of  # noqa: E402
from test_gpu_yuv_planar import lay_out, planner_boundary_444  # noqa: E402
from test_nv12 import make_nv12  # noqa: E402
from test_yuv16 import COLOURS16, make_yuv16  # noqa: E402
from test_yuv_planar import COLOURS, OP_CASES, SUBS, make_yuv  # noqa: E402
import yuv16_ref as W  # noqa: E402
import packed422_ref as P  # noqa: E402
from test_packed422 import PACKED_CASES, V210_WIDTHS  # noqa: E402
import packed444_ref as Q  # noqa: E402
from test_packed444 import PACKED_CASES as CASES444  # noqa: E402

EXE = os.path.join(ROOT, "tools", "yuv_host_check")
PKG = os.path.join(ROOT, "vit-fpga_amd")


def build():
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "yuv_host_check.hip"), "-o", EXE, "-L" + PKG, "-lvithip", "-Wl,-rpath," + PKG, "-lpthread"])


def run(tmp, label, planes, boxes, s, m, site, subs, wide=False, **layout):
    """One call of the host build; returns False if its bytes differ from the emulation.  subs None: `planes` are NV12 pairs (the
    other instantiation of the same body).  wide: uint16 planes, the two 16-bit instantiations."""
    if wide:
        buf, desc = lay_out_p016(planes, boxes, **layout) if subs is None else lay_out16(planes, boxes, subs, **layout)
    else:
        buf, desc = lay_out_nv12(planes, boxes, **layout) if subs is None else lay_out(planes, boxes, subs, **layout)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<4i", (0 if subs is None else 1) | (2 if wide else 0), s, len(planes), site))
        f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(struct.pack("<Q", buf.nbytes))
        f.write(bytes(desc))
        f.write(buf.tobytes())
    p = subprocess.run([EXE, case, out], capture_output=True, text=True)
    if p.returncode:
        print(f"FAIL {label}: exit {p.returncode}\n{p.stdout}{p.stderr}")
        return False
    got = np.fromfile(out, np.uint8).reshape(len(planes), s, s, 3)
    if subs is None:
        want = np.stack([N.resize_nv12_f32(y, uv, box, s, m, site) for (y, uv), box in zip(planes, boxes)])
    else:
        want = np.stack([Y.resize_yuv_f32(*yuv, box, s, m, site, sub) for yuv, box, sub in zip(planes, boxes, subs)])
    same = np.array_equal(got, want)
    print(f"{'ok  ' if same else 'DIFF'} {label}: {p.stdout.strip()}")
    return same


def run_packed(tmp, label, planes, boxes, s, m, site, layouts, shift_base=False, **layout):
    """One call of the packed instantiations; `planes` are the de-interleaved (Y, U, V) triples (v210: 10-bit codes), the emulation
    is that of the planar 4:2:2 frame (v210: of the codes << 6)."""
    wide = planes[0][0].dtype == np.uint16
    buf, desc = P.lay_out(planes, boxes, layouts, **layout)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<4i", 4 | (2 if wide else 0) | (8 if shift_base else 0), s, len(planes), site))
        f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(struct.pack("<Q", buf.nbytes))
        f.write(bytes(desc))
        f.write(buf.tobytes())
    p = subprocess.run([EXE, case, out], capture_output=True, text=True)
    if p.returncode:
        print(f"FAIL {label}: exit {p.returncode}\n{p.stdout}{p.stderr}")
        return False
    got = np.fromfile(out, np.uint8).reshape(len(planes), s, s, 3)
    words = lambda yuv, d: tuple((a << 6).astype(np.uint16) for a in yuv) if d.layout == P.V210 else yuv
    want = np.stack([Y.resize_yuv_f32(*words(yuv, d), box, s, m, site, P.SUB) for yuv, box, d in zip(planes, boxes, desc)])
    same = np.array_equal(got, want)
    print(f"{'ok  ' if same else 'DIFF'} packed {label}: {p.stdout.strip()}")
    return same


CODES10 = "bt2020_limited_10_lsb_left"   # make_yuv16 planes of 10-bit codes in the low bits: what v210 carries


def main_packed(tmp):
    """The packed 4:2:2 instantiations."""
    good = True
    mats8 = {k: (N.yuv_matrix(std, full), site) for k, (std, full, site) in COLOURS.items()}
    mats16 = {k: (W.yuv_matrix16(std, full, bits, msb), site) for k, (std, full, bits, msb, site) in COLOURS16.items()}
    two16 = ("bt709_limited_10_msb_left", "bt709_full_16_msb_centre")
    for name, (h, w, box, s) in PACKED_CASES.items():
        for lay in (P.YUYV, P.UYVY, P.YVYU, P.VYUY):
            for colour, (m, site) in mats8.items():
                good &= run_packed(tmp, f"{P.NAMES[lay]} {name} {colour}", [make_yuv(h, w, P.SUB, seed=h + w)], [box], s, m, site, lay)
            for colour in two16:
                m, site = mats16[colour]
                good &= run_packed(tmp, f"16-bit {P.NAMES[lay]} {name} {colour}", [make_yuv16(h, w, P.SUB, h + w, colour)], [box], s, m, site, lay)
        for colour in two16:
            m, site = mats16[colour]
            good &= run_packed(tmp, f"v210 {name} {colour}", [make_yuv16(h, w, P.SUB, h + w, CODES10)], [box], s, m, site, P.V210, high_bits=3)
    # v210 at every width mod 6, codes 0 and 1023 in every plane, bits 30-31 set; 1918 x 4: 320 blocks a row (-> 64: scale <= 32)
    for w in V210_WIDTHS:
        h, s = (4, 64) if w == 1918 else (5, 16)
        yuv = make_yuv16(h, w, P.SUB, w, CODES10)
        for a in yuv:
            a[0, 0], a[-1, -1] = 0, 1023
        for colour in two16:
            m, site = mats16[colour]
            good &= run_packed(tmp, f"v210 {h}x{w} {colour}", [yuv], [None], s, m, site, P.V210, high_bits=2)
    # either side of the one-load-per-macropixel rule: offsets, row padding and the base itself
    boxes = [None, (0.5, 3.0, 29.5, 40.0)]
    m, site = mats8["bt709_limited_left"]
    planes = [make_yuv(37, 53, P.SUB, seed=21), make_yuv(42, 30, P.SUB, seed=31)]
    for lead in (0, 1, 2, 3):
        for pad in (0, 1, 2):
            for shift in (False, True):
                good &= run_packed(tmp, f"8-bit alignment lead {lead} pad {pad} base+{int(shift)}", planes, boxes, 16, m, site, [P.UYVY, P.YVYU], shift, lead=lead, pad=pad, gap=lead)
    m, site = mats16["bt709_limited_10_msb_left"]
    planes = [make_yuv16(37, 53, P.SUB, 21, "bt709_limited_10_msb_left"), make_yuv16(42, 30, P.SUB, 31, "bt709_limited_10_msb_left")]
    for lead in (0, 2, 4, 6):
        for pad in (0, 2):
            for shift in (False, True):
                good &= run_packed(tmp, f"16-bit alignment lead {lead} pad {pad} base+{2 * int(shift)}", planes, boxes, 16, m, site, [P.YUYV, P.VYUY], shift, lead=lead, pad=pad, gap=lead)
    planes = [make_yuv16(37, 53, P.SUB, 21, CODES10), make_yuv16(42, 30, P.SUB, 31, CODES10)]
    for lead in (0, 4, 8, 12):
        for pad in (0, 4):
            good &= run_packed(tmp, f"v210 alignment lead {lead} pad {pad}", planes, boxes, 16, m, site, P.V210, lead=lead, pad=pad, gap=lead, high_bits=1)
    # bands and batches
    shapes = [(37, 53), (64, 64), (20, 24), (98, 132), (270, 480), (1, 1), (33, 2)]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
    m8, site8 = mats8["bt709_limited_left"]
    good &= run_packed(tmp, "8-bit mixed batch of 7", [make_yuv(h, w, P.SUB, seed=40 + i) for i, (h, w) in enumerate(shapes)], boxes, 32, m8, site8,
                       [i % 4 for i in range(7)], lead=1, gap=3, pad=1)
    good &= run_packed(tmp, "16-bit + v210 mixed batch of 7", [make_yuv16(h, w, P.SUB, 40 + i, CODES10) for i, (h, w) in enumerate(shapes)], boxes, 32,
                       W.yuv_matrix16(N.BT2020, False, 10, False), N.CHROMA_LEFT, [P.YUYV, P.UYVY, P.YVYU, P.VYUY, P.YUYV, P.UYVY, P.VYUY], lead=4, gap=4)
    mixed = [P.YUYV, P.V210, P.YVYU, P.V210, P.V210, P.UYVY, P.V210]
    planes = [make_yuv16(h, w, P.SUB, 40 + i, CODES10) for i, (h, w) in enumerate(shapes)]
    planes = [yuv if lay == P.V210 else tuple((a << 6).astype(np.uint16) for a in yuv) for yuv, lay in zip(planes, mixed)]
    good &= run_packed(tmp, "Y210 and v210 frames in one batch of 7", planes, boxes, 32, m, site, mixed, lead=4, gap=4)
    small = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    good &= run_packed(tmp, "8-bit 40 frames of 41x39 (tall bands)", [make_yuv(41, 39, P.SUB, seed=100 + i) for i in range(40)], small, 32, m8, site8,
                       [i % 4 for i in range(40)])
    good &= run_packed(tmp, "v210 40 frames of 41x39 (tall bands)", [make_yuv16(41, 39, P.SUB, 100 + i, CODES10) for i in range(40)], small, 32, m, site, P.V210)
    from test_nv12 import make_rgb
    rgb = make_rgb(1080, 1920, 3)
    crop = [vithip.center_crop_box(1080, 1920)]
    good &= run_packed(tmp, "1080x1920 UYVY -> 64", [Y.rgb_to_yuv_planes(rgb, *P.SUB)], crop, 64, m8, site8, P.UYVY)
    good &= run_packed(tmp, "1080x1920 v210 -> 64", [W.rgb_to_yuv16_planes(rgb, *P.SUB, 10, False)], crop, 64, m, site, P.V210)
    return good


PASS_THROUGH = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
GARBAGE = np.full((3, 4), 1e30, np.float32)   # what an RGB layout is handed as its matrix: it must not be read


def run_444(tmp, label, frames, boxes, s, m, layouts, shift=0, **layout):
    """One call of the packed 4:4:4 body; `frames` are component triples in output order (10-bit layouts: codes), the emulation is
    that of the planar 4:4:4 frame (10-bit: of the codes << 6; RGB layouts: under the pass-through matrix)."""
    wide = frames[0][0].dtype == np.uint16
    buf, desc = Q.lay_out(frames, boxes, layouts, **layout)
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<4i", 16 | (2 if wide else 0) | (shift << 8), s, len(frames), 0))
        f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(struct.pack("<Q", buf.nbytes))
        f.write(bytes(desc))
        f.write(buf.tobytes())
    p = subprocess.run([EXE, case, out], capture_output=True, text=True)
    if p.returncode:
        print(f"FAIL {label}: exit {p.returncode}\n{p.stdout}{p.stderr}")
        return False
    got = np.fromfile(out, np.uint8).reshape(len(frames), s, s, 3)
    words = lambda c, d: tuple((a << 6).astype(np.uint16) for a in c) if d.layout & 256 else c
    want = np.stack([Y.resize_yuv_f32(*words(c, d), box, s, m if Q.is_yuv(d.layout) else PASS_THROUGH, N.CHROMA_CENTER, Q.SUB)
                     for c, box, d in zip(frames, boxes, desc)])
    same = np.array_equal(got, want)
    print(f"{'ok  ' if same else 'DIFF'} packed 4:4:4 {label}: {p.stdout.strip()}")
    return same


def rgb_planes(h, w, seed):
    from test_nv12 import make_rgb
    rgb = make_rgb(h, w, seed)
    return tuple(np.ascontiguousarray(rgb[..., k]) for k in range(3))


def main_packed444(tmp):
    """The packed 4:4:4 instantiations."""
    good = True
    m8 = N.yuv_matrix(N.BT709, False)
    mats16 = {k: W.yuv_matrix16(std, full, bits, msb) for k, (std, full, bits, msb, _) in COLOURS16.items()}
    m10, m16 = mats16["bt709_limited_10_msb_left"], mats16["bt709_full_16_msb_centre"]
    for name, (h, w, box, s) in CASES444.items():
        for key, lay in Q.RGB_LAYOUTS.items():
            good &= run_444(tmp, f"{key} {name}", [rgb_planes(h, w, h + w)], [box], s, GARBAGE, lay)
        for key, lay in Q.YUV_LAYOUTS.items():
            for colour, (std, full, _) in COLOURS.items():
                good &= run_444(tmp, f"{key} {name} {colour}", [make_yuv(h, w, Q.SUB, seed=h + w)], [box], s, N.yuv_matrix(std, full), lay)
        for key, lay in Q.WORD_LAYOUTS.items():
            good &= run_444(tmp, f"{key} {name} 10 bits msb", [make_yuv16(h, w, Q.SUB, h + w, "bt709_limited_10_msb_left")], [box], s, m10, lay)
            good &= run_444(tmp, f"{key} {name} 16 bits", [make_yuv16(h, w, Q.SUB, h + w, "bt709_full_16_msb_centre")], [box], s, m16, lay)
        codes = make_yuv16(h, w, Q.SUB, h + w, CODES10)
        for a in codes:
            a[0, 0], a[-1, -1] = 0, 1023
        for key, lay in (("y410", Q.Y410), ("v410", Q.V410)):
            good &= run_444(tmp, f"{key} {name}", [codes], [box], s, m10, lay, ignored=3)
    # either side of the one-load-per-pixel rule: offsets, row padding and the base itself, every residue mod 8 that matters
    boxes = [None, (0.5, 3.0, 29.5, 40.0)]
    frames = [rgb_planes(37, 53, 21), make_yuv(42, 30, Q.SUB, seed=31)]
    for lead in (0, 1, 2, 3, 4, 6):
        for pad in (0, 1, 2, 3, 4):
            for shift in (0, 1, 2, 3):
                good &= run_444(tmp, f"4-byte pixels lead {lead} pad {pad} base+{shift}", frames, boxes, 16, m8, [Q.BGRA, Q.VUYA], shift, lead=lead, pad=pad, gap=lead)
    for lead in (0, 1, 3):
        for pad in (0, 1, 2):
            good &= run_444(tmp, f"3-byte pixels lead {lead} pad {pad}", frames, boxes, 16, m8, [Q.BGR, Q.YUV24], lead, lead=lead, pad=pad, gap=lead)
    frames = [make_yuv16(37, 53, Q.SUB, 21, "bt709_limited_10_msb_left"), make_yuv16(42, 30, Q.SUB, 31, "bt709_limited_10_msb_left")]
    for lead in (0, 2, 4, 6):
        for pad in (0, 2, 4, 6):
            for shift in (0, 2, 4, 6):
                good &= run_444(tmp, f"16-bit words lead {lead} pad {pad} base+{shift}", frames, boxes, 16, m10, [Q.Y416, Q.AYUV64], shift, lead=lead, pad=pad, gap=lead)
    frames = [make_yuv16(37, 53, Q.SUB, 21, CODES10), make_yuv16(42, 30, Q.SUB, 31, CODES10)]
    for lead in (0, 4, 12):
        for pad in (0, 4):
            for shift in (0, 4):
                good &= run_444(tmp, f"10-bit words lead {lead} pad {pad} base+{shift}", frames, boxes, 16, m10, [Q.Y410, Q.V410], shift, lead=lead, pad=pad, gap=lead, ignored=1)
    # a frame that ends with the heap block: the last pixel of a 3-byte and of a 4-byte layout, at every base residue
    for shift in (0, 1, 2, 3):
        for key, lay in (("bgr", Q.BGR), ("yuv24", Q.YUV24), ("bgra", Q.BGRA), ("argb", Q.ARGB)):
            good &= run_444(tmp, f"{key} 5x3 ends its block, base+{shift}", [rgb_planes(5, 3, 9)], [None], 16, m8, lay, shift, pad=shift)
            good &= run_444(tmp, f"{key} 7x54 ends its block, base+{shift}", [rgb_planes(7, 54, 9)], [None], 16, m8, lay, shift)
    # bands and batches
    shapes = [(37, 53), (64, 64), (20, 24), (98, 132), (270, 480), (1, 1), (33, 2)]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
    lays = [Q.BGR, Q.BGRA, Q.ARGB, Q.VUYA, Q.RGB, Q.AYUV, Q.YUV24]
    frames = [make_yuv(h, w, Q.SUB, seed=40 + i) if Q.is_yuv(lay) else rgb_planes(h, w, 40 + i) for i, ((h, w), lay) in enumerate(zip(shapes, lays))]
    good &= run_444(tmp, "8-bit mixed batch of 7", frames, boxes, 32, m8, lays, lead=1, gap=3, pad=1)
    mixed = [Q.Y416, Q.Y410, Q.V410, Q.AYUV64, Q.V410, Q.Y416, Q.Y410]
    frames = [make_yuv16(h, w, Q.SUB, 40 + i, CODES10) for i, (h, w) in enumerate(shapes)]
    frames = [c if lay & 256 else tuple((a << 6).astype(np.uint16) for a in c) for c, lay in zip(frames, mixed)]
    good &= run_444(tmp, "Y416, AYUV64, Y410 and V410 frames in one batch of 7", frames, boxes, 32, m10, mixed, lead=4, gap=4)
    small = [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)]
    every8 = list(Q.RGB_LAYOUTS.values()) + list(Q.YUV_LAYOUTS.values())
    lays = [every8[i % 9] for i in range(40)]
    good &= run_444(tmp, "8-bit 40 frames of 41x39 (tall bands)", [make_yuv(41, 39, Q.SUB, seed=100 + i) for i in range(40)], small, 32, m8, lays)
    good &= run_444(tmp, "Y410 40 frames of 41x39 (tall bands)", [make_yuv16(41, 39, Q.SUB, 100 + i, CODES10) for i in range(40)], small, 32, m10, Q.Y410)
    crop = [vithip.center_crop_box(1080, 1920)]
    good &= run_444(tmp, "1080x1920 BGRA -> 64", [rgb_planes(1080, 1920, 3)], crop, 64, GARBAGE, Q.BGRA)
    good &= run_444(tmp, "1080x1920 Y410 -> 64", [make_yuv16(1080, 1920, Q.SUB, 3, CODES10)], crop, 64, m10, Q.Y410)
    for h in planner_boundary_444(130):
        good &= run_444(tmp, f"4:4:4 planner boundary, VUYA {h}x36 -> 130", [make_yuv(h, 36, Q.SUB, seed=7)], [None], 130, m8, Q.VUYA)
        good &= run_444(tmp, f"4:4:4 planner boundary, Y416 {h}x36 -> 130", [make_yuv16(h, 36, Q.SUB, 7, "bt709_limited_10_msb_left")], [None], 130, m10, Q.Y416)
    return good


def main16(tmp):
    """The 16-bit instantiations."""
    good = True
    mats = {k: (W.yuv_matrix16(std, full, bits, msb), site) for k, (std, full, bits, msb, site) in COLOURS16.items()}
    for name, (h, w, box, s) in OP_CASES.items():
        for key, sub in SUBS.items():
            for colour, (m, site) in mats.items():
                good &= run(tmp, f"16-bit {name} {key} {colour}", [make_yuv16(h, w, sub, h + w, colour)], [box], s, m, site, [sub], wide=True)
        if h % 2 == 0 and w % 2 == 0:
            for colour in ("bt709_limited_10_msb_left", "bt709_full_16_msb_centre"):
                m, site = mats[colour]
                good &= run(tmp, f"P016 {name} {colour}", pairs_of([make_yuv16(h, w, (2, 2), h + w, colour)]), [box], s, m, site, None, wide=True)
    # words above 0x7fff
    unit = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32) * np.float32(255.0 / 65535.0)
    ones = lambda *shape: np.full(shape, 0xFFFF, np.uint16)
    good &= run(tmp, "all-0xFFFF planar 4:2:0", [(ones(38, 54), ones(19, 27), ones(19, 27))], [None], 16, unit, N.CHROMA_LEFT, [(2, 2)], wide=True)
    for lay in (dict(), dict(lead=2)):
        good &= run(tmp, f"all-0xFFFF P016 {lay}", [(ones(38, 54), ones(19, 27, 2))], [None], 16, unit, N.CHROMA_LEFT, None, wide=True, **lay)
    # even offsets and strides that are no multiple of 4: every 16-bit load aligned by the planner's rule alone
    colour = "bt601_full_12_lsb_centre"
    m, site = mats[colour]
    planes = [make_yuv16(37, 53, (2, 2), 21, colour), make_yuv16(42, 31, (2, 1), 31, colour), make_yuv16(29, 30, (1, 1), 41, colour)]
    boxes, subs = [None, (0.5, 3.0, 29.5, 40.0), None], [(2, 2), (2, 1), (1, 1)]
    for lay in (dict(pads=(6, 10, 2)), dict(pads=(4, 0, 0), lead=2), dict(pads=(0, 2, 0)), dict(lead=6, gap=2), dict(order="yvu"), dict(gap=64, order="uvy"),
                dict(lead=10, gap=6, order="vyu", pads=(2, 0, 4))):
        good &= run(tmp, f"16-bit layout {lay}", planes, boxes, 16, m, site, subs, wide=True, **lay)
    # P016: one 32-bit load per pair (uv_offset, uv_stride = 0 mod 4) and two 16-bit loads (either = 2 mod 4)
    m, site = mats["bt709_limited_10_msb_left"]
    p010 = "bt709_limited_10_msb_left"
    pairs = pairs_of([make_yuv16(38, 54, (2, 2), 21, p010), make_yuv16(42, 30, (2, 2), 31, p010)])
    for lay in (dict(), dict(lead=2), dict(uv_pad=2), dict(lead=4), dict(y_pad=6, uv_pad=12), dict(lead=2, gap=2, y_pad=2, uv_pad=6), dict(gap=64, uv_first=True)):
        good &= run(tmp, f"P016 layout {lay}", pairs, [None, (0.5, 3.0, 29.5, 40.0)], 16, m, site, None, wide=True, **lay)
    shapes = [(37, 53, "420"), (64, 64, "444"), (20, 24, "422"), (98, 132, "440"), (270, 480, "420"), (1, 1, "420"), (33, 2, "422")]
    planes = [make_yuv16(h, w, SUBS[k], 40 + i, p010) for i, (h, w, k) in enumerate(shapes)]
    boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
    good &= run(tmp, "16-bit mixed batch of 7", planes, boxes, 32, m, site, [SUBS[k] for _, _, k in shapes], wide=True, lead=2, gap=6)
    keys = list(SUBS)
    subs = [SUBS[keys[i % 4]] for i in range(40)]
    planes = [make_yuv16(41, 39, subs[i], 100 + i, p010) for i in range(40)]
    good &= run(tmp, "16-bit 40 frames of 41x39 (tall bands)", planes, [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)], 32, m, site, subs, wide=True)
    from test_nv12 import make_rgb
    big = [W.rgb_to_yuv16_planes(make_rgb(1080, 1920, 3), 2, 2, 10, True)]
    good &= run(tmp, "1080x1920 P010 -> 64", pairs_of(big), [vithip.center_crop_box(1080, 1920)], 64, m, site, None, wide=True)
    m, site = mats[colour]
    for h in planner_boundary_444(130):
        good &= run(tmp, f"16-bit 4:4:4 planner boundary, {h}x36 -> 130", [make_yuv16(h, 36, (1, 1), 7, colour)], [None], 130, m, site, [(1, 1)], wide=True)
    return good


def main():
    build()
    good = True
    if "--packed444" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            good = main_packed444(tmp)
        print("every output equals the fp32 emulation; no sanitizer report" if good else "FAILED")
        return 0 if good else 1
    if "--packed" in sys.argv[1:]:
        with tempfile.TemporaryDirectory() as tmp:
            good = main_packed(tmp)
        print("every output equals the fp32 emulation; no sanitizer report" if good else "FAILED")
        return 0 if good else 1
    with tempfile.TemporaryDirectory() as tmp:
        for name, (h, w, box, s) in OP_CASES.items():
            for key, sub in SUBS.items():
                for colour, (std, full, site) in COLOURS.items():
                    good &= run(tmp, f"{name} {key} {colour}", [make_yuv(h, w, sub, seed=h + w)], [box], s, N.yuv_matrix(std, full), site, [sub])
        m = N.yuv_matrix(N.BT709, False)
        # left siting: an odd width reaches into the half-covered last chroma column, an even one overhangs it by a quarter sample
        for h, w in ((37, 53), (38, 54), (33, 2), (1, 1)):
            for key in ("420", "422"):
                good &= run(tmp, f"left-sited whole frame {h}x{w} {key}", [make_yuv(h, w, SUBS[key], seed=5)], [None], 16, m, N.CHROMA_LEFT, [SUBS[key]])
        planes = [make_yuv(37, 53, (2, 2), seed=21), make_yuv(42, 31, (2, 1), seed=31), make_yuv(29, 30, (1, 1), seed=41)]
        boxes, subs = [None, (0.5, 3.0, 29.5, 40.0), None], [(2, 2), (2, 1), (1, 1)]
        for lay in (dict(pads=(6, 10, 2)), dict(pads=(5, 0, 0), lead=2), dict(pads=(0, 3, 0)), dict(lead=3, gap=7), dict(lead=1, gap=2, pads=(5, 7, 3)),
                    dict(order="yvu"), dict(gap=64, order="uvy"), dict(lead=5, gap=1, order="vyu", pads=(1, 0, 2))):
            good &= run(tmp, f"layout {lay}", planes, boxes, 16, m, N.CHROMA_LEFT, subs, **lay)
        shapes = [(37, 53, "420"), (64, 64, "444"), (20, 24, "422"), (98, 132, "440"), (270, 480, "420"), (1, 1, "420"), (33, 2, "422")]
        planes = [make_yuv(h, w, SUBS[k], seed=40 + i) for i, (h, w, k) in enumerate(shapes)]
        boxes = [None, None, (2.0, 1.0, 22.0, 19.5), (10.0, 5.0, 101.0, 96.0), vithip.center_crop_box(270, 480), None, None]
        good &= run(tmp, "mixed batch of 7", planes, boxes, 32, m, N.CHROMA_LEFT, [SUBS[k] for _, _, k in shapes], lead=1, gap=3)
        keys = list(SUBS)
        subs = [SUBS[keys[i % 4]] for i in range(40)]
        planes = [make_yuv(41, 39, subs[i], seed=100 + i) for i in range(40)]
        good &= run(tmp, "40 frames of 41x39 (tall bands)", planes, [None if i % 2 else (0.5, 1.0, 38.25, 40.0) for i in range(40)], 32,
                    N.yuv_matrix(N.BT601, True), N.CHROMA_CENTER, subs)
        y, uv = make_nv12(1080, 1920, seed=3)
        good &= run(tmp, "1080x1920 I420 -> 224", [(y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]))],
                    [vithip.center_crop_box(1080, 1920)], 224, m, N.CHROMA_LEFT, [(2, 2)])
        # the NV12 instantiation: 16-bit UV loads (even offsets and strides) and byte loads (odd), left-sited overhang
        nv = [make_nv12(38, 54, seed=21), make_nv12(42, 30, seed=31)]
        for lay in (dict(), dict(y_pad=6, uv_pad=10), dict(lead=1, gap=2, y_pad=5, uv_pad=7), dict(gap=64, uv_first=True)):
            good &= run(tmp, f"NV12 layout {lay}", nv, [None, (0.5, 3.0, 29.5, 40.0)], 16, m, N.CHROMA_LEFT, None, **lay)
        for h in planner_boundary_444(130):
            good &= run(tmp, f"4:4:4 planner boundary, {h}x36 -> 130", [make_yuv(h, 36, (1, 1), seed=7)], [None], 130, m, N.CHROMA_LEFT, [(1, 1)])
        good &= main16(tmp)
        good &= main_packed(tmp)
    print("every output equals the fp32 emulation; no sanitizer report" if good else "FAILED")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
