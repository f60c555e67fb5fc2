#!/usr/bin/env python3
"""Frames measurements (run on the GPU box): what resizing and cropping on the GPU costs on the host path.

  python tools/frames_bench.py [--out profiles] [--steps 30] [--passes 3] [--only NAME]

In ONE process, for ViT-B/16 bf16 at batch 512, ViT-B/16 fp8 at batch 512 and CLIP ViT-B/32 bf16 at batch 256, three rings of 3
slots (pinned host memory -> logits in host memory), interleaved `passes` times, the median pass reported with min and max:
  (1) the u8 ring fed pre-resized 224 x 224 images -- the yardstick;
  (2) the frames ring fed 256 x 256 frames with the 0.875 centre box (scale exactly 1: the resize is a crop);
  (3) the frames ring fed 360 x 480 frames with the 0.875 centre box (315 x 315 -> 224, about 4 taps per axis).
The images of (1) are the centre crops of the frames of (2), so those two rings compute the same logits, which is checked.
Then the resize launch of (2) and (3) alone, hip events around it (vh_set_stage_timing("resize")), two interleaved passes: us per
launch and the GB/s of source bytes inside the boxes.  Written to <out>/frames_host_path.txt and .json.

  python tools/frames_bench.py --nv12 [--out profiles] [--steps 30] [--passes 3]

NV12 passes instead, ViT-B/16 bf16, in ONE process: the frames ring fed RGB frames against the frames ring fed the
NV12 frames of the same pictures (nv12_ref.rgb_to_nv12, BT.709 limited range), at 360 x 480 (batch 512) and at 1080 x 1920 (batch
64), 0.875 centre box, interleaved passes and medians as above; then the resize launch of each in us and GB/s of source bytes
inside the boxes.  Written to <out>/nv12_host_path.txt and .json.

  python tools/frames_bench.py --yuv420p [--out profiles] [--steps 30] [--passes 3]

Planar passes, ViT-B/16 bf16, in ONE process: the frames ring fed NV12 frames -- the yardstick, it moves the same
bytes -- against the frames ring fed the I420 (yuv420p) planes of the same pictures, the same two shapes, boxes, passes and medians;
the two rings compute the same logits, which is checked.  Written to <out>/yuv_planar_host_path.txt and .json.

  python tools/frames_bench.py --p010 [--out profiles] [--steps 30] [--passes 3]

10-bit passes, ViT-B/16 bf16, in ONE process: the frames ring fed RGB frames, the frames ring fed the NV12 frames of
the same pictures and the frames ring fed their P010 frames (10-bit code = 8-bit code x 4, in the high bits of the word: byte << 8),
the same two shapes, boxes, passes and medians.  P010 uploads 3 bytes per pixel, as RGB does and twice what NV12 does.  Under the two
default colour states the NV12 and the P010 ring compute the same logits, which is checked.  Then the resize launch of each of the
three.  Written to <out>/yuv16_host_path.txt and .json.

  python tools/frames_bench.py --yuy2 [--out profiles] [--steps 30] [--passes 3]

Packed 4:2:2 passes, ViT-B/16 bf16, in ONE process: the frames rings fed RGB frames, the NV12 frames, the planar
4:2:2 planes, the YUY2 frames of those planes and their v210 frames (10-bit code = 8-bit code x 4), the same two shapes, boxes, passes
and medians.  YUY2 uploads 2 bytes per pixel, v210 16 bytes per 6 pixels.  The planar 4:2:2, the YUY2 and the v210 ring compute the
same logits under the two default colour states, which is checked.  Then the resize launch of each of the five.  Written to
<out>/packed422_host_path.txt and .json.

  python tools/frames_bench.py --bgra [--out profiles] [--steps 30] [--passes 3]

Packed 4:4:4 passes, ViT-B/16 bf16, in ONE process: the frames rings fed the SAME pictures as RGB frames, as their
BGRA frames, as the planar 4:4:4 planes, as the VUYA frames of those planes and as their Y410 frames (10-bit code = 8-bit code x 4),
the same two shapes, boxes, passes and medians.  BGRA, VUYA and Y410 upload 4 bytes per pixel, RGB and planar 4:4:4 three.  The BGRA
ring computes the RGB ring's logits, the VUYA and the Y410 ring the planar ring's, which is checked.  Then the resize launch of each
of the five, and the two ratios measured in this process: packed against planar 4:4:4 and BGRA against RGB.  Written to
<out>/packed444_host_path.txt and .json.
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

DT = {"bf16": vithip.DTYPE_BF16, "fp8": vithip.DTYPE_FP8}
CLIP_B32 = dict(image_size=224, patch_size=32, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=512)
RUNS = [("ViT-B/16 bf16 b512", "vit_b16_bf16", S.CONFIGS["vit_base"], "bf16", 512, 0, 1e-6),
        ("ViT-B/16 fp8 b512", "vit_b16_fp8", S.CONFIGS["vit_base"], "fp8", 512, 0, 1e-6),
        ("CLIP ViT-B/32 bf16 b256", "clip_b32_bf16", CLIP_B32, "bf16", 256, vithip.FLAG_PRE_LN | vithip.FLAG_QUICK_GELU, 1e-5)]
SLOTS = 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Side:
    """One context with one ring: u8 slots fed `images`, or frames slots fed `frames` (one [B, H, W, C] array) and one box."""

    def __init__(self, cfg, dname, batch, flags, eps, scale, shift, images=None, frames=None, box=None):
        self.batch, self.frames = batch, frames is not None
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        if self.frames:
            _, h, w, ch = frames.shape
            self.nbytes = frames.nbytes
            self.desc = (vithip.Frame * batch)()
            for b in range(batch):
                d = self.desc[b]
                d.offset, d.height, d.width, d.row_stride = b * h * w * ch, h, w, w * ch
                d.box[:] = box
            self.box_bytes = batch * (box[2] - box[0]) * (box[3] - box[1]) * ch
            self.ctx.ring_create_frames(SLOTS, batch, self.nbytes)
        else:
            self.nbytes = images.nbytes
            self.ctx.ring_create(SLOTS, batch, u8=True)
        for _ in range(SLOTS):   # fill every slot's pinned staging buffer once (a producer writes there in place); warms up too
            if self.frames:
                self.ctx.ring_input_frames()[:self.nbytes] = frames.reshape(-1)
            else:
                self.ctx.ring_input_u8(batch)[...] = images
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]

    def submit(self):
        if self.frames:
            self.ctx.ring_submit_frames_packed(None, self.nbytes, self.desc)
        else:
            self.ctx.ring_submit_u8(None, self.batch)

    def ring_rate(self, steps):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        inflight = 0
        for _ in range(steps):
            if inflight == SLOTS:
                self.ctx.ring_collect(); inflight -= 1
            self.submit(); inflight += 1
        while inflight:
            self.ctx.ring_collect(); inflight -= 1
        return self.batch * steps / (time.perf_counter() - t0)

    def resize_us(self, steps):
        self.ctx.set_stage_timing("resize")
        for _ in range(steps):
            self.submit()
            self.ctx.ring_collect()
        avg_ms, min_ms, launches = self.ctx.get_stage_timing()
        self.ctx.set_stage_timing(None)
        return avg_ms * 1e3, min_ms * 1e3, launches

    def close(self):
        self.ctx.close()


class SideNV12(Side):
    """One context with a frames ring fed NV12 frames: y [B, H, W] and uv [B, H/2, W/2, 2], each frame's planes back to back."""

    def __init__(self, cfg, dname, batch, flags, eps, scale, shift, y, uv, box):
        self.batch, self.frames = batch, True
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        _, h, w = y.shape
        per = h * w * 3 // 2
        buf = np.empty((batch, per), np.uint8)
        buf[:, :h * w] = y.reshape(batch, -1)
        buf[:, h * w:] = uv.reshape(batch, -1)
        self.nbytes = buf.nbytes
        self.desc = (vithip.FrameNV12 * batch)()
        for b in range(batch):
            d = self.desc[b]
            d.y_offset, d.uv_offset, d.height, d.width, d.y_stride, d.uv_stride = b * per, b * per + h * w, h, w, w, w
            d.box[:] = box
        self.box_bytes = batch * (box[2] - box[0]) * (box[3] - box[1]) * 1.5
        self.ctx.ring_create_frames(SLOTS, batch, self.nbytes)
        for _ in range(SLOTS):
            self.ctx.ring_input_frames()[:self.nbytes] = buf.reshape(-1)
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]

    def submit(self):
        self.ctx.ring_submit_frames_nv12_packed(None, self.nbytes, self.desc)


class SideYUV(SideNV12):
    """One context with a frames ring fed I420 frames: y [B, H, W], u and v [B, H/2, W/2], each frame's planes back to back."""

    def __init__(self, cfg, dname, batch, flags, eps, scale, shift, y, u, v, box):
        self.batch, self.frames = batch, True
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        _, h, w = y.shape
        q = (h // 2) * (w // 2)
        per = h * w + 2 * q
        buf = np.empty((batch, per), np.uint8)
        buf[:, :h * w] = y.reshape(batch, -1)
        buf[:, h * w:h * w + q] = u.reshape(batch, -1)
        buf[:, h * w + q:] = v.reshape(batch, -1)
        self.nbytes = buf.nbytes
        self.desc = (vithip.FrameYUV * batch)()
        for b in range(batch):
            d = self.desc[b]
            d.y_offset, d.u_offset, d.v_offset = b * per, b * per + h * w, b * per + h * w + q
            d.height, d.width, d.y_stride, d.u_stride, d.v_stride, d.sub_x, d.sub_y = h, w, w, w // 2, w // 2, 2, 2
            d.box[:] = box
        self.box_bytes = batch * (box[2] - box[0]) * (box[3] - box[1]) * 1.5
        self.ctx.ring_create_frames(SLOTS, batch, self.nbytes)
        for _ in range(SLOTS):
            self.ctx.ring_input_frames()[:self.nbytes] = buf.reshape(-1)
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]

    def submit(self):
        self.ctx.ring_submit_frames_yuv_packed(None, self.nbytes, self.desc)


class SideP010(SideNV12):
    """One context with a frames ring fed P010 frames: y [B, H, W] and uv [B, H/2, W/2, 2] uint16, each frame's planes back to back."""

    def __init__(self, cfg, dname, batch, flags, eps, scale, shift, y, uv, box):
        self.batch, self.frames = batch, True
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        _, h, w = y.shape
        per = h * w * 3 // 2                                                               # words per frame
        buf = np.empty((batch, per), "<u2")
        buf[:, :h * w] = y.reshape(batch, -1)
        buf[:, h * w:] = uv.reshape(batch, -1)
        self.nbytes = buf.nbytes
        self.desc = (vithip.FrameNV12 * batch)()
        for b in range(batch):
            d = self.desc[b]
            d.y_offset, d.uv_offset, d.height, d.width, d.y_stride, d.uv_stride = 2 * b * per, 2 * (b * per + h * w), h, w, 2 * w, 2 * w
            d.box[:] = box
        self.box_bytes = batch * (box[2] - box[0]) * (box[3] - box[1]) * 3.0
        self.ctx.ring_create_frames(SLOTS, batch, self.nbytes)
        for _ in range(SLOTS):
            self.ctx.ring_input_frames()[:self.nbytes] = buf.reshape(-1).view(np.uint8)
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]

    def submit(self):
        self.ctx.ring_submit_frames_p016_packed(None, self.nbytes, self.desc)


class SideRaw(SideNV12):
    """One context with a frames ring fed `buf` [B, bytes per frame] as `desc` describes it; submit: the name of the ring submit."""

    def __init__(self, cfg, dname, batch, flags, eps, scale, shift, buf, desc, box_bytes, submit):
        self.batch, self.frames = batch, True
        self.ctx = vithip.VitContext(cfg, dtype=DT[dname], max_batch=batch, flags=flags, ln_eps=eps)
        self.ctx.init_weights_seeded(0)
        self.ctx.set_input_norm(scale, shift)
        self.nbytes, self.desc, self.box_bytes = buf.nbytes, desc, box_bytes
        self.call = getattr(self.ctx, submit)
        self.ctx.ring_create_frames(SLOTS, batch, self.nbytes)
        for _ in range(SLOTS):
            self.ctx.ring_input_frames()[:self.nbytes] = buf.reshape(-1)
            self.submit()
        self.first = [self.ctx.ring_collect().copy() for _ in range(SLOTS)][0]

    def submit(self):
        self.call(None, self.nbytes, self.desc)


def yuy2_main(a):
    import nv12_ref as N
    import packed422_ref as P
    import yuv_ref as Y
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    title, key, cfg, dname, _, flags, eps = RUNS[0]
    log(f"frames_bench --yuy2: {title[:-5]}, frames rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (RGB frames, "
        f"the NV12 frames, the planar 4:2:2 planes, the YUY2 and the v210 frames of the same pictures, v210 code = byte x 4; 0.875 centre box); "
        f"median pass [min .. max]; images/s")
    for h, w, batch in ((360, 480, 512), (1080, 1920, 64)):
        rng = np.random.default_rng(3)
        small = rng.integers(0, 256, size=(batch, h // 8, w // 8, 3), dtype=np.uint8)
        rgb = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))     # the pictures of --nv12
        rgb ^= rng.integers(0, 8, size=rgb.shape, dtype=np.uint8)
        box = vithip.center_crop_box(h, w)
        inside = batch * (box[2] - box[0]) * (box[3] - box[1])
        common = (cfg, dname, batch, flags, eps, scale, shift)
        nv = [N.rgb_to_nv12(f) for f in rgb]
        p422 = [Y.rgb_to_yuv_planes(f, 2, 1) for f in rgb]
        cw = w // 2
        planar = np.stack([np.concatenate([p.reshape(-1) for p in t]) for t in p422])
        yuy2 = np.stack([P.interleave(*t, P.YUYV).reshape(-1) for t in p422])
        v210 = np.stack([P.to_v210(*(p.astype(np.uint16) << 2 for p in t)).astype("<u4").view(np.uint8).reshape(-1) for t in p422])
        dpl, dyu, dv2 = (vithip.FrameYUV * batch)(), (vithip.FrameYUY2 * batch)(), (vithip.FrameYUY2 * batch)()
        for b in range(batch):
            d, per = dpl[b], planar.shape[1]
            d.y_offset, d.u_offset, d.v_offset = b * per, b * per + h * w, b * per + h * w + h * cw
            d.height, d.width, d.y_stride, d.u_stride, d.v_stride, d.sub_x, d.sub_y = h, w, w, cw, cw, 2, 1
            d.box[:] = box
            for d, buf, lay in ((dyu[b], yuy2, P.YUYV), (dv2[b], v210, P.V210)):
                d.offset, d.height, d.width, d.row_stride, d.layout = b * buf.shape[1], h, w, buf.shape[1] // h, lay
                d.box[:] = box
        sides = dict(rgb=Side(*common, frames=rgb, box=box),
                     nv12=SideNV12(*common, y=np.stack([p[0] for p in nv]), uv=np.stack([p[1] for p in nv]), box=box),
                     p422=SideRaw(*common, planar, dpl, inside * 2.0, "ring_submit_frames_yuv_packed"),
                     yuy2=SideRaw(*common, yuy2, dyu, inside * 2.0, "ring_submit_frames_yuy2_packed"),
                     v210=SideRaw(*common, v210, dv2, inside * 16.0 / 6.0, "ring_submit_frames_y210_packed"))
        del rgb, nv, p422, planar, yuy2, v210
        bits = lambda k: sides[k].first.view(np.uint32)
        same = bool(np.array_equal(bits("p422"), bits("yuy2")) and np.array_equal(bits("p422"), bits("v210")) and np.isfinite(sides["yuy2"].first).all())
        rates = {k: [] for k in sides}
        for _ in range(a.passes):
            for k, sd in sides.items():
                rates[k].append(sd.ring_rate(a.steps))
        us = {k: [] for k in sides}
        for _ in range(2):                                                                 # two interleaved passes of the launch alone
            for k, sd in sides.items():
                us[k].append(sd.resize_us(8))
        r = dict(config=key, frame=[h, w], batch=batch, logits_yuy2_and_v210_equal_planar_422=same,
                 ring={k: mid(v) for k, v in rates.items()}, h2d_MB_per_step={k: sd.nbytes / 1e6 for k, sd in sides.items()},
                 bytes_per_pixel={k: sd.nbytes / (batch * h * w) for k, sd in sides.items()},
                 resize_us_avg={k: [t[0] for t in v] for k, v in us.items()}, resize_us_min={k: min(t[1] for t in v) for k, v in us.items()},
                 box_MB={k: sd.box_bytes / 1e6 for k, sd in sides.items()})
        rows.append(r)
        log(f"{h}x{w}, batch {batch}: logits of the YUY2 and the v210 ring equal the planar 4:2:2 ring's bit for bit: {same}")
        for k, sd in sides.items():
            m, lo, hi = r["ring"][k]
            log(f"    frames ring, {k.upper():4s}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / r['ring']['rgb'][0]:6.2f} % of the RGB ring, "
                f"{100 * m / r['ring']['p422'][0]:6.2f} % of the planar 4:2:2 ring | upload {sd.nbytes / 1e6:7.1f} MB per step "
                f"({r['bytes_per_pixel'][k]:.3f} bytes per pixel) = {sd.nbytes * 1e-9 * m / batch:5.1f} GB/s")
        for k, sd in sides.items():
            avg, mb = r["resize_us_avg"][k], sd.box_bytes / 1e6
            t = float(np.mean(avg))
            log(f"    resize {k.upper():4s}: {t:8.1f} us per launch avg ({r['resize_us_min'][k]:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (t * 1e-6):.0f} GB/s")
        for sd in sides.values():
            sd.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "packed422_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "packed422_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def bgra_main(a):
    import packed444_ref as Q
    import yuv_ref as Y
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    title, key, cfg, dname, _, flags, eps = RUNS[0]
    log(f"frames_bench --bgra: {title[:-5]}, frames rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (RGB frames, "
        f"their BGRA frames, the planar 4:4:4 planes, the VUYA and the Y410 frames of those planes, Y410 code = byte x 4; 0.875 centre box); "
        f"median pass [min .. max]; images/s")
    for h, w, batch in ((360, 480, 512), (1080, 1920, 64)):
        rng = np.random.default_rng(3)
        small = rng.integers(0, 256, size=(batch, h // 8, w // 8, 3), dtype=np.uint8)
        rgb = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))     # the pictures of --nv12
        rgb ^= rng.integers(0, 8, size=rgb.shape, dtype=np.uint8)
        box = vithip.center_crop_box(h, w)
        inside = batch * (box[2] - box[0]) * (box[3] - box[1])
        common = (cfg, dname, batch, flags, eps, scale, shift)
        p444 = [Y.rgb_to_yuv_planes(f, 1, 1) for f in rgb]
        planar = np.stack([np.concatenate([p.reshape(-1) for p in t]) for t in p444])
        bgra = np.stack([Q.row_bytes(tuple(f[..., k] for k in range(3)), Q.BGRA).reshape(-1) for f in rgb])
        vuya = np.stack([Q.row_bytes(t, Q.VUYA).reshape(-1) for t in p444])
        y410 = np.stack([Q.row_bytes(tuple(p.astype(np.uint16) << 2 for p in t), Q.Y410).reshape(-1) for t in p444])
        dpl = (vithip.FrameYUV * batch)()
        dbg, dvu, dy4 = ((vithip.FrameBGRA * batch)() for _ in range(3))
        for b in range(batch):
            d, per = dpl[b], planar.shape[1]
            d.y_offset, d.u_offset, d.v_offset = b * per, b * per + h * w, b * per + 2 * h * w
            d.height, d.width, d.y_stride, d.u_stride, d.v_stride, d.sub_x, d.sub_y = h, w, w, w, w, 1, 1
            d.box[:] = box
            for d, buf, lay in ((dbg[b], bgra, Q.BGRA), (dvu[b], vuya, Q.VUYA), (dy4[b], y410, Q.Y410)):
                d.offset, d.height, d.width, d.row_stride, d.layout = b * buf.shape[1], h, w, buf.shape[1] // h, lay
                d.box[:] = box
        sides = dict(rgb=Side(*common, frames=rgb, box=box),
                     bgra=SideRaw(*common, bgra, dbg, inside * 4.0, "ring_submit_frames_bgra_packed"),
                     p444=SideRaw(*common, planar, dpl, inside * 3.0, "ring_submit_frames_yuv_packed"),
                     vuya=SideRaw(*common, vuya, dvu, inside * 4.0, "ring_submit_frames_bgra_packed"),
                     y410=SideRaw(*common, y410, dy4, inside * 4.0, "ring_submit_frames_y410_packed"))
        del rgb, p444, planar, bgra, vuya, y410
        bits = lambda k: sides[k].first.view(np.uint32)
        same_rgb = bool(np.array_equal(bits("rgb"), bits("bgra")) and np.isfinite(sides["bgra"].first).all())
        same_yuv = bool(np.array_equal(bits("p444"), bits("vuya")) and np.array_equal(bits("p444"), bits("y410")) and np.isfinite(sides["vuya"].first).all())
        rates = {k: [] for k in sides}
        for _ in range(a.passes):
            for k, sd in sides.items():
                rates[k].append(sd.ring_rate(a.steps))
        us = {k: [] for k in sides}
        for _ in range(2):                                                                 # two interleaved passes of the launch alone
            for k, sd in sides.items():
                us[k].append(sd.resize_us(8))
        t = {k: float(np.mean([x[0] for x in v])) for k, v in us.items()}
        r = dict(config=key, frame=[h, w], batch=batch, logits_bgra_equal_rgb=same_rgb, logits_vuya_and_y410_equal_planar_444=same_yuv,
                 ring={k: mid(v) for k, v in rates.items()}, h2d_MB_per_step={k: sd.nbytes / 1e6 for k, sd in sides.items()},
                 bytes_per_pixel={k: sd.nbytes / (batch * h * w) for k, sd in sides.items()},
                 resize_us_avg={k: [x[0] for x in v] for k, v in us.items()}, resize_us_min={k: min(x[1] for x in v) for k, v in us.items()},
                 box_MB={k: sd.box_bytes / 1e6 for k, sd in sides.items()},
                 resize_ratio=dict(vuya_over_planar_444=t["vuya"] / t["p444"], y410_over_planar_444=t["y410"] / t["p444"], bgra_over_rgb=t["bgra"] / t["rgb"]))
        rows.append(r)
        log(f"{h}x{w}, batch {batch}: logits of the BGRA ring equal the RGB ring's bit for bit: {same_rgb}; of the VUYA and the Y410 ring the planar 4:4:4 ring's: {same_yuv}")
        for k, sd in sides.items():
            m, lo, hi = r["ring"][k]
            log(f"    frames ring, {k.upper():4s}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / r['ring']['rgb'][0]:6.2f} % of the RGB ring, "
                f"{100 * m / r['ring']['p444'][0]:6.2f} % of the planar 4:4:4 ring | upload {sd.nbytes / 1e6:7.1f} MB per step "
                f"({r['bytes_per_pixel'][k]:.3f} bytes per pixel) = {sd.nbytes * 1e-9 * m / batch:5.1f} GB/s")
        for k, sd in sides.items():
            avg, mb = r["resize_us_avg"][k], sd.box_bytes / 1e6
            log(f"    resize {k.upper():4s}: {t[k]:8.1f} us per launch avg ({r['resize_us_min'][k]:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (t[k] * 1e-6):.0f} GB/s")
        q = r["resize_ratio"]
        log(f"    resize launch, same process: VUYA / planar 4:4:4 = {q['vuya_over_planar_444']:.3f}, Y410 / planar 4:4:4 = {q['y410_over_planar_444']:.3f}, "
            f"BGRA / RGB = {q['bgra_over_rgb']:.3f}")
        for sd in sides.values():
            sd.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "packed444_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "packed444_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def p010_main(a):
    import nv12_ref as N
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    title, key, cfg, dname, _, flags, eps = RUNS[0]
    log(f"frames_bench --p010: {title[:-5]}, frames rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (RGB frames, "
        f"the NV12 frames and the P010 frames of the same pictures, word = byte << 8; 0.875 centre box); median pass [min .. max]; images/s")
    for h, w, batch in ((360, 480, 512), (1080, 1920, 64)):
        rng = np.random.default_rng(3)
        small = rng.integers(0, 256, size=(batch, h // 8, w // 8, 3), dtype=np.uint8)
        rgb = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))     # the pictures of --nv12
        rgb ^= rng.integers(0, 8, size=rgb.shape, dtype=np.uint8)
        planes = [N.rgb_to_nv12(f) for f in rgb]
        y, uv = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        del planes
        box = vithip.center_crop_box(h, w)
        common = (cfg, dname, batch, flags, eps, scale, shift)
        sides = dict(rgb=Side(*common, frames=rgb, box=box), nv12=SideNV12(*common, y=y, uv=uv, box=box),
                     p010=SideP010(*common, y=y.astype(np.uint16) << 8, uv=uv.astype(np.uint16) << 8, box=box))
        del rgb
        same = bool(np.array_equal(sides["nv12"].first.view(np.uint32), sides["p010"].first.view(np.uint32)) and np.isfinite(sides["p010"].first).all())
        rates = {k: [] for k in sides}
        for _ in range(a.passes):
            for k, sd in sides.items():
                rates[k].append(sd.ring_rate(a.steps))
        us = {k: [] for k in sides}
        for _ in range(2):                                                                 # two interleaved passes of the launch alone
            for k, sd in sides.items():
                us[k].append(sd.resize_us(8))
        r = dict(config=key, frame=[h, w], batch=batch, logits_p010_equal_nv12=same,
                 ring={k: mid(v) for k, v in rates.items()}, h2d_MB_per_step={k: sd.nbytes / 1e6 for k, sd in sides.items()},
                 resize_us_avg={k: [t[0] for t in v] for k, v in us.items()}, resize_us_min={k: min(t[1] for t in v) for k, v in us.items()},
                 box_MB={k: sd.box_bytes / 1e6 for k, sd in sides.items()})
        rows.append(r)
        log(f"{h}x{w}, batch {batch}: logits of the P010 ring equal the NV12 ring's bit for bit: {same}")
        for k, sd in sides.items():
            m, lo, hi = r["ring"][k]
            log(f"    frames ring, {k.upper():4s}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / r['ring']['nv12'][0]:6.2f} % of the NV12 ring, "
                f"{100 * m / r['ring']['rgb'][0]:6.2f} % of the RGB ring | upload {sd.nbytes / 1e6:7.1f} MB per step = {sd.nbytes * 1e-9 * m / batch:5.1f} GB/s")
        for k, sd in sides.items():
            avg, mb = r["resize_us_avg"][k], sd.box_bytes / 1e6
            t = float(np.mean(avg))
            log(f"    resize {k.upper():4s}: {t:8.1f} us per launch avg ({r['resize_us_min'][k]:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (t * 1e-6):.0f} GB/s")
        for sd in sides.values():
            sd.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "yuv16_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "yuv16_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def yuv420p_main(a):
    import nv12_ref as N
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    title, key, cfg, dname, _, flags, eps = RUNS[0]
    log(f"frames_bench --yuv420p: {title[:-5]}, frames rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (NV12 frames "
        f"against the I420 planes of the same pictures; 0.875 centre box); median pass [min .. max]; images/s")
    for h, w, batch in ((360, 480, 512), (1080, 1920, 64)):
        rng = np.random.default_rng(3)
        small = rng.integers(0, 256, size=(batch, h // 8, w // 8, 3), dtype=np.uint8)
        rgb = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))     # the pictures of --nv12
        rgb ^= rng.integers(0, 8, size=rgb.shape, dtype=np.uint8)
        planes = [N.rgb_to_nv12(f) for f in rgb]
        del rgb
        y, uv = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        box = vithip.center_crop_box(h, w)
        common = (cfg, dname, batch, flags, eps, scale, shift)
        A = SideNV12(*common, y=y, uv=uv, box=box)
        B = SideYUV(*common, y=y, u=np.ascontiguousarray(uv[..., 0]), v=np.ascontiguousarray(uv[..., 1]), box=box)
        same = bool(np.array_equal(A.first.view(np.uint32), B.first.view(np.uint32)) and np.isfinite(A.first).all())
        ra, rb = [], []
        for _ in range(a.passes):
            ra.append(A.ring_rate(a.steps)); rb.append(B.ring_rate(a.steps))
        k = [A.resize_us(8), B.resize_us(8), A.resize_us(8), B.resize_us(8)]
        r = dict(config=key, frame=[h, w], batch=batch, ring_nv12=mid(ra), ring_i420=mid(rb),
                 h2d_MB_per_step=dict(nv12=A.nbytes / 1e6, i420=B.nbytes / 1e6), logits_i420_equal_nv12=same,
                 resize_nv12_us_avg=[k[0][0], k[2][0]], resize_i420_us_avg=[k[1][0], k[3][0]],
                 resize_nv12_us_min=min(k[0][1], k[2][1]), resize_i420_us_min=min(k[1][1], k[3][1]),
                 box_MB=dict(nv12=A.box_bytes / 1e6, i420=B.box_bytes / 1e6))
        rows.append(r)
        base = r["ring_nv12"][0]
        log(f"{h}x{w}, batch {batch}: logits of the I420 ring equal the NV12 ring's bit for bit: {same}")
        for name, kk, mb in (("frames ring, NV12 ", "ring_nv12", A.nbytes / 1e6), ("frames ring, I420 ", "ring_i420", B.nbytes / 1e6)):
            m, lo, hi = r[kk]
            log(f"    {name}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / base:6.2f} % of the NV12 ring | upload {mb:7.1f} MB per step = "
                f"{mb * 1e-3 * m / batch:5.1f} GB/s")
        for name, avg, mn, mb in (("NV12", r["resize_nv12_us_avg"], r["resize_nv12_us_min"], A.box_bytes / 1e6),
                                  ("I420", r["resize_i420_us_avg"], r["resize_i420_us_min"], B.box_bytes / 1e6)):
            us = float(np.mean(avg))
            log(f"    resize {name}: {us:8.1f} us per launch avg ({mn:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (us * 1e-6):.0f} GB/s")
        A.close(); B.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "yuv_planar_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "yuv_planar_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def nv12_main(a):
    import nv12_ref as N
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    title, key, cfg, dname, _, flags, eps = RUNS[0]
    log(f"frames_bench --nv12: {title[:-5]}, frames rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (RGB frames "
        f"against the NV12 frames of the same pictures; 0.875 centre box); median pass [min .. max]; images/s")
    for h, w, batch in ((360, 480, 512), (1080, 1920, 64)):
        rng = np.random.default_rng(3)
        small = rng.integers(0, 256, size=(batch, h // 8, w // 8, 3), dtype=np.uint8)
        rgb = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))     # pictures with structure: 8 x 8 blocks
        rgb ^= rng.integers(0, 8, size=rgb.shape, dtype=np.uint8)                          # plus noise in the low bits
        planes = [N.rgb_to_nv12(f) for f in rgb]
        y, uv = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        box = vithip.center_crop_box(h, w)
        common = (cfg, dname, batch, flags, eps, scale, shift)
        A = Side(*common, frames=rgb, box=box)
        B = SideNV12(*common, y=y, uv=uv, box=box)
        diff = float(np.abs(A.first - B.first).max() / np.abs(A.first).max())
        ra, rb = [], []
        for _ in range(a.passes):
            ra.append(A.ring_rate(a.steps)); rb.append(B.ring_rate(a.steps))
        k = [A.resize_us(8), B.resize_us(8), A.resize_us(8), B.resize_us(8)]
        r = dict(config=key, frame=[h, w], batch=batch, ring_rgb=mid(ra), ring_nv12=mid(rb),
                 h2d_MB_per_step=dict(rgb=A.nbytes / 1e6, nv12=B.nbytes / 1e6), logits_rel_diff_rgb_vs_nv12=diff,
                 resize_rgb_us_avg=[k[0][0], k[2][0]], resize_nv12_us_avg=[k[1][0], k[3][0]],
                 resize_rgb_us_min=min(k[0][1], k[2][1]), resize_nv12_us_min=min(k[1][1], k[3][1]),
                 box_MB=dict(rgb=A.box_bytes / 1e6, nv12=B.box_bytes / 1e6))
        rows.append(r)
        base = r["ring_rgb"][0]
        log(f"{h}x{w}, batch {batch}: logits of the NV12 ring differ from the RGB ring's by {diff:.3e} of the largest logit (4:2:0 subsampling and "
            f"the 8-bit round trip of the test pictures; not a parity figure)")
        for name, kk, mb in (("frames ring, RGB  ", "ring_rgb", A.nbytes / 1e6), ("frames ring, NV12 ", "ring_nv12", B.nbytes / 1e6)):
            m, lo, hi = r[kk]
            log(f"    {name}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / base:6.2f} % of the RGB ring | upload {mb:7.1f} MB per step = "
                f"{mb * 1e-3 * m / batch:5.1f} GB/s")
        for name, avg, mn, mb in (("RGB ", r["resize_rgb_us_avg"], r["resize_rgb_us_min"], A.box_bytes / 1e6),
                                  ("NV12", r["resize_nv12_us_avg"], r["resize_nv12_us_min"], B.box_bytes / 1e6)):
            us = float(np.mean(avg))
            log(f"    resize {name}: {us:8.1f} us per launch avg ({mn:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (us * 1e-6):.0f} GB/s")
        A.close(); B.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "nv12_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "nv12_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def mid(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--nv12", action="store_true", help="the NV12 passes (RGB frames ring against NV12 frames ring) instead")
    ap.add_argument("--yuv420p", action="store_true", help="the planar passes (NV12 frames ring against I420 frames ring) instead")
    ap.add_argument("--p010", action="store_true", help="the 10-bit passes (RGB, NV12 and P010 frames rings of the same pictures) instead")
    ap.add_argument("--yuy2", action="store_true", help="the packed 4:2:2 passes (RGB, NV12, planar 4:2:2, YUY2 and v210 frames rings) instead")
    ap.add_argument("--bgra", action="store_true", help="the packed 4:4:4 passes (RGB, BGRA, planar 4:4:4, VUYA and Y410 frames rings) instead")
    a = ap.parse_args()
    if a.bgra:
        return bgra_main(a)
    if a.yuy2:
        return yuy2_main(a)
    if a.p010:
        return p010_main(a)
    if a.yuv420p:
        return yuv420p_main(a)
    if a.nv12:
        return nv12_main(a)
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    scale, shift = vithip.input_norm_from_mean_std(MEAN, STD)
    log(f"frames_bench: rings of {SLOTS} slots, {a.steps} steps per pass, {a.passes} interleaved passes (u8 ring 224x224, frames ring "
        f"256x256, frames ring 360x480; 0.875 centre box); median pass [min .. max]; images/s")
    for title, key, cfg, dname, batch, flags, eps in RUNS:
        if a.only and a.only != key:
            continue
        rng = np.random.default_rng(3)
        f256 = rng.integers(0, 256, size=(batch, 256, 256, 3), dtype=np.uint8)
        f360 = rng.integers(0, 256, size=(batch, 360, 480, 3), dtype=np.uint8)
        crops = np.ascontiguousarray(f256[:, 16:240, 16:240])
        common = (cfg, dname, batch, flags, eps, scale, shift)
        U = Side(*common, images=crops)
        A = Side(*common, frames=f256, box=vithip.center_crop_box(256, 256))
        B = Side(*common, frames=f360, box=vithip.center_crop_box(360, 480))
        same = bool(np.array_equal(U.first.view(np.uint32), A.first.view(np.uint32)) and np.isfinite(U.first).all())
        ru, ra, rb = [], [], []
        for _ in range(a.passes):
            ru.append(U.ring_rate(a.steps)); ra.append(A.ring_rate(a.steps)); rb.append(B.ring_rate(a.steps))
        k = [A.resize_us(8), B.resize_us(8), A.resize_us(8), B.resize_us(8)]
        r = dict(config=key, title=title, batch=batch, dtype=dname, logits_256_equal_u8_ring=same,
                 ring_u8=mid(ru), ring_frames_256=mid(ra), ring_frames_360x480=mid(rb),
                 h2d_MB_per_step=dict(u8=U.nbytes / 1e6, frames_256=A.nbytes / 1e6, frames_360x480=B.nbytes / 1e6),
                 resize_256_us_avg=[k[0][0], k[2][0]], resize_360x480_us_avg=[k[1][0], k[3][0]],
                 resize_256_us_min=min(k[0][1], k[2][1]), resize_360x480_us_min=min(k[1][1], k[3][1]),
                 resize_launches=k[0][2], box_MB=dict(frames_256=A.box_bytes / 1e6, frames_360x480=B.box_bytes / 1e6))
        rows.append(r)
        base = r["ring_u8"][0]
        log(f"{title}: logits of the 256x256 frames ring equal the u8 ring's on the centre crops: {same}")
        for name, kk, mb in (("u8 ring, 224x224     ", "ring_u8", U.nbytes / 1e6), ("frames ring, 256x256 ", "ring_frames_256", A.nbytes / 1e6),
                             ("frames ring, 360x480 ", "ring_frames_360x480", B.nbytes / 1e6)):
            m, lo, hi = r[kk]
            log(f"    {name}: {m:9.0f} [{lo:9.0f} .. {hi:9.0f}] = {100 * m / base:6.2f} % of the u8 ring | upload {mb:6.1f} MB per step = "
                f"{mb * 1e-3 * m / batch:5.1f} GB/s")
        for name, avg, mn, mb in (("256x256", r["resize_256_us_avg"], r["resize_256_us_min"], A.box_bytes / 1e6),
                                  ("360x480", r["resize_360x480_us_avg"], r["resize_360x480_us_min"], B.box_bytes / 1e6)):
            us = float(np.mean(avg))
            log(f"    resize {name}: {us:8.1f} us per launch avg ({mn:.1f} min; passes {avg[0]:.1f} {avg[1]:.1f}; {r['resize_launches']} launches) | "
                f"{mb:.1f} MB inside the boxes = {mb * 1e-3 / (us * 1e-6):.0f} GB/s | {100 * us * 1e-6 * base / batch:.2f} % of a u8-ring step")
        U.close(); A.close(); B.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "frames_host_path.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "frames_host_path.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
