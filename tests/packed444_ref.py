"""Packed 4:4:4 frames (include/vithip.h, "Packed 4:4:4 frames") in numpy: memory layouts only.

A packed 4:4:4 frame is the planar 4:4:4 frame (sub_x = sub_y = 1) of its de-interleaved samples in another memory layout, so the
reference of every byte is yuv_ref.resize_yuv_f32 of those planes (YUV layouts) or frames_ref on the RGB-ordered frame (RGB layouts)
and nothing here does arithmetic.  interleave / deinterleave: three components into pixels of three or four samples at the positions
of a VH_444 word, for uint8 samples or uint16 words.  to_y410 / to_v410 (and from_word10): 10-bit codes in one 32-bit word per pixel.
lay_out: frames into one buffer with lead bytes, row padding and gaps."""
import numpy as np

import vithip

V = vithip
RGB, BGR, RGBA, BGRA, ARGB, ABGR = V.L444_RGB, V.L444_BGR, V.L444_RGBA, V.L444_BGRA, V.L444_ARGB, V.L444_ABGR
YUV24, VUYA, AYUV, Y416, AYUV64, Y410, V410 = V.L444_YUV24, V.L444_VUYA, V.L444_AYUV, V.L444_Y416, V.L444_AYUV64, V.L444_Y410, V.L444_V410
RGB_LAYOUTS = {"rgb": RGB, "bgr": BGR, "rgba": RGBA, "bgra": BGRA, "argb": ARGB, "abgr": ABGR}
YUV_LAYOUTS = {"yuv24": YUV24, "vuya": VUYA, "ayuv": AYUV}
WORD_LAYOUTS = {"y416": Y416, "ayuv64": AYUV64}
# memory order of the samples of a pixel, written out per name ("x": the unread 4th sample); the component that becomes output
# channel k is "rgb"[k] or "yuv"[k]
ORDER = {RGB: "rgb", BGR: "bgr", RGBA: "rgbx", BGRA: "bgrx", ARGB: "xrgb", ABGR: "xbgr", YUV24: "yuv", VUYA: "vuyx", AYUV: "xyuv", Y416: "uyvx"}
SUB = (1, 1)
FILL = 0xEE


def is_yuv(layout):
    return bool(layout & 128)


def samples(layout):
    return 4 if layout & 64 else 3


def positions(layout):
    return [(layout >> (2 * k)) & 3 for k in range(3)]


def pixel_bytes(layout, sample_bytes):
    return 4 if layout & 256 else samples(layout) * sample_bytes


def interleave(c0, c1, c2, layout, fill=0):
    """Three [H, W] planes in output order (uint8 or uint16) -> [H, ns W] samples, ns = 3 or 4; the 4th sample is `fill`."""
    comps = [np.asarray(p) for p in (c0, c1, c2)]
    h, w = comps[0].shape
    assert all(p.shape == (h, w) and p.dtype == comps[0].dtype for p in comps) and not layout & 256
    ns = samples(layout)
    m = np.full((h, w, ns), fill, comps[0].dtype)
    for p, at in zip(comps, positions(layout)):
        assert at < ns
        m[:, :, at] = p
    return m.reshape(h, ns * w)


def deinterleave(rows, w, layout):
    """The inverse: [H, >= ns w] samples -> three [H, w] planes in output order."""
    rows = np.asarray(rows)
    ns = samples(layout)
    m = rows[:, :ns * w].reshape(rows.shape[0], w, ns)
    return tuple(np.ascontiguousarray(m[:, :, at]) for at in positions(layout))


def to_y410(y, u, v, ignored=0):
    """[H, W] uint16 codes 0..1023 -> [H, W] uint32 words: U bits 0-9, Y 10-19, V 20-29; bits 30-31 are `ignored` (0..3)."""
    y, u, v = (np.asarray(p).astype(np.uint32) for p in (y, u, v))
    assert max(int(y.max()), int(u.max()), int(v.max())) <= 1023
    return u | (y << np.uint32(10)) | (v << np.uint32(20)) | (np.uint32(ignored) << np.uint32(30))


def to_v410(y, u, v, ignored=0):
    """[H, W] uint16 codes 0..1023 -> [H, W] uint32 words: U bits 2-11, Y 12-21, V 22-31; bits 0-1 are `ignored` (0..3)."""
    y, u, v = (np.asarray(p).astype(np.uint32) for p in (y, u, v))
    assert max(int(y.max()), int(u.max()), int(v.max())) <= 1023
    return (u << np.uint32(2)) | (y << np.uint32(12)) | (v << np.uint32(22)) | np.uint32(ignored)


def from_word10(words, layout):
    """The inverse of both: [H, W] uint32 words -> (Y, U, V) uint16 codes; the ignored bits dropped."""
    words = np.asarray(words, np.uint32)
    lsb = 2 if layout == V410 else 0
    return tuple(((words >> np.uint32(s + lsb)) & np.uint32(0x3FF)).astype(np.uint16) for s in (10, 0, 20))


def row_bytes(comps, layout, ignored=0):
    """The rows of one frame as [H, n] bytes, words little-endian, nothing padded: n = 3 W or 4 W (uint8), 8 W (uint16), 4 W (10-bit)."""
    if layout & 256:
        a = (to_v410 if layout == V410 else to_y410)(*comps, ignored).astype("<u4")
    else:
        a = interleave(*comps, layout, fill=FILL if np.asarray(comps[0]).dtype == np.uint8 else 0xEEEE)
        a = np.ascontiguousarray(a, a.dtype.newbyteorder("<"))
    return a.view(np.uint8).reshape(a.shape[0], -1)


def lay_out(frames, boxes, layouts, pad=0, lead=0, gap=0, ignored=0, last_gap=True):
    """Component triples in output order -> (one uint8 buffer, the (FrameBGRA * n) descriptors): `lead` bytes in front, `gap` bytes
    behind every frame (last_gap False: none behind the last, so the buffer ends with the last pixel), every row but a frame's last
    padded by `pad` bytes, one layout per frame (or one for all).  Filler bytes are 0xEE."""
    if isinstance(layouts, int):
        layouts = [layouts] * len(frames)
    desc = (vithip.FrameBGRA * len(frames))()
    chunks, off = [np.full(lead, FILL, np.uint8)], lead
    for i, (comps, box, lay) in enumerate(zip(frames, boxes, layouts)):
        rows = row_bytes(comps, lay, ignored)
        h, n = rows.shape
        stride = n + pad
        buf = np.full((h, stride), FILL, np.uint8)
        buf[:, :n] = rows
        flat = buf.reshape(-1)[:(h - 1) * stride + n]
        g = gap if last_gap or i + 1 < len(frames) else 0
        d = desc[i]
        d.offset, d.height, d.width, d.row_stride, d.layout = off, h, np.asarray(comps[0]).shape[1], stride, lay
        d.box[:] = (0.0, 0.0, float(d.width), float(h)) if box is None else box
        chunks += [flat, np.full(g, FILL, np.uint8)]
        off += flat.size + g
    return np.concatenate(chunks), desc
