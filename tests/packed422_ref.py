"""Packed 4:2:2 frames (include/vithip.h, "Packed 4:2:2 frames") in numpy: memory layouts only.

A packed frame is the planar 4:2:2 frame (sub_x = 2, sub_y = 1) of its de-interleaved planes in another memory layout, so the
reference of every byte is yuv_ref.resize_yuv_f32 of those planes and nothing here does arithmetic.  interleave / deinterleave: the
four macropixel orders, for uint8 samples or uint16 words.  to_v210 / from_v210: 10-bit codes in v210 blocks.  lay_out: frames into
one buffer with lead bytes, row padding and gaps, as lay_out / lay_out16 of the GPU planar tests do for planes."""
import numpy as np

import vithip

YUYV, UYVY, YVYU, VYUY, V210 = vithip.L422_YUYV, vithip.L422_UYVY, vithip.L422_YVYU, vithip.L422_VYUY, vithip.L422_V210
NAMES = {YUYV: "yuyv", UYVY: "uyvy", YVYU: "yvyu", VYUY: "vyuy", V210: "v210"}
SUB = (2, 1)
# positions of (Y0, U, Y1, V) among the four samples of a macropixel, written out per layout
ORDER = {YUYV: (0, 1, 2, 3), UYVY: (1, 0, 3, 2), YVYU: (0, 3, 2, 1), VYUY: (1, 2, 3, 0)}
# sample slots of one v210 block: (plane, index within the block's 6 luma / 3 chroma samples), three to a 32-bit word
V210_SLOTS = [("u", 0), ("y", 0), ("v", 0), ("y", 1), ("u", 1), ("y", 2), ("v", 1), ("y", 3), ("u", 2), ("y", 4), ("v", 2), ("y", 5)]
FILL = 0xEE


def cw_of(w):
    return (w + 1) // 2


def interleave(y, u, v, layout, fill=0):
    """Y [H, W], U and V [H, cw] (uint8 or uint16) -> [H, 4 cw] samples; with an odd W the second luma of the last macropixel is `fill`."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape
    cw = cw_of(w)
    assert u.shape == (h, cw) and v.shape == (h, cw) and u.dtype == y.dtype and v.dtype == y.dtype
    p0, pu, p1, pv = ORDER[layout]
    m = np.full((h, cw, 4), fill, y.dtype)
    m[:, :, p0] = y[:, 0::2]
    m[:, :w // 2, p1] = y[:, 1::2]
    m[:, :, pu] = u
    m[:, :, pv] = v
    return m.reshape(h, 4 * cw)


def deinterleave(rows, w, layout):
    """The inverse: [H, >= 4 cw] samples -> (Y [H, w], U [H, cw], V [H, cw])."""
    rows = np.asarray(rows)
    h, cw = rows.shape[0], cw_of(w)
    p0, pu, p1, pv = ORDER[layout]
    m = rows[:, :4 * cw].reshape(h, cw, 4)
    y = np.empty((h, 2 * cw), rows.dtype)
    y[:, 0::2], y[:, 1::2] = m[:, :, p0], m[:, :, p1]
    return np.ascontiguousarray(y[:, :w]), np.ascontiguousarray(m[:, :, pu]), np.ascontiguousarray(m[:, :, pv])


def to_v210(y, u, v, high_bits=0):
    """Y [H, W], U and V [H, cw] uint16 codes 0..1023 -> [H, 4 ceil(W / 6)] uint32 words; the unused slots of the last block are zero,
    bits 30-31 of every word are `high_bits` (0..3; the format ignores them)."""
    y, u, v = (np.asarray(p) for p in (y, u, v))
    h, w = y.shape
    cw, blocks = cw_of(w), (w + 5) // 6
    assert u.shape == (h, cw) and v.shape == (h, cw) and max(int(y.max()), int(u.max()), int(v.max())) <= 1023
    pad = {"y": np.zeros((h, 6 * blocks), np.uint32), "u": np.zeros((h, 3 * blocks), np.uint32), "v": np.zeros((h, 3 * blocks), np.uint32)}
    pad["y"][:, :w], pad["u"][:, :cw], pad["v"][:, :cw] = y, u, v
    words = np.full((h, blocks, 4), np.uint32(high_bits) << np.uint32(30), np.uint32)
    for slot, (plane, k) in enumerate(V210_SLOTS):
        per_block = 6 if plane == "y" else 3
        words[:, :, slot // 3] |= pad[plane][:, k::per_block] << np.uint32(10 * (slot % 3))
    return words.reshape(h, 4 * blocks)


def from_v210(words, w):
    """The inverse: [H, >= 4 ceil(w / 6)] uint32 words -> (Y [H, w], U [H, cw], V [H, cw]) uint16 codes; bits 30-31 dropped."""
    words = np.asarray(words, np.uint32)
    h, cw, blocks = words.shape[0], cw_of(w), (w + 5) // 6
    blk = words[:, :4 * blocks].reshape(h, blocks, 4)
    out = {"y": np.zeros((h, 6 * blocks), np.uint16), "u": np.zeros((h, 3 * blocks), np.uint16), "v": np.zeros((h, 3 * blocks), np.uint16)}
    for slot, (plane, k) in enumerate(V210_SLOTS):
        per_block = 6 if plane == "y" else 3
        out[plane][:, k::per_block] = (blk[:, :, slot // 3] >> np.uint32(10 * (slot % 3))) & np.uint32(0x3FF)
    return np.ascontiguousarray(out["y"][:, :w]), np.ascontiguousarray(out["u"][:, :cw]), np.ascontiguousarray(out["v"][:, :cw])


def row_bytes(y, u, v, layout, high_bits=0):
    """The rows of one frame as [H, n] bytes, words little-endian, nothing padded: n = 4 cw (uint8), 8 cw (uint16) or 16 ceil(W / 6)."""
    if layout == V210:
        a = to_v210(y, u, v, high_bits).astype("<u4")
    else:
        a = interleave(y, u, v, layout, fill=FILL if np.asarray(y).dtype == np.uint8 else 0xEEEE)
        a = np.ascontiguousarray(a, a.dtype.newbyteorder("<"))
    return a.view(np.uint8).reshape(a.shape[0], -1)


def lay_out(planes, boxes, layouts, pad=0, lead=0, gap=0, high_bits=0):
    """(Y, U, V) triples -> (one uint8 buffer, the (FrameYUY2 * n) descriptors): `lead` bytes in front, `gap` bytes behind every
    frame, every row but a frame's last padded by `pad` bytes (so the buffer ends with the last macropixel), one layout per frame
    (or one for all).  Filler bytes are 0xEE."""
    if isinstance(layouts, int):
        layouts = [layouts] * len(planes)
    desc = (vithip.FrameYUY2 * len(planes))()
    chunks, off = [np.full(lead, FILL, np.uint8)], lead
    for i, ((y, u, v), box, lay) in enumerate(zip(planes, boxes, layouts)):
        rows = row_bytes(y, u, v, lay, high_bits)
        h, n = rows.shape
        stride = n + pad
        buf = np.full((h, stride), FILL, np.uint8)
        buf[:, :n] = rows
        flat = buf.reshape(-1)[:(h - 1) * stride + n]
        d = desc[i]
        d.offset, d.height, d.width, d.row_stride, d.layout = off, h, np.asarray(y).shape[1], stride, lay
        d.box[:] = (0.0, 0.0, float(d.width), float(h)) if box is None else box
        chunks += [flat, np.full(gap, FILL, np.uint8)]
        off += flat.size + gap
    return np.concatenate(chunks), desc
