"""Reference and generators of the image-tensor input path (include/vithip.h, "Image tensors").

An image tensor is dense, of one element type (vithip.ELEM_*) in one layout (vithip.LAYOUT_*).  Element (b, y, x, c) enters the
model as the fp32 value v: the element itself (F32), the element widened exactly (F16 / BF16), or fmaf(p, scale[c], shift[c])
(U8).  tensor_reference returns the NHWC fp32 array of v: the forward of a tensor is DEFINED to have the bits vh_forward gives
for that array, and the patch matrix the bits vh_op_im2col_padded gives for it.

bf16 has no numpy dtype: such a tensor is a uint16 array of bit patterns.  Widening needs no arithmetic: the fp32 with these
16 bits on top and zeros below, uint32(bits) << 16.  float16 -> float32 in numpy is exact for every value (subnormals and
infinities included)."""
import numpy as np

import vithip

ELEMS = [vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16, vithip.ELEM_U8]
LAYOUTS = [vithip.LAYOUT_NHWC, vithip.LAYOUT_NCHW]
ELEM_NAME = {vithip.ELEM_F32: "f32", vithip.ELEM_F16: "f16", vithip.ELEM_BF16: "bf16", vithip.ELEM_U8: "u8"}
LAYOUT_NAME = {vithip.LAYOUT_NHWC: "nhwc", vithip.LAYOUT_NCHW: "nchw"}
NUMPY_DTYPE = {vithip.ELEM_F32: np.float32, vithip.ELEM_F16: np.float16, vithip.ELEM_BF16: np.uint16, vithip.ELEM_U8: np.uint8}

# Bit patterns every float generator plants (as_bits order: +0, -0, smallest subnormal, smallest normal, largest finite, +inf,
# -inf), then values that the two operand types round differently
#   f32: 1 + 2^-8 (exact in fp16, a tie in bf16), 1 + 2^-9 + 2^-23 (bf16: 1, fp16: 1 + 2^-9), 65520 (fp16: a tie that goes to inf,
#        bf16: finite), 2^-25 (fp16: a tie that goes to zero, bf16: normal)
SPECIAL_BITS = {
    vithip.ELEM_F32: [0x00000000, 0x80000000, 0x00000001, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                      0x3F808000, 0x3F804001, 0x477FF000, 0x33000000],
    # f16: 1 + 2^-8 and 1 + 2^-8 + 2^-10 (a tie and above it in bf16, exact in fp16), 2^-24 and 65504 (exact in both, at fp16's ends)
    vithip.ELEM_F16: [0x0000, 0x8000, 0x0001, 0x0400, 0x7BFF, 0x7C00, 0xFC00, 0x3C04, 0x3C05],
    # bf16: 2^16 (fp16: inf), 1.5 * 2^-25 (fp16: rounds up to its smallest subnormal), 1 + 2^-7 (exact in both)
    vithip.ELEM_BF16: [0x0000, 0x8000, 0x0001, 0x0080, 0x7F7F, 0x7F80, 0xFF80, 0x4780, 0x3340, 0x3F81],
}
EXTREME = 60000.0   # the forward tests leave out specials of this magnitude or more (see make_tensor)


def to_layout(nhwc, layout):
    """A dense copy of an NHWC array in `layout`."""
    nhwc = np.asarray(nhwc)
    return np.ascontiguousarray(nhwc if layout == vithip.LAYOUT_NHWC else nhwc.transpose(0, 3, 1, 2))


def from_layout(arr, layout):
    """The NHWC view of a dense array in `layout`."""
    arr = np.asarray(arr)
    return arr if layout == vithip.LAYOUT_NHWC else arr.transpose(0, 2, 3, 1)


def widen(arr, elem):
    """The exact fp32 value of every element of a float tensor."""
    arr = np.asarray(arr)
    if elem == vithip.ELEM_F32:
        assert arr.dtype == np.float32
        return arr
    if elem == vithip.ELEM_F16:
        assert arr.dtype == np.float16
        return arr.astype(np.float32)
    assert elem == vithip.ELEM_BF16 and arr.dtype == np.uint16
    return (arr.astype(np.uint32) << np.uint32(16)).view(np.float32)


def assert_norm_in_precondition(scale, shift):
    """The bounds under which u8_reference equals the single-rounding fma exactly (tests/test_u8_input.py's docstring)."""
    scale, shift = np.asarray(scale, dtype=np.float32), np.asarray(shift, dtype=np.float32)
    assert np.isfinite(scale).all() and np.isfinite(shift).all()
    assert (np.abs(scale) >= 2.0 ** -12).all() and (np.abs(scale) < 8).all(), scale
    assert (np.abs(shift) <= 8).all(), shift
    assert ((shift == 0) | (np.abs(shift) >= 2.0 ** -12)).all(), shift


def u8_reference(u8, scale, shift):
    """The fp32 array a u8 forward is defined to consume: [..., C] uint8 -> float32, x = fma(p, scale[c], shift[c])."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8
    scale, shift = np.asarray(scale, dtype=np.float32).reshape(-1), np.asarray(shift, dtype=np.float32).reshape(-1)
    assert scale.shape == shift.shape == (u8.shape[-1],)
    assert_norm_in_precondition(scale, shift)
    return (u8.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)


def make_u8_images(batch, image, channels, seed):
    """[batch, image, image, channels] uint8: every byte value appears, 0 and 255 sit at image corners."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(batch, image, image, channels), dtype=np.uint8)
    row = image * channels
    assert row * (image - 2) >= 256
    a.reshape(-1)[row:row + 256] = np.arange(256, dtype=np.uint8)   # image 0 from row 1 on: clear of the corners
    a[:, 0, 0, :] = 0
    a[:, -1, -1, :] = 255
    a[0, 0, -1, :] = 255
    a[0, -1, 0, :] = 0
    assert len(np.unique(a)) == 256
    return a


def tensor_reference(arr, elem, layout, scale=None, shift=None):
    """The NHWC fp32 array of v for a dense tensor of `elem` in `layout` (scale / shift: [C], ELEM_U8 only)."""
    nhwc = from_layout(arr, layout)
    if elem == vithip.ELEM_U8:
        return np.ascontiguousarray(u8_reference(nhwc, scale, shift))
    return np.ascontiguousarray(widen(nhwc, elem))


def make_tensor(elem, batch, image, channels, seed, extremes=True):
    """An NHWC tensor of `elem` ([batch, image, image, channels] in NUMPY_DTYPE[elem]) with SPECIAL_BITS planted in image 0 (and
    again at the very end of the last image).  extremes=False leaves out the specials of magnitude EXTREME or more (the largest
    finite value, the infinities, what overflows fp16): one such element makes every logit of its image inf or NaN, and a forward
    comparison of NaNs shows nothing -- the operator test carries them.  No NaN anywhere: a NaN's payload is no part of the
    contract (test_gpu_tensor_input.test_nan_positions_survive)."""
    rng = np.random.default_rng(seed)
    shape = (batch, image, image, channels)
    if elem == vithip.ELEM_U8:
        return make_u8_images(batch, image, channels, seed)
    x = rng.standard_normal(shape).astype(np.float32)
    if elem == vithip.ELEM_F32:
        a = x
    elif elem == vithip.ELEM_F16:
        a = x.astype(np.float16)
    else:
        a = (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)   # truncation: any bf16 pattern will do
    bits = a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize]).reshape(-1)
    specials = np.array(SPECIAL_BITS[elem], dtype=bits.dtype)
    if not extremes:
        specials = specials[np.abs(widen(specials.view(a.dtype), elem)) < EXTREME]
    n = len(specials)
    assert bits.size >= 4 * n
    bits[7:7 + n] = specials            # scattered over channels and pixels of the first rows
    bits[-n:] = specials[::-1]          # and the last elements of the tensor
    assert not np.isnan(widen(a, elem)).any()
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))
