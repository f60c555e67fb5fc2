"""Dense correspondence in numpy (include/vithip.h, "Dense correspondence"): float64 scores of the operand rows as the device holds
them, and the argmax whose ties go to the lower index."""
import numpy as np

import vit_ref
import vithip


def round16(a, dtype):
    """Round to nearest even to the 16-bit type; the values as float64."""
    return (vit_ref.bf16(a) if dtype == vithip.DTYPE_BF16 else vit_ref.fp16(a)).astype(np.float64)


def operands(x, dtype, cosine):
    """The operand rows of x [..., W]: RNE16(x), and for the cosine RNE16(x16 / ||x16||), the norm over the ROUNDED row; a zero row stays
    zero.  (The quotient passes fp32 on its way to 16 bits, like the device's: a double rounding the callers' bounds leave room for.)"""
    x16 = round16(x, dtype)
    if not cosine:
        return x16
    n = np.sqrt((x16 * x16).sum(axis=-1, keepdims=True))
    return round16(x16 / np.where(n > 0, n, 1.0), dtype)


def scores(a16, b16):
    """[..., na, nb] float64 inner products of operand rows a16 [..., na, W] and b16 [..., nb, W]."""
    return a16 @ np.swapaxes(b16, -1, -2)


def best(s):
    """(idx int32, score float64) of the largest score per row of s [..., na, nb]; numpy's argmax returns the FIRST maximum: ties go to the
    lower index."""
    idx = s.argmax(axis=-1)
    return idx.astype(np.int32), np.take_along_axis(s, idx[..., None], axis=-1)[..., 0]
