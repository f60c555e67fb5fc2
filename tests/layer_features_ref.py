"""Host reference of the layer features (include/vithip.h, "Layer features"), numpy only, on top of features_ref: which rows of an
image's residual stream each output takes (cls <- row 0, reg <- rows 1 .. lead - 1, patch <- rows lead ..), the channels-first
form of the patch rows (the same elements, transposed), and the canary-guarded device buffer the GPU tests write into."""
import numpy as np

import features_ref as R
import vithip


def outputs(x, lead, gamma=None, beta=None, eps=1e-6):
    """x [B, T, D] fp32 rows as the device reconstructs them -> {"cls" [B, D], "reg" [B, lead - 1, D], "patch" [B, T - lead, D]}:
    the rows themselves (gamma None: exact, fp32) or their fp64 LayerNorm (to be met within features_ref.NORM_BOUND)."""
    x = np.asarray(x)
    assert x.ndim == 3 and 1 <= lead < x.shape[1]
    v = x if gamma is None else R.layernorm64(x, gamma, beta, eps)
    return {"cls": v[:, 0, :], "reg": v[:, 1:lead, :], "patch": v[:, lead:, :]}


def nchw(patch_rows, grid=None):
    """[B, NP, D] -> [B, D, NP] (grid None) or [B, D, gh, gw]: out[b][k][p] = rows[b][p][k], no arithmetic."""
    t = np.ascontiguousarray(np.asarray(patch_rows).transpose(0, 2, 1))
    return t if grid is None else t.reshape(t.shape[0], t.shape[1], grid[0], grid[1])


def rows_of(patch_nchw):
    """The inverse of nchw: [B, D, NP] or [B, D, gh, gw] -> [B, NP, D]."""
    a = np.asarray(patch_nchw)
    a = a.reshape(a.shape[0], a.shape[1], -1)
    return np.ascontiguousarray(a.transpose(0, 2, 1))


NP_DTYPE = {vithip.ELEM_F32: np.float32, vithip.ELEM_F16: np.float16, vithip.ELEM_BF16: np.uint16}


class Guarded:
    """A device buffer with 64 canary bytes in front of and behind the `nbytes` a call may write."""
    CANARY = 0xA5

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = vithip.DeviceBuffer.from_numpy(np.full(self.n + 128, self.CANARY, dtype=np.uint8))
        self.ptr = self.buf.ptr + 64

    def read(self, dtype, shape):
        raw = self.buf.to_numpy(np.uint8, (self.n + 128,))
        assert (raw[:64] == self.CANARY).all() and (raw[64 + self.n:] == self.CANARY).all(), "canary bytes overwritten"
        return raw[64:64 + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.to_numpy(np.uint8, (self.n + 128,)) == self.CANARY).all())

    def free(self):
        self.buf.free()
