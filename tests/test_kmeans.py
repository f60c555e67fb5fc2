"""CPU suite of the patch clustering (include/vithip.h, "Patch clustering"): the symbols, the descriptor's size and the refusals that
need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, INIT, LAB, CENT, CNT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # never dereferenced: the tap refuses before it touches a device
SYMBOLS = ["vh_cluster_patches", "vh_cluster_patches_device", "vh_cluster_patches_device_async", "vh_op_kmeans"]
REFUSALS = {"null rows": [dict(x_ptr=None)],
            "null output": [dict(labels_ptr=None), dict(cent_ptr=None)],
            "dtype is not": [dict(dtype=vithip.DTYPE_FP8)],
            "metric is not": [dict(metric=2)],
            "n is outside 1..65536": [dict(n=0), dict(n=65537)],
            "np is outside 1..4096": [dict(np_rows=0), dict(np_rows=4097)],
            "width is not a multiple of 64": [dict(width=0), dict(width=96), dict(width=2112)],
            "k is outside 2..64": [dict(k=1), dict(k=65)],
            "k exceeds np": [dict(k=8, np_rows=7)],
            "iters is outside 0..64": [dict(iters=-1), dict(iters=65)],
            "not 16-byte aligned": [dict(x_ptr=X + 8), dict(init_ptr=INIT + 2), dict(labels_ptr=LAB + 4), dict(cent_ptr=CENT + 8),
                                    dict(counts_ptr=CNT + 4)]}


def test_header_and_symbol_table_agree():
    header = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert "/* ---- Patch clustering" in header
    for name in SYMBOLS:
        assert f" {name}(" in header and name in vithip.SYMBOLS and hasattr(vithip.lib(), name), name
    assert C.sizeof(vithip.KmeansDesc) == 32
    assert (vithip.KMEANS_COSINE, vithip.KMEANS_L2, vithip.KMEANS_INIT_STRIDE, vithip.KMEANS_INIT_GIVEN) == (0, 1, 0, 1)


@pytest.mark.parametrize("text", list(REFUSALS))
def test_tap_refuses_before_touching_a_device(text):
    for kw in REFUSALS[text]:
        a = dict(x_ptr=X, dtype=vithip.DTYPE_BF16, n=2, np_rows=196, width=768, k=8, iters=10, metric=vithip.KMEANS_L2, init_ptr=INIT,
                 labels_ptr=LAB, cent_ptr=CENT, counts_ptr=CNT)
        a.update(kw)
        with pytest.raises(vithip.VhError, match="kmeans: .*" + text) as e:
            vithip.op_kmeans(**a)
        assert e.value.code == VH_ERR_INVALID


def test_descriptor_call_refuses_a_null_context():
    d = vithip.KmeansDesc(0, -1, 0, 8, 10, 0, 1, 0)
    assert vithip.lib().vh_cluster_patches(None, C.byref(d), X, None, LAB, None, None) == VH_ERR_INVALID
    assert b"cluster_patches: null context" in vithip.lib().vh_last_error(None)


def test_segment_masks_are_one_hot():
    labels = np.array([[[0, 2], [1, -1]]])
    m = vithip.segment_masks(labels, 3)
    assert m.shape == (1, 3, 2, 2) and m.dtype == bool
    assert m[0, :, 0, 1].tolist() == [False, False, True] and not m[0, :, 1, 1].any() and m.sum() == 3
