"""CPU suite of the label propagation (include/vithip.h, "Label propagation"): the symbols, the tap's refusals (which need no device),
and the reference's window and tie order on a hand-written 3 x 3 case."""
import ctypes as C
import os

import numpy as np
import pytest

import propagate_ref as PR
import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, ITEMS, LABELS, OUT, IDX, SCORE = (0x10000 * i for i in range(1, 7))   # never dereferenced: the tap refuses before a device
SYMBOLS = ["vh_propagate_labels", "vh_propagate_labels_device", "vh_propagate_labels_device_async", "vh_op_propagate"]
REFUSALS = {"null rows": [dict(rows_ptr=None)],
            "null item list": [dict(items_ptr=None)],
            "null labels or out": [dict(labels_ptr=None), dict(out_ptr=None)],
            "dtype is not": [dict(dtype=vithip.DTYPE_FP8)],
            "images is outside": [dict(images=0), dict(images=(1 << 20) + 1)],
            "gh \\* gw is above 4096": [dict(gh=0), dict(gw=0), dict(gh=65, gw=64)],
            "width is not a multiple of 64": [dict(width=0), dict(width=96), dict(width=2112)],
            "nitems is outside": [dict(nitems=0), dict(nitems=65537)],
            "nsrc is outside": [dict(nsrc=0), dict(nsrc=9)],
            "k is outside": [dict(k=0), dict(k=17)],
            "radius is outside": [dict(radius=-1), dict(radius=4097)],
            "tau is not finite and positive": [dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan"))],
            "classes is outside": [dict(classes=0), dict(classes=257)],
            "not 16-byte aligned": [dict(rows_ptr=ROWS + 8), dict(items_ptr=ITEMS + 4), dict(out_ptr=OUT + 4), dict(idx_ptr=IDX + 8),
                                    dict(score_ptr=SCORE + 4)]}


def test_header_and_symbol_table_agree():
    header = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert "/* ---- Label propagation" in header
    for name in SYMBOLS:
        assert f" {name}(" in header and name in vithip.SYMBOLS and hasattr(vithip.lib(), name), name
    assert C.sizeof(vithip.PropagateDesc) == 40


@pytest.mark.parametrize("text", list(REFUSALS))
def test_tap_refuses_before_touching_a_device(text):
    for kw in REFUSALS[text]:
        a = dict(rows_ptr=ROWS, dtype=vithip.DTYPE_BF16, images=8, gh=14, gw=14, width=768, items_ptr=ITEMS, nitems=2, nsrc=7, k=5, radius=0,
                 tau=0.1, labels_ptr=LABELS, classes=3, out_ptr=OUT, idx_ptr=IDX, score_ptr=SCORE)
        a.update(kw)
        with pytest.raises(vithip.VhError, match="propagate: .*" + text) as e:
            vithip.op_propagate(**a)
        assert e.value.code == VH_ERR_INVALID


def test_reference_window_and_tie_order_by_hand():
    """A 3 x 3 grid, radius 1, two slots of the same image, every score equal: the corner patch 0 sees patches {0, 1, 3, 4}, the
    centre all nine; equal scores come out in ascending id, slot 0 before slot 1; an absent slot contributes nothing."""
    rows = np.ones((1, 9, 4))
    s = PR.scores(rows, (0, 0, 0), 3, 3, 1)
    idx, score = PR.select(s, 6)
    assert idx[0].tolist() == [0, 1, 3, 4, 9, 10] and idx[4].tolist() == [0, 1, 2, 3, 4, 5] and (score == 4.0).all()
    assert idx[8].tolist() == [4, 5, 7, 8, 13, 14]
    idx, score = PR.select(PR.scores(rows, (0, -1, 0), 3, 3, 1), 6)
    assert idx[0].tolist() == [9, 10, 12, 13, -1, -1] and score[0].tolist() == [4.0] * 4 + [-np.inf] * 2
    s[2, 14] = 5.0   # a better score wins over a lower id
    assert PR.select(s, 2)[0][2].tolist() == [14, 1]
    labels = np.arange(9.0).reshape(1, 9, 1)
    out = PR.vote(*PR.select(PR.scores(rows, (0, -1, 0), 3, 3, 1), 6), (0, -1, 0), labels, 0.1)
    assert out[0, 0] == (0 + 1 + 3 + 4) / 4 and out[4, 0] == (0 + 1 + 2 + 3 + 4 + 5) / 6
