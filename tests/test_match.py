"""CPU suite of the dense correspondence (include/vithip.h, "Dense correspondence"): the symbols, the tap's refusals (which need no
device), the mutual-nearest-neighbour mask and the reference's tie rule."""
import ctypes as C
import os

import numpy as np
import pytest

import match_ref as MR
import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, IDX, SCORE = 0x10000, 0x20000, 0x30000, 0x40000   # never dereferenced: the tap refuses before it touches a device
MATCH_SYMBOLS = ["vh_match_patches", "vh_match_patches_device", "vh_match_patches_device_async", "vh_match_operands", "vh_op_match"]
REFUSALS = {"null rows": [dict(a_ptr=None), dict(b_ptr=None)],
            "null output": [dict(idx_ptr=None), dict(score_ptr=None)],
            "dtype is not": [dict(dtype=vithip.DTYPE_FP8)],
            "metric is not": [dict(metric=2)],
            "npairs is outside": [dict(npairs=0), dict(npairs=65537)],
            "na or nb is outside": [dict(na=0), dict(na=4097), dict(nb=0), dict(nb=4097)],
            "width is not a multiple of 64": [dict(width=0), dict(width=96), dict(width=2112)],
            "not 16-byte aligned": [dict(a_ptr=A + 8), dict(score_ptr=SCORE + 4)]}


def test_header_and_symbol_table_agree():
    header = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert "/* ---- Dense correspondence" in header
    for name in MATCH_SYMBOLS:
        assert f" {name}(" in header and name in vithip.SYMBOLS and hasattr(vithip.lib(), name), name
    assert {n for n in vithip.SYMBOLS if "match" in n} == set(MATCH_SYMBOLS)
    assert C.sizeof(vithip.MatchDesc) == 16


@pytest.mark.parametrize("text", list(REFUSALS))
def test_tap_refuses_before_touching_a_device(text):
    for kw in REFUSALS[text]:
        a = dict(a_ptr=A, b_ptr=B, dtype=vithip.DTYPE_BF16, npairs=2, na=196, nb=196, width=768, metric=vithip.MATCH_DOT, idx_ptr=IDX,
                 score_ptr=SCORE)
        a.update(kw)
        with pytest.raises(vithip.VhError, match="match: .*" + text) as e:
            vithip.op_match(**a)
        assert e.value.code == VH_ERR_INVALID


def test_mutual_matches_by_hand():
    ab = np.array([[2, 0, 0, -1]])      # 0 -> 2, 1 -> 0, 2 -> 0, 3: no match
    ba = np.array([[1, 3, 0, 3]])       # 0 -> 1, 1 -> 3, 2 -> 0, 3 -> 3
    assert vithip.mutual_matches(ab, ba).tolist() == [[True, True, False, False]]


def test_reference_ties_go_to_the_lower_index():
    s = np.array([[1.0, 3.0, 3.0, 2.0], [-5.0, -7.0, -5.0, -9.0], [0.0, 0.0, 0.0, 0.0]])
    idx, score = MR.best(s)
    assert idx.tolist() == [1, 0, 0] and score.tolist() == [3.0, -5.0, 0.0] and idx.dtype == np.int32
