"""CPU suite of the embedding search (include/vithip.h, "Embedding search"): the refusals that need no device, the launcher's split,
the agreement of the header with the binding's symbol table, and the k-NN vote."""
import ctypes as C
import os

import numpy as np
import pytest

import vithip

VH_ERR_INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# device pointers that are never dereferenced: the tap refuses before it touches a device
ROWS, BANK, WS, INDEX, SCORE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
SEARCH_SYMBOLS = ["vh_set_bank", "vh_bank_dims", "vh_search_bank", "vh_search_bank_device", "vh_search_bank_device_async", "vh_op_search",
                  "vh_op_search_workspace_bytes", "vh_op_search_slabs"]


def tap(**kw):
    a = dict(rows_ptr=ROWS, nq=8, width=768, normalise=1, bank_ptr=BANK, n=5000, dtype=vithip.DTYPE_BF16, k=20, workspace_ptr=WS,
             index_ptr=INDEX, score_ptr=SCORE)
    a.update(kw)
    vithip.op_search(**a)


REFUSALS = [dict(rows_ptr=None), dict(bank_ptr=None), dict(workspace_ptr=None), dict(index_ptr=None), dict(score_ptr=None),
            dict(dtype=vithip.DTYPE_FP8), dict(width=0), dict(width=776), dict(width=4112), dict(n=0), dict(n=(1 << 28) + 1),
            dict(nq=0), dict(nq=4097), dict(k=0), dict(k=33), dict(normalise=2), dict(rows_ptr=ROWS + 4), dict(score_ptr=SCORE + 8)]
SHARED = 7   # both outputs, three ways out of the width, both ends of n, nq and k, two pointers: 18 causes, 11 messages


def message(kw):
    with pytest.raises(vithip.VhError) as e:
        tap(**kw)
    assert e.value.code == VH_ERR_INVALID, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("kw", REFUSALS, ids=[str(k) for k in REFUSALS])
def test_tap_refuses_before_touching_a_device(kw):
    assert "search: " in message(kw)


def test_refusals_with_different_causes_have_different_messages():
    assert len({message(kw) for kw in REFUSALS}) == len(REFUSALS) - SHARED


def test_context_calls_refuse_a_null_context():
    L = vithip.lib()
    d = vithip.Search(vithip.SEARCH_ROWS, 5, 1, 1, ROWS, INDEX, SCORE)
    calls = [lambda: L.vh_set_bank(None, BANK, 10, 16, vithip.ELEM_F32, 1), lambda: L.vh_bank_dims(None, None, None),
             lambda: L.vh_search_bank(None, C.byref(d)), lambda: L.vh_search_bank_device(None, C.byref(d)),
             lambda: L.vh_search_bank_device_async(None, C.byref(d))]
    for call in calls:
        assert call() == VH_ERR_INVALID
        assert b"null context" in L.vh_last_error(None)


def test_split_and_workspace():
    assert vithip.op_search_slabs(200, 70001) > 1 and vithip.op_search_slabs(33, 4129) > 1 and vithip.op_search_slabs(512, 1000) == 1
    assert vithip.op_search_slabs(0, 1000) == 0 and vithip.op_search_workspace_bytes(8, 0, 5) == 0
    for nq, n, k in ((1, 1, 1), (200, 70001, 32), (4096, 1 << 28, 32)):
        slabs, nq_pad = vithip.op_search_slabs(nq, n), (nq + 63) // 64 * 64
        assert 1 <= slabs <= 256   # the merge holds four list heads per lane
        assert vithip.op_search_workspace_bytes(nq, n, k) >= nq_pad * (slabs * k * 8 + 2 * vithip.SEARCH_MAX_WIDTH)


def test_header_and_symbol_table_agree():
    header = open(os.path.join(ROOT, "include", "vithip.h")).read()
    assert "/* ---- Embedding search" in header and "#define VH_ABI_VERSION 1\n" in header
    for name in SEARCH_SYMBOLS:
        assert f" {name}(" in header and name in vithip.SYMBOLS and hasattr(vithip.lib(), name), name
    assert {n for n in vithip.SYMBOLS if "search" in n or "bank" in n} == set(SEARCH_SYMBOLS)
    assert C.sizeof(vithip.Search) == 40


def test_knn_vote_against_a_literal_loop():
    rng = np.random.default_rng(2)
    index, score = rng.integers(-1, 50, (7, 10)), rng.uniform(-1, 1, (7, 10)).astype(np.float32)
    labels = rng.integers(0, 6, 50)
    votes = np.zeros((7, 6))
    for i in range(7):
        for j in range(10):
            if index[i, j] >= 0:
                votes[i, labels[index[i, j]]] += np.exp(float(score[i, j]) / 0.07)
    pred, got = vithip.knn_vote(index, score, labels, 6)
    assert np.allclose(got, votes, rtol=1e-12, atol=0) and np.array_equal(pred, votes.argmax(axis=1))


def test_measurement_tool_compiles():
    import py_compile
    py_compile.compile(os.path.join(ROOT, "tools", "search_bench.py"), doraise=True)
