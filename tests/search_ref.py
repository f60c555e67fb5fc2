"""The embedding search in numpy (include/vithip.h, "Embedding search"): float64 scores of the operands as the device holds them
(rounded to nearest even to the 16-bit type), ordered by the total order (score descending, index ascending)."""
import numpy as np

import vithip


def operand(a, dtype):
    """The 16-bit image of fp32 values, as float64."""
    return vithip.from16(vithip.to16(np.ascontiguousarray(a, dtype=np.float32), dtype), dtype).astype(np.float64)


def unit_rows(a):
    """Rows divided by their L2 norm in float64, the sum taken j ascending (the library's host loop); a zero row stays zero."""
    a = np.asarray(a, dtype=np.float64)
    ss = np.cumsum(a * a, axis=1)[:, -1:]
    return a * np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 1.0)


def scores(q, b, dtype, normalise=False):
    """[nq, n] float64 scores of fp32 queries q (normalised in float64 first, if asked) against bank rows b."""
    return operand(unit_rows(q) if normalise else q, dtype) @ operand(b, dtype).T


def topk(s, k):
    """(index [nq, k] int32, score [nq, k] float64) of the first k columns of s per row; the tail beyond n is -1 / -inf."""
    nq, n = s.shape
    index, score = np.full((nq, k), -1, np.int32), np.full((nq, k), -np.inf)
    for i in range(nq):
        cand = np.flatnonzero(s[i] >= np.partition(s[i], n - k)[n - k]) if n > k else np.arange(n)   # (only these can be among the k)
        order = cand[np.lexsort((cand, -s[i][cand]))][:k]
        index[i, :order.size], score[i, :order.size] = order, s[i, order]
    return index, score
