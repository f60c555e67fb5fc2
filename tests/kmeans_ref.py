"""Patch clustering in numpy (include/vithip.h, "Patch clustering"): the function in float64 on the operand rows as the device holds
them, with the centroids rounded to the 16-bit type after every update, and the update's division and root emulated in fp32."""
import numpy as np

import match_ref as MR


def stride_rows(np_rows, k):
    """The rows the stride init takes: floor((2 j + 1) np / (2 k))."""
    return [((2 * j + 1) * np_rows) // (2 * k) for j in range(k)]


def assign(x, c, l2):
    """(labels int32, counts int32, margin): s = x . c (- 0.5 |c|^2 for L2) in float64, the first maximum per row (ties to the lower
    index); margin = the smallest gap between a row's best and second-best score."""
    s = x @ c.T - (0.5 * (c * c).sum(axis=1) if l2 else 0.0)
    labels = s.argmax(axis=1).astype(np.int32)
    top = np.sort(s, axis=1)
    return labels, np.bincount(labels, minlength=c.shape[0]).astype(np.int32), float((top[:, -1] - top[:, -2]).min())


def update(x, labels, c, l2, dtype, fp32):
    """The new centroids, rounded to `dtype`.  fp32: sums, the sum of squares, the root and the quotients in float32 (exact sums are the
    caller's to assert); else float64 throughout.  An empty cluster, or one whose sums are all zero, keeps its centroid."""
    f = np.float32 if fp32 else np.float64
    out = c.copy()
    for j in range(c.shape[0]):
        rows = x[labels == j]
        total = rows.sum(axis=0).astype(f)
        den = f(len(rows)) if l2 else np.sqrt((total * total).sum(dtype=f), dtype=f)
        if len(rows) and den > 0:
            out[j] = MR.round16((total / den).astype(f), dtype)
    return out


def kmeans(x, k, iters, l2, dtype, init=None, fp32=False):
    """One image x [np, W] (values exact in `dtype`): (labels, centroids, counts, smallest margin over all assignments)."""
    c = x[stride_rows(x.shape[0], k)].copy() if init is None else MR.round16(init, dtype)
    margin = np.inf
    for it in range(iters + 1):
        labels, counts, m = assign(x, c, l2)
        margin = min(margin, m)
        if it < iters:
            c = update(x, labels, c, l2, dtype, fp32)
    return labels, c, counts, margin
