"""The float64 reference of the feature moments (include/vithip.h, "Feature moments"): the column sums, X^T X and the row count of
given operand rows."""
import numpy as np


def moments(x):
    """(sum [W], gram [W, W], count) in float64 of rows x [R, W]."""
    x = np.asarray(x, dtype=np.float64)
    return x.sum(axis=0), x.T @ x, x.shape[0]


def bound(x):
    """(sum bound [W], gram bound [W, W]) of an fp32 sum of R exact products in any order: R 2^-24 sum |terms|."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return a.shape[0] * 2.0 ** -24 * a.sum(axis=0), a.shape[0] * 2.0 ** -24 * (a.T @ a)
