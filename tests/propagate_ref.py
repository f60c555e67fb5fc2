"""Label propagation in numpy (include/vithip.h, "Label propagation"), float64: the scores of the operand rows as the device holds them,
the square window, the first k under (score descending, id ascending), the weights and the vote."""
import numpy as np


def window(gh, gw, radius):
    """[NP, NP] bool: key patch j is a candidate of query patch q (radius 0: every patch is)."""
    y, x = np.divmod(np.arange(gh * gw), gw)
    if radius == 0:
        return np.ones((gh * gw, gh * gw), dtype=bool)
    return (np.abs(y[:, None] - y[None]) <= radius) & (np.abs(x[:, None] - x[None]) <= radius)


def scores(rows, item, gh, gw, radius):
    """[NP, S * NP] float64 scores of item (t, s_0 ..) on rows [images, NP, W]; -inf where key id g = slot * NP + j is no candidate."""
    n = gh * gw
    s = np.full((n, (len(item) - 1) * n), -np.inf)
    for slot, img in enumerate(item[1:]):
        if img >= 0:
            s[:, slot * n:(slot + 1) * n] = np.where(window(gh, gw, radius), rows[item[0]] @ rows[img].T, -np.inf)
    return s


def select(s, k):
    """(idx [NP, k] int32, score [NP, k]): the first k ids under (score descending, id ascending) -- a stable sort --, tails -1 / -inf."""
    s = np.concatenate([s, np.full((s.shape[0], k), -np.inf)], axis=1)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    score = np.take_along_axis(s, order, axis=1)
    return np.where(np.isfinite(score), order, -1).astype(np.int32), score


def vote(idx, score, item, labels, tau):
    """out [NP, C] float64 of a kept set: weights exp((s_e - s_0) / tau), labels [images, NP, C] indexed by the slot's image; a row
    without a kept id is zero."""
    n, ok, g = labels.shape[1], idx >= 0, np.maximum(idx, 0)
    sc = np.where(ok, score, 0.0).astype(np.float64)
    w = np.where(ok, np.exp((sc - sc[:, :1]) / tau), 0.0)
    rows = labels[np.asarray(item[1:])[g // n], g % n].astype(np.float64)
    z = w.sum(axis=1, keepdims=True)
    return (w[..., None] * rows).sum(axis=1) / np.where(z > 0, z, 1.0)
