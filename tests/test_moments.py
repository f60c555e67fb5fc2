"""The host side of the feature moments (include/vithip.h, "Feature moments"), no device: the float64 accumulator, its PCA and the
dense head made of it, the descriptor and the bindings."""
import ctypes as C

import numpy as np

import moments_ref as R
import vithip


def planted(rows=400, w=24):
    """Rank-3 data (scales 5, 3, 2) plus small noise around a mean."""
    rng = np.random.default_rng(7)
    basis = np.linalg.qr(rng.standard_normal((w, 3)))[0].T
    return rng.standard_normal((rows, 3)) * [5.0, 3.0, 2.0] @ basis + 0.01 * rng.standard_normal((rows, w)) + rng.standard_normal(w)


def test_feature_moments_pca_and_head():
    x = planted()
    fm = vithip.FeatureMoments(x.shape[1])
    fm.add(*R.moments(x[:150])).add(*R.moments(x[150:]))
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert fm.count == len(x) and rel(fm.mean(), x.mean(axis=0)) <= 1e-12 and rel(fm.covariance(), np.cov(x.T)) <= 1e-12
    val, comp = fm.pca(3)
    _, sv, vt = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)
    assert comp.shape == (3, x.shape[1]) and (np.diff(val) < 0).all() and rel(val, sv[:3] ** 2 / (len(x) - 1)) <= 1e-9
    assert all(abs(comp[i] @ vt[i]) >= 1 - 1e-9 for i in range(3))
    assert all(comp[i][np.argmax(np.abs(comp[i]))] > 0 for i in range(3))   # the sign rule
    weight, bias = vithip.pca_head(fm.mean(), comp)
    assert rel(x @ weight.T + bias, (x - fm.mean()) @ comp.T) <= 1e-12
    mean, white = fm.whitening(3, 0.0)
    assert rel(np.cov(((x - mean) @ white.T).T), np.eye(3)) <= 1e-9


def test_descriptor_and_symbols():
    assert C.sizeof(vithip.MomentsDesc) == 16
    assert {"vh_patch_moments", "vh_patch_moments_device", "vh_patch_moments_device_async", "vh_op_moments", "vh_op_moments_workspace_bytes",
            "vh_op_moments_slabs"} <= set(vithip.SYMBOLS)
