"""GPU suite of the feature moments (include/vithip.h, "Feature moments"): column sums, X^T X and the count exact on small integers over
tails, slab boundaries and half tiles, the accumulate forms, the fp32 bound on real values, and a context's moments pinned bit for bit to
the tap on the rows vh_match_operands returns."""
import numpy as np
import pytest

import match_ref as MR
import moments_ref as R
import vithip
from test_gpu_dense import FOLD25
from test_gpu_match import context, dev

pytestmark = pytest.mark.gpu

BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
TYPES = pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
CANARY = 8
MULTI = 257   # the smallest row count with two slabs at width 64: min(512, ceil(257 / 256)) = 2 slabs of 160 rows


class Outputs:
    """sum, gram and count on the device, prefilled with NaNs / a garbage count, canary words behind them."""

    def __init__(self, w):
        self.w = w
        self.bufs = [dev(np.full(w + CANARY, np.nan, np.float32)), dev(np.full(w * w + CANARY, np.nan, np.float32)), dev(np.full(1 + CANARY, -7, np.int64))]
        self.ptrs = [b.ptr for b in self.bufs]

    def read(self):
        w = self.w
        s, g, n = (b.to_numpy(t, (k + CANARY,)) for b, t, k in zip(self.bufs, (np.float32, np.float32, np.int64), (w, w * w, 1)))
        for b in self.bufs:
            b.free()
        assert np.isnan(s[w:]).all() and np.isnan(g[w * w:]).all() and (n[1:] == -7).all(), "a word behind the outputs was written"
        return s[:w], g[:w * w].reshape(w, w), int(n[0])


def run_tap(sets, dtype):
    """vh_op_moments of every row set of `sets` (values exact in `dtype`) into the same outputs, the first call overwriting garbage."""
    w = sets[0].shape[1]
    out = Outputs(w)
    for k, x in enumerate(sets):
        ws, x16 = dev(np.zeros(vithip.op_moments_workspace_bytes(len(x), w), np.uint8)), dev(vithip.to16(x.astype(np.float32), dtype))
        vithip.op_moments(x16.ptr, dtype, len(x), w, int(k > 0), *out.ptrs, ws.ptr)
        ws.free()
        x16.free()
    return out.read()


def assert_exact(got, sets):
    refs = [R.moments(x) for x in sets]
    assert max((np.abs(x).T @ np.abs(x)).max() for x in sets) * len(sets) < 2 ** 24   # every partial sum is an integer below 2^24
    assert np.array_equal(got[1], got[1].T), "gram is not bitwise symmetric"
    assert np.array_equal(got[0].astype(np.float64), sum(r[0] for r in refs)) and got[2] == sum(r[2] for r in refs)
    assert np.array_equal(got[1].astype(np.float64), sum(r[1] for r in refs))


def test_the_multi_slab_shape_has_two_slabs():
    assert vithip.op_moments_slabs(MULTI, 64) >= 2 and vithip.op_moments_slabs(MULTI - 1, 64) == 1


@pytest.mark.parametrize("rows,w", [(r, w) for r in (1, 15, 37, 65, 197) for w in (64, 192, 320)] + [(65, 2048), (MULTI, 64), (MULTI, 192)])
@TYPES
def test_exact_on_small_integers(dtype, rows, w):
    x = np.random.default_rng(100 * rows + w).integers(-3, 4, (rows, w)).astype(np.float64)
    assert_exact(run_tap([x], dtype), [x])


@pytest.mark.parametrize("w", [64, 320])
@TYPES
def test_accumulate(dtype, w):
    rng = np.random.default_rng(w)
    sets = [rng.integers(-3, 4, (r, w)).astype(np.float64) for r in (65, MULTI, 15)]
    assert_exact(run_tap(sets, dtype), sets)


@pytest.mark.parametrize("rows", [197, MULTI])
@TYPES
def test_real_values(dtype, rows):
    """Unit rows: |gram - ref| <= R 2^-24 |x|^T |x| elementwise, the bound of an fp32 sum of R exact products in any order; sum alike."""
    x = MR.operands(np.random.default_rng(rows).standard_normal((rows, 192)), dtype, True)
    s, g, n = run_tap([x], dtype)
    (rs, rg, rn), (bs, bg) = R.moments(x), R.bound(x)
    print(f"moments real values {'bf16' if dtype == BF16 else 'fp16'} rows={rows}: worst |d| / bound: gram {(np.abs(g - rg) / bg).max():.3e}, "
          f"sum {(np.abs(s - rs) / bs).max():.3e}")
    assert n == rn and np.array_equal(g, g.T) and (np.abs(g - rg) <= bg).all() and (np.abs(s - rs) <= bs).all()


@TYPES
def test_context_equals_the_tap(dtype):
    ctx, images, _ = context("micro", dtype, forward=False)
    ctx.set_feature_layers([1])
    ctx.forward(images)
    order = [0, 1, 2, 1, 0]
    for layer in (-1, 1):
        for norm in (True, False):
            rows = [vithip.from16(ctx.match_operands(i, norm, layer, "dot"), dtype).astype(np.float64) for i in range(3)]
            tap = run_tap([np.concatenate([rows[i] for i in order])], dtype)
            host = ctx.patch_moments(order, norm, layer)
            assert all(np.array_equal(a, b) for a, b in zip(host, tap)), (layer, norm)
            # the device form, one index outside the batch: the list without it
            out, lst = Outputs(128), dev(np.array([0, 1, 7, 2, 1, 0], np.int32))
            ctx.patch_moments_device(vithip.MomentsDesc(vithip.FEAT_NORM if norm else vithip.FEAT_RAW, layer, 0, 6), lst.ptr, *out.ptrs)
            lst.free()
            got = out.read()
            assert got[2] == 5 * 16 and all(np.array_equal(a, b) for a, b in zip(got, tap)), (layer, norm)
    ctx.close()


def test_refusals():
    """Every refusal of the descriptor calls by its own message (the pointers are never dereferenced), and the contexts the match refuses."""
    D, A = vithip.MomentsDesc, (0x1000, 0x2000, 0x3000, 0x4000)   # images, sum, gram, count
    ctx, images, _ = context("micro", BF16, forward=False, extra=vithip.FLAG_LN_FOLD_OFF)
    with pytest.raises(vithip.VhError, match="patch_moments: no forward has run"):
        ctx.patch_moments([0])
    ctx.forward(images)
    dev_call = lambda d, *p: (lambda: ctx.patch_moments_device(d, *p))
    host_acc = lambda: vithip._check(vithip.lib().vh_patch_moments(ctx.h, vithip.C.byref(D(0, -1, 1, 1)), *A), ctx.h)
    for call, text in ((lambda: ctx.patch_moments([3]), "names image 3, outside 0..2"), (lambda: ctx.patch_moments([0] * 13), "nimages 13 is outside 1..12"),
                       (lambda: ctx.patch_moments([0], layer=3), "layer 3 is not -1 or 1..2"), (lambda: ctx.patch_moments([0], layer=1), "layer 1 was not in the list"),
                       (dev_call(D(2, -1, 0, 1), *A), "norm 2 is not"), (dev_call(D(0, -1, 2, 1), *A), "accumulate 2 is not 0 or 1"),
                       (host_acc, "accumulate is for the device forms"), (dev_call(D(0, -1, 0, 0), *A), "nimages 0 is outside"),
                       (dev_call(D(0, -1, 0, 1), 0x1000, 0x2008, 0x3000, 0x4000), "not 16-byte aligned"),
                       (dev_call(D(0, -1, 0, 1), 0x1000, 0x2000, 0x3000, 0x4008), "not 16-byte aligned"),
                       (dev_call(D(0, -1, 0, 1), None, 0x2000, 0x3000, 0x4000), "null image list"),
                       (dev_call(D(0, -1, 0, 1), 0x1000, 0x2000, None, 0x4000), "null output"),
                       (lambda: vithip._check(vithip.lib().vh_patch_moments_device(ctx.h, None, *A), ctx.h), "null descriptor")):
        with pytest.raises(vithip.VhError, match="patch_moments: .*" + text):
            call()
    assert ctx.patch_moments([0])[2] == 16   # the refusals left the context usable
    ctx.ring_create(2, 2)
    with pytest.raises(vithip.VhError, match="patch_moments: a ring exists"):
        ctx.patch_moments([0])
    ctx.close()
    for kw, text in ((dict(dtype=BF16, flags=vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL), "a VH_FLAG_CLS_TAIL context"),
                     (dict(dtype=vithip.DTYPE_FP8), "a VH_DTYPE_FP8 context")):
        other = vithip.VitContext(FOLD25, max_batch=2, ln_eps=1e-6, **kw)
        with pytest.raises(vithip.VhError, match="patch_moments: " + text):
            other.patch_moments([0])
        other.close()
