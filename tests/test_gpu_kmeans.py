"""GPU suite of the patch clustering (include/vithip.h, "Patch clustering"): assignment and one update exact on small integers (ties
and an empty cluster included), the stride init, iterated runs on planted clusters against float64, and a context's clustering pinned
bit for bit to the tap on the rows vh_match_operands returns."""
import numpy as np
import pytest

import kmeans_ref as KR
import match_ref as MR
import vithip
from test_gpu_dense import FOLD25
from test_gpu_match import context, dev

pytestmark = pytest.mark.gpu

BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
TYPES = pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
METRICS = pytest.mark.parametrize("metric", [vithip.KMEANS_COSINE, vithip.KMEANS_L2], ids=["cosine", "l2"])
CANARY = 8


def run_tap(x, k, iters, metric, dtype, init=None):
    """vh_op_kmeans of operand values x [n, np, w] (exact in `dtype`) -> (labels [n, np], centroids [n, k, w] float64, counts [n, k]); the
    outputs start as garbage, with canary words behind them."""
    n, rows, w = x.shape
    bufs = [dev(vithip.to16(x.astype(np.float32), dtype)), dev(np.full(n * rows + CANARY, -7, np.int32)),
            dev(np.full(n * k * w + CANARY, 0x7FC1, np.uint16)), dev(np.full(n * k + CANARY, -7, np.int32))]
    ini = None if init is None else dev(vithip.to16(init.astype(np.float32), dtype))
    vithip.op_kmeans(bufs[0].ptr, dtype, n, rows, w, k, iters, metric, None if ini is None else ini.ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
    lab, cent, cnt = (bufs[1].to_numpy(np.int32, (n * rows + CANARY,)), bufs[2].to_numpy(np.uint16, (n * k * w + CANARY,)),
                      bufs[3].to_numpy(np.int32, (n * k + CANARY,)))
    for b in bufs + ([ini] if ini else []):
        b.free()
    assert (lab[n * rows:] == -7).all() and (cent[n * k * w:] == 0x7FC1).all() and (cnt[n * k:] == -7).all(), "a word behind the outputs was written"
    return lab[:n * rows].reshape(n, rows), vithip.from16(cent[:n * k * w], dtype).astype(np.float64).reshape(n, k, w), cnt[:n * k].reshape(n, k)


def integers(seed, n, rows, w, k):
    """x in -3 .. 3 with column 0 = 3, and k centroids in -3 .. 3 of which every one appears twice (every best score is a tie)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (n, rows, w)).astype(np.float64)
    x[..., 0] = 3
    c = rng.integers(-3, 4, ((k + 1) // 2, w)).astype(np.float64)[np.arange(k) % ((k + 1) // 2)]
    c[:, 0] = 3
    return x, c


# ---- 1. assignment, exact ---------------------------------------------------------------------------------------------------------
SHAPES = [(r, w) for r in (2, 37, 64, 65, 197) for w in (64, 192)] + [(65, 2048)]


@pytest.mark.parametrize("rows,w,k", [(r, w, k) for r, w in SHAPES for k in (2, 3, 33, 64) if k <= r])
@TYPES
def test_assignment_is_exact_on_small_integers(dtype, rows, w, k):
    x, c = integers(1000 * rows + w + k, 3, rows, w, k)
    for metric in (vithip.KMEANS_COSINE, vithip.KMEANS_L2):
        lab, cent, cnt = run_tap(x, k, 0, metric, dtype, c)
        for i in range(3):
            ref = KR.kmeans(x[i], k, 0, metric == vithip.KMEANS_L2, dtype, c)
            assert np.array_equal(lab[i], ref[0]) and np.array_equal(cnt[i], ref[2]) and np.array_equal(cent[i], c), (metric, i)


# ---- 2. one update, for bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 33])
@pytest.mark.parametrize("w", [64, 192, 320])   # 320: five 64-column chunks, wave 0 of the update takes a second one
@pytest.mark.parametrize("rows", [37, 65])
@METRICS
@TYPES
def test_one_update_for_bits(dtype, metric, rows, w, k):
    """Every sum and every S_j is an integer below 2^24 (asserted), so no summation order matters: the centroids are numpy's fp32
    quotients, rounded, bit for bit.  Centroid 1 is far off (-100 in column 0, where every row has 3): empty, it comes back unchanged.
    The final labels belong to the updated centroids, which are no integers: the fp32 score of a row carries at most W 2^-23 (sum |x c| + h_j)
    (the match's bound, and the same for the half norm), so the chosen centroid's float64 score is within two bounds of the best, and where the float64 margin exceeds
    two bounds the label is the reference's."""
    l2 = metric == vithip.KMEANS_L2
    x, c = integers(77 * rows + w + k, 3, rows, w, k)
    c[1] = 0
    c[1, 0] = -100
    lab, cent, cnt = run_tap(x, k, 1, metric, dtype, c)
    for i in range(3):
        first = KR.assign(x[i], c, l2)[0]
        sums = np.stack([x[i][first == j].sum(axis=0) for j in range(k)])
        assert np.abs(sums).max() < 2 ** 24 and (sums * sums).sum(axis=1).max() < 2 ** 24 and not (first == 1).any()
        ref = KR.update(x[i], first, c, l2, dtype, fp32=True)
        assert np.array_equal(vithip.to16(cent[i].astype(np.float32), dtype), vithip.to16(ref.astype(np.float32), dtype)), i
        assert np.array_equal(cent[i][1], c[1]) and cnt[i][1] == 0 and np.array_equal(cnt[i], np.bincount(lab[i], minlength=k))
        s = x[i] @ ref.T - (0.5 * (ref * ref).sum(axis=1) if l2 else 0.0)
        bound = 2 * w * 2.0 ** -23 * (np.abs(x[i]) @ np.abs(ref).T + (0.5 * (ref * ref).sum(axis=1) if l2 else 0.0)).max(axis=1)
        top = np.sort(s, axis=1)
        clear = top[:, -1] - top[:, -2] > bound
        assert clear.any() and np.array_equal(lab[i][clear], s.argmax(axis=1)[clear])
        assert (s[np.arange(rows), lab[i]] >= top[:, -1] - bound).all()


# ---- 3. stride init ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,k", [(2, 2), (37, 3), (65, 33), (197, 64)])
@TYPES
def test_stride_init(dtype, rows, k):
    x, _ = integers(rows + k, 2, rows, 64, k)
    lab, cent, cnt = run_tap(x, k, 0, vithip.KMEANS_L2, dtype)
    assert np.array_equal(cent, x[:, KR.stride_rows(rows, k)])
    assert all(np.array_equal(lab[i], KR.kmeans(x[i], k, 0, True, dtype)[0]) for i in range(2))


# ---- 4. iterated, planted clusters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("rows", [65, 197])
@METRICS
@TYPES
def test_planted_clusters(dtype, metric, rows, k):
    """k random directions plus noise, as unit operand rows, the rows of a cluster neighbours (the stride init lands in every cluster).
    The float64 reference's smallest score margin over all rows and iterations is asserted >= 0.05, more than six times the 2^-7 that
    bounds a dot of two unit rows both carrying a bf16 rounding, so the labels must be the reference's for every row.  An update depends
    on the labels and the rows alone, so nothing accumulates: the device's centroid is RNE16 of an fp32 quotient of fp32 sums, the
    reference's RNE16 of the float64 one; the two 16-bit roundings differ by at most half an ulp16 at the element each way round a tie,
    bounded here by half an ulp16 plus the unit roundoff (2^-8 bf16, 2^-11 fp16) of the value, which also covers the fp32 errors
    (197 * 2^-24 relative).  Measured worst |d| / bound: profiles/kmeans_gpu_tests.txt."""
    rng = np.random.default_rng(5)
    dirs = rng.standard_normal((k, 192))
    planted = (np.arange(rows) * k) // rows
    x = MR.operands(np.stack([dirs[planted] + 0.5 * rng.standard_normal((rows, 192)) for _ in range(2)]), dtype, True)
    lab, cent, cnt = run_tap(x, k, 5, metric, dtype)
    mant, emin, u = (7, -126, 2.0 ** -8) if dtype == BF16 else (10, -14, 2.0 ** -11)
    worst = 0.0
    for i in range(2):
        rl, rc, rn, margin = KR.kmeans(x[i], k, 5, metric == vithip.KMEANS_L2, dtype)
        assert margin >= 0.05, margin
        assert np.array_equal(lab[i], rl) and np.array_equal(cnt[i], rn)
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(rc), 2.0 ** emin))) - mant)
        worst = max(worst, (np.abs(cent[i] - rc) / (0.5 * ulp + u * np.abs(rc))).max())
    print(f"kmeans planted {'bf16' if dtype == BF16 else 'fp16'} metric={metric} np={rows} k={k}: worst |d| / bound = {worst:.3e}")
    assert worst <= 1.0


# ---- 5. through a context ---------------------------------------------------------------------------------------------------------
@TYPES
def test_context_equals_the_tap(dtype):
    ctx, images, _ = context("micro", dtype, forward=False)
    ctx.set_feature_layers([1])
    ctx.forward(images)
    order = [0, 1, 2, 1, 0]   # images listed twice, at other positions
    for layer in (-1, 1):
        for metric, m in (("cosine", vithip.KMEANS_COSINE), ("l2", vithip.KMEANS_L2)):
            rows = np.stack([vithip.from16(ctx.match_operands(i, True, layer, "cosine" if metric == "cosine" else "dot"), dtype) for i in range(3)])
            lab, cent, cnt = ctx.cluster_patches(order, 3, iters=3, metric=metric, layer=layer, return_centroids=True)
            tap = run_tap(rows.astype(np.float64), 3, 3, m, dtype)
            for pos, i in enumerate(order):
                assert np.array_equal(lab[pos].reshape(-1), tap[0][i]) and np.array_equal(cnt[pos], tap[2][i]), (layer, metric, pos)
                assert np.array_equal(cent[pos].astype(np.float64), tap[1][i]), (layer, metric, pos)
            again = ctx.cluster_patches([2], 3, iters=0, metric=metric, layer=layer, init=cent[2], return_centroids=True)
            assert np.array_equal(again[0][0], lab[2]) and np.array_equal(again[1][0], cent[2]) and np.array_equal(again[2][0], cnt[2])
    assert lab.shape == (5, 4, 4) and vithip.segment_masks(lab, 3).sum() == 5 * 16
    ctx.close()


def test_refusals():
    """Every refusal of the descriptor calls by its own message (the pointers are never dereferenced), and the contexts the match refuses."""
    D, A = vithip.KmeansDesc, (0x1000, None, 0x3000, 0x4000, 0x5000)   # images, init, labels, centroids, counts
    ctx, images, _ = context("micro", BF16, forward=False, extra=vithip.FLAG_LN_FOLD_OFF)   # (no calibration forward at the load)
    with pytest.raises(vithip.VhError, match="cluster_patches: no forward has run"):
        ctx.cluster_patches([0], 3)
    ctx.forward(images)
    dev_call = lambda d, *p: (lambda: ctx.cluster_patches_device(d, *p))
    for call, text in ((lambda: ctx.cluster_patches([3], 3), "names image 3, outside 0..2"), (lambda: ctx.cluster_patches([0], 1), "k 1 is outside 2..64"),
                       (lambda: ctx.cluster_patches([0], 17), "k 17 exceeds the 16 patches"), (lambda: ctx.cluster_patches([0], 3, iters=65), "iters 65 is outside"),
                       (lambda: ctx.cluster_patches([0], 3, metric=2), "metric 2 is not"), (lambda: ctx.cluster_patches([0] * 13, 3), "nimages 13 is outside 1..12"),
                       (lambda: ctx.cluster_patches([0], 3, layer=3), "layer 3 is not -1 or 1..2"),
                       (lambda: ctx.cluster_patches([0], 3, layer=1), "layer 1 was not in the list"),
                       (dev_call(D(2, -1, 0, 3, 1, 0, 1, 0), *A), "norm 2 is not"), (dev_call(D(0, -1, 0, 3, 1, 2, 1, 0), *A), "init 2 is not"),
                       (dev_call(D(0, -1, 0, 3, 1, 1, 1, 0), *A), "VH_KMEANS_INIT_GIVEN, and only it, takes an init"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 0), 0x1000, 0x2000, 0x3000, None, None), "VH_KMEANS_INIT_GIVEN, and only it, takes an init"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 7), *A), "reserved is not 0"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 0), 0x1000, None, 0x3008, None, None), "not 16-byte aligned"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 0), 0x1000, None, 0x3000, None, 0x5004), "not 16-byte aligned"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 0), None, None, 0x3000, None, None), "null image list"),
                       (dev_call(D(0, -1, 0, 3, 1, 0, 1, 0), 0x1000, None, None, None, None), "null labels"),
                       (lambda: vithip._check(vithip.lib().vh_cluster_patches_device(ctx.h, None, *A), ctx.h), "null descriptor")):
        with pytest.raises(vithip.VhError, match="cluster_patches: .*" + text):
            call()
    assert ctx.cluster_patches([0], 3).shape == (1, 4, 4)   # the refusals left the context usable
    ctx.ring_create(2, 2)
    with pytest.raises(vithip.VhError, match="cluster_patches: a ring exists"):
        ctx.cluster_patches([0], 3)
    ctx.close()
    for kw, text in ((dict(dtype=BF16, flags=vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL), "a VH_FLAG_CLS_TAIL context"),
                     (dict(dtype=vithip.DTYPE_FP8), "a VH_DTYPE_FP8 context")):
        other = vithip.VitContext(FOLD25, max_batch=2, ln_eps=1e-6, **kw)
        with pytest.raises(vithip.VhError, match="cluster_patches: " + text):
            other.cluster_patches([0], 3)
        other.close()
