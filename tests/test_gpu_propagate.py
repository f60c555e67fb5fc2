"""GPU suite of the label propagation (include/vithip.h, "Label propagation"): the selection exact on integers (every rank a tie), the
window by planted maxima, the vote exact where the weights are 1 and bounded on real values, and a context's call pinned bit for bit to
the tap on the match's operand rows."""
import numpy as np
import pytest

import features_ref as R
import match_ref as MR
import propagate_ref as PR
import vithip
from test_gpu_match import BF16, COS, DOT, FP16, TYPES, context, dev

pytestmark = pytest.mark.gpu

CANARY = 8
ITEMS = {1: [[0, 1], [2, 2]], 2: [[0, 0, 1], [2, 1, 0]], 3: [[0, 1, -1, 2], [1, -1, 0, 0]]}   # by S; the S = 3 items have an absent slot
# out against the float64 vote on the kernel's own kept set: |d| <= K_VOTE 2^-23 max|L|.  K_VOTE = four times the worst ratio measured on
# an MI355X, 0.717 (profiles/propagate_gpu_tests.txt); it must stay below k + 8 + max|(s_e - s_0) c|: one rounding per term of the chain
# and of Z, the quotient, and the rounding of the exponential's argument.
K_VOTE = 2.9


def run_tap(rows, items, labels, gh, gw, k, dtype, tau=0.1, radius=0):
    """vh_op_propagate of operand values rows [images, NP, W] (exact in `dtype`) -> (out, idx, score) per item; the outputs start as
    garbage, with canary words behind them."""
    items, labels = np.asarray(items, np.int32), np.asarray(labels, np.float32)
    (images, n, w), (ni, c) = rows.shape, (items.shape[0], labels.shape[2])
    no, ns = ni * n * c, ni * n * k
    bufs = [dev(vithip.to16(rows.astype(np.float32), dtype)), dev(items), dev(labels), dev(np.full(no + CANARY, np.nan, np.float32)),
            dev(np.full(ns + CANARY, -7, np.int32)), dev(np.full(ns + CANARY, np.nan, np.float32))]
    vithip.op_propagate(bufs[0].ptr, dtype, images, gh, gw, w, bufs[1].ptr, ni, items.shape[1] - 1, k, radius, tau, bufs[2].ptr, c,
                        bufs[3].ptr, bufs[4].ptr, bufs[5].ptr)
    out, idx, score = (bufs[3].to_numpy(np.float32, (no + CANARY,)), bufs[4].to_numpy(np.int32, (ns + CANARY,)),
                       bufs[5].to_numpy(np.float32, (ns + CANARY,)))
    for b in bufs:
        b.free()
    assert np.isnan(out[no:]).all() and (idx[ns:] == -7).all() and np.isnan(score[ns:]).all(), "a word behind the outputs was written"
    return out[:no].reshape(ni, n, c), idx[:ns].reshape(ni, n, k), score[:ns].reshape(ni, n, k)


def assert_selection(got, rows, items, gh, gw, k, radius, what):
    for i, item in enumerate(items):
        idx, score = PR.select(PR.scores(rows, item, gh, gw, radius), k)
        assert np.array_equal(got[1][i], idx) and np.array_equal(got[2][i].astype(np.float64), score), (what, i)


def integer_case(seed, images, n, w, duplicate):
    rng = np.random.default_rng(seed)
    half = (n + 1) // 2 if duplicate else n
    return rng.integers(-4, 5, (images, half, w)).astype(np.float64)[:, np.arange(n) % half], rng.integers(-8, 9, (images, n, 3))


# ---- 1. the selection, exact on integers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,k", [(1, 1), (3, 5), (2, 16)])
@pytest.mark.parametrize("w", [64, 192])
@pytest.mark.parametrize("gh,gw", [(1, 1), (5, 5), (8, 8), (5, 13), (10, 13), (14, 14)])
@TYPES
def test_selection_is_exact_on_small_integers(dtype, gh, gw, w, s, k):
    """Operands in -4 .. 4 (exact in both types); every key row appears twice in its image, so every rank is a tie."""
    rows, labels = integer_case(100 * gh * gw + w + s, 3, gh * gw, w, True)
    assert_selection(run_tap(rows, ITEMS[s], labels, gh, gw, k, dtype, tau=64.0), rows, ITEMS[s], gh, gw, k, 0, (gh, gw, w, s, k))


# ---- 2. the window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("gh,gw", [(5, 13), (14, 14)])
@TYPES
def test_window(dtype, gh, gw, radius):
    """S = 1, k = 5: a corner query has 4 candidates at radius 1 (tails -1 / -inf).  S = 2: the all-4 row of the centre query meets an
    all-4 key -- the unique global maximum 16 W -- one column outside its window: it must not appear; the same maximum in the last,
    partly filled key tile of the second slot, inside the last query's window, must come first with id NP + j."""
    n, w = gh * gw, 64
    rows, labels = integer_case(7 * n + radius, 3, n, w, False)
    got = run_tap(rows, ITEMS[1], labels, gh, gw, 5, dtype, tau=64.0, radius=radius)
    assert_selection(got, rows, ITEMS[1], gh, gw, 5, radius, "corner")
    if radius == 1:
        assert (got[1][0, 0, :4] >= 0).all() and (got[1][0, 0, 4:] == -1).all() and np.isneginf(got[2][0, 0, 4:]).all()
    centre, outside = (gh // 2) * gw + gw // 2, (gh // 2) * gw + gw // 2 + radius + 1
    rows[0, [centre, n - 1]] = rows[1, outside] = rows[2, n - 1] = 4
    got = run_tap(rows, [[0, 1, 2]], labels, gh, gw, 5, dtype, tau=64.0, radius=radius)
    assert_selection(got, rows, [[0, 1, 2]], gh, gw, 5, radius, "planted")
    assert outside not in got[1][0, centre] and got[2][0, centre].max() < 16 * w
    assert got[1][0, n - 1, 0] == n + n - 1 and got[2][0, n - 1, 0] == 16 * w


# ---- 3. the vote, exact where the weights are 1 ---------------------------------------------------------------------------------------
@TYPES
def test_vote_is_exact_with_unit_weights(dtype):
    """k = 1: out is the chosen label row bit for bit.  Every candidate the same row, k = 4: the first four ids with weights 1, out =
    sum L / 4 exactly (integer labels)."""
    gh, gw, w, items = 5, 13, 64, ITEMS[3]
    rows, labels = integer_case(3, 3, gh * gw, w, True)
    out, idx, _ = run_tap(rows, items, labels, gh, gw, 1, dtype)
    for i, item in enumerate(items):
        chosen = labels[np.asarray(item[1:])[idx[i, :, 0] // (gh * gw)], idx[i, :, 0] % (gh * gw)]
        assert np.array_equal(out[i], chosen.astype(np.float32)), i
    rows[:] = rows[0, 0]
    out, idx, _ = run_tap(rows, items, labels, gh, gw, 4, dtype)
    assert (idx[0] == np.arange(4)).all() and (idx[1] == gh * gw + np.arange(4)).all()   # slot 0 of item 0; slot 1 of item 1 (slot 0 absent)
    assert np.array_equal(out[0], np.broadcast_to(labels[1, :4].sum(axis=0) / 4.0, out[0].shape).astype(np.float32))
    assert np.array_equal(out[1], np.broadcast_to(labels[0, :4].sum(axis=0) / 4.0, out[1].shape).astype(np.float32))


# ---- 4. the vote on real values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [3, 150])
@pytest.mark.parametrize("tau", [0.1, 1.0])
@TYPES
def test_vote_on_real_values(dtype, tau, classes):
    """Gaussian unit rows: |score - ref| <= W 2^-23 sum |a b| (ref = float64 on the same operands), every kept key within two bounds of
    the reference's k-th score, and out within K_VOTE 2^-23 max|L| of the float64 vote on the kernel's own kept set and scores."""
    gh, gw, w, k, items = 10, 13, 192, 5, ITEMS[3]
    rng = np.random.default_rng(4)
    rows = MR.operands(rng.standard_normal((3, gh * gw, w)), dtype, True)
    labels = rng.standard_normal((3, gh * gw, classes)).astype(np.float32)
    out, idx, score = run_tap(rows, items, labels, gh, gw, k, dtype, tau=tau)
    worst = cap = 0.0
    for i, item in enumerate(items):
        ref = PR.scores(rows, item, gh, gw, 0)
        bound = w * 2.0 ** -23 * np.where(np.isfinite(ref), PR.scores(np.abs(rows), item, gh, gw, 0), 0.0)
        pick = lambda m: np.take_along_axis(m, idx[i].astype(np.int64), axis=1)
        assert idx[i].min() >= 0 and (np.abs(score[i] - pick(ref)) <= pick(bound)).all()
        assert (pick(ref) >= PR.select(ref, k)[1][:, -1:] - 2 * pick(bound)).all()
        d = np.abs(out[i] - PR.vote(idx[i], score[i], item, labels, tau))
        worst = max(worst, d.max() / (2.0 ** -23 * np.abs(labels).max()))
        cap = max(cap, k + 8 + np.abs((score[i] - score[i][:, :1]) * np.float32(np.log2(np.e) / tau)).max())
    print(f"propagate vote {'bf16' if dtype == BF16 else 'fp16'} tau={tau} C={classes}: worst |d| / (2^-23 max|L|) = {worst:.3f}, "
          f"K_VOTE = {K_VOTE}, cap k + 8 + max|ds c| = {cap:.2f}")
    assert K_VOTE <= cap and worst <= K_VOTE


# ---- 5. through a context -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["micro", "fold25"])
@TYPES
def test_context_equals_the_tap(dtype, model):
    ctx, _, _ = context(model, dtype)
    _, _, n, _ = ctx.features_dims()
    g, items = int(round(n ** 0.5)), ITEMS[3]
    labels = np.random.default_rng(2).standard_normal((3, n, 4)).astype(np.float32)
    same = lambda a, b: all(np.array_equal(R.bits(x), R.bits(y)) for x, y in zip(a, b))
    for metric in (COS, DOT):
        for radius in (0, 1):
            got = ctx.propagate_labels(items, labels, k=3, tau=0.5, radius=radius, metric=metric, topk=True)
            rows = np.stack([vithip.from16(ctx.match_operands(i, metric=metric), dtype) for i in range(3)]).astype(np.float64)
            tap = run_tap(rows, items, labels, g, g, 3, dtype, tau=0.5, radius=radius)
            assert same(got, tap), (metric, radius)
    # the device form, asynchronous: the same bits; an index outside the batch (3) marks its item and reads nothing
    d_it, d_lab = dev(np.array([[1, -1, 0, 0], [0, 3, -1, 2]], np.int32)), dev(labels)
    d_out, d_idx, d_sc = dev(np.full((2, n, 4), np.nan, np.float32)), dev(np.zeros((2, n, 3), np.int32)), dev(np.zeros((2, n, 3), np.float32))
    ctx.propagate_labels_device(vithip.PropagateDesc(vithip.FEAT_NORM, -1, DOT, 2, 3, 3, 1, 4, 0.5, 0), d_it.ptr, d_lab.ptr, d_out.ptr, d_idx.ptr,
                                d_sc.ptr, sync=False)
    ctx.synchronize()
    out, idx, sc = d_out.to_numpy(np.float32, (2, n, 4)), d_idx.to_numpy(np.int32, (2, n, 3)), d_sc.to_numpy(np.float32, (2, n, 3))
    assert same((out[0], idx[0], sc[0]), (got[0][1], got[1][1], got[2][1]))
    assert (idx[1] == -1).all() and np.isneginf(sc[1]).all() and not out[1].any()
    for b in (d_it, d_lab, d_out, d_idx, d_sc):
        b.free()
    # the video chain: frame t from {0} and the frames before it, each step the host form's bits on the labels so far, and every step
    # within the vote's bound of the float64 vote on its kept set
    video = vithip.propagate_video(ctx, labels[0], n_ctx=2, k=3, tau=0.5)
    chain = np.zeros_like(labels)
    chain[0] = labels[0]
    for t, item in ((1, [1, 0, -1, -1]), (2, [2, 0, 1, -1])):
        chain[t], idx, sc = (a[0] for a in ctx.propagate_labels([item], chain, k=3, tau=0.5, topk=True))
        assert np.abs(chain[t] - PR.vote(idx, sc, item, chain, 0.5)).max() <= K_VOTE * 2.0 ** -23 * np.abs(chain).max()
    assert np.array_equal(R.bits(video), R.bits(chain))
    ctx.close()


def test_refusals():
    ctx, images, _ = context("micro", BF16, forward=False, extra=vithip.FLAG_LN_FOLD_OFF)   # (no calibration forward at the load)
    labels = np.zeros((2, 16, 3), np.float32)
    with pytest.raises(vithip.VhError, match="propagate_labels: no forward has run"):
        ctx.propagate_labels_device(vithip.PropagateDesc(0, -1, 0, 1, 1, 1, 0, 3, 0.1, 0), 0x1000, 0x2000, 0x3000)
    ctx.forward(images[:2])
    call = lambda items=[[0, 1]], **kw: (lambda: ctx.propagate_labels(items, labels, **kw))
    desc = lambda *a: (lambda: ctx.propagate_labels_device(vithip.PropagateDesc(*a), 0x1000, 0x2000, 0x3000))
    for f, text in ((call([[0, 2]]), "item 0 names image 2, outside 0..1"), (call([[-1, 0]]), "item 0 names image -1"),
                    (call(layer=1), "layer 1 was not in the list"), (call(layer=3), "layer 3 is not -1 or 1..2"),
                    (call(metric=2), "metric 2 is not"), (call(norm=2), "norm 2 is not"), (call([[0, 1]] * 13), "nitems 13 is outside 1..12"),
                    (call([[0] * 10]), "nsrc 9 is outside 1..8"), (call(k=0), "k 0 is outside 1..16"), (call(k=17), "k 17 is outside"),
                    (call(radius=-1), "radius -1 is outside"), (call(radius=4097), "radius 4097 is outside"), (call(tau=0.0), "tau 0 is not finite"),
                    (call(tau=float("nan")), "tau nan is not finite"), (desc(0, -1, 0, 1, 1, 1, 0, 0, 0.1, 0), "classes 0 is outside"),
                    (desc(0, -1, 0, 1, 1, 1, 0, 257, 0.1, 0), "classes 257 is outside"), (desc(0, -1, 0, 1, 1, 1, 0, 3, 0.1, 1), "reserved is not 0"),
                    (lambda: ctx.propagate_labels_device(vithip.PropagateDesc(0, -1, 0, 1, 1, 1, 0, 3, 0.1, 0), 0x1000, 0x2008, 0x3000),
                     "not 16-byte aligned"),
                    (lambda: ctx.propagate_labels_device(vithip.PropagateDesc(0, -1, 0, 1, 1, 1, 0, 3, 0.1, 0), 0x1000, None, 0x3000),
                     "null labels or out")):
        with pytest.raises(vithip.VhError, match="propagate_labels: .*" + text):
            f()
    ctx.close()
