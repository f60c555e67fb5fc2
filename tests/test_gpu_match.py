"""GPU suite of the dense correspondence (include/vithip.h, "Dense correspondence"): exact on small integers (ties included), bounded on
real values and in the prepare pass, and a context's match pinned bit for bit to the tap on the rows the token features return."""
import numpy as np
import pytest

import features_ref as R
import match_ref as MR
import vh_synth as S
import vit_ref
import vithip
from test_gpu_dense import FOLD25

pytestmark = pytest.mark.gpu

BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
TYPES = pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
COS, DOT = vithip.MATCH_COSINE, vithip.MATCH_DOT
EPS, CANARY = 1e-6, 8
MICRO = S.CONFIGS["vit_micro"]   # dim 128, 16 patches, fp32 residual; FOLD25: dim 256, 25 patches, split planes
REG4, NOCLS = vithip.FLAG_REGISTERS(4), vithip.FLAG_NO_CLS | vithip.FLAG_POOL(vithip.POOL_AVG_NORM)
MODELS = {"micro": (MICRO, 0), "fold25": (FOLD25, 0), "micro_reg4": (MICRO, REG4), "fold25_nocls": (FOLD25, NOCLS)}


def dev(a):
    return vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def run_tap(a16, b16, dtype, metric=DOT):
    """vh_op_match of operand values (exact in `dtype`) -> (idx, score); the outputs start as garbage, with canary words behind them."""
    (npairs, na, w), nb = a16.shape, b16.shape[1]
    n = npairs * na
    bufs = [dev(vithip.to16(a16.astype(np.float32), dtype)), dev(vithip.to16(b16.astype(np.float32), dtype)),
            dev(np.full(n + CANARY, -7, np.int32)), dev(np.full(n + CANARY, np.nan, np.float32))]
    vithip.op_match(bufs[0].ptr, bufs[1].ptr, dtype, npairs, na, nb, w, metric, bufs[2].ptr, bufs[3].ptr)
    idx, score = bufs[2].to_numpy(np.int32, (n + CANARY,)), bufs[3].to_numpy(np.float32, (n + CANARY,))
    for b in bufs:
        b.free()
    assert (idx[n:] == -7).all() and np.isnan(score[n:]).all(), "a word behind the outputs was written"
    return idx[:n].reshape(npairs, na), score[:n].reshape(npairs, na)


def assert_exact(got, s, what):
    idx, score = MR.best(s)
    assert np.array_equal(got[0], idx) and np.array_equal(got[1].astype(np.float64), score), what


# ---- 1. exact on integers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npairs", [1, 3])
@pytest.mark.parametrize("w", [64, 192])
@pytest.mark.parametrize("na,nb", [(1, 1), (17, 5), (64, 64), (65, 33), (130, 197)])
@TYPES
def test_op_match_is_exact_on_small_integers(dtype, na, nb, w, npairs):
    """Operands in -4 .. 4 (exact in both types, |sum| <= 16 * 192); every row of B appears twice, so every maximum is a tie."""
    rng = np.random.default_rng(1000 * na + 10 * nb + w + npairs)
    a = rng.integers(-4, 5, (npairs, na, w)).astype(np.float64)
    b = rng.integers(-4, 5, (npairs, (nb + 1) // 2, w)).astype(np.float64)[:, np.arange(nb) % ((nb + 1) // 2)]
    assert_exact(run_tap(a, b, dtype), MR.scores(a, b), (na, nb, w, npairs))


@TYPES
def test_op_match_with_128_query_rows(dtype):
    """128 pairs of 130 rows: npairs * ceil(na / 128) reaches 256 and the launcher takes its 128-row query block; rows 128, 129 a second."""
    a, b = (np.random.default_rng(9).integers(-4, 5, (128, n, 64)).astype(np.float64) for n in (130, 197))
    assert_exact(run_tap(a, b[:, np.arange(197) % 99], dtype), MR.scores(a, b[:, np.arange(197) % 99]), "QB 128")


@pytest.mark.parametrize("kind", ["negative", "last_key", "two_tiles"])
@TYPES
def test_op_match_placements(dtype, kind):
    """A in 1 .. 4.  negative: B < 0, every score is negative (a zero-padded key would win).  last_key: B <= 0 but its last row, the
    unique maximum, in the partly filled fourth tile.  two_tiles: the same maximum in rows 5 and 130 (tiles 0 and 2): 5 wins."""
    rng = np.random.default_rng(5)
    a = rng.integers(1, 5, (3, 130, 192)).astype(np.float64)
    b = rng.integers(-4, 0 if kind == "negative" else 1, (3, 197, 192)).astype(np.float64)
    if kind != "negative":
        b[:, [196] if kind == "last_key" else [5, 130]] = 4
    got = run_tap(a, b, dtype)
    assert_exact(got, MR.scores(a, b), kind)
    assert (got[1] < 0).all() if kind == "negative" else (got[0] == (196 if kind == "last_key" else 5)).all()


# ---- 2. bounded on real values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, DOT], ids=["cosine", "dot"])
@TYPES
def test_op_match_on_real_values(dtype, metric):
    """|score - ref| <= W 2^-23 sum_k |a_k b_k| (fp32 summation), ref = float64 on the same operands; the chosen key is within 2 bounds."""
    rng = np.random.default_rng(3)
    w = 192
    a16 = MR.operands(rng.standard_normal((2, 130, w)), dtype, metric == COS)
    b16 = MR.operands(rng.standard_normal((2, 197, w)), dtype, metric == COS)
    idx, score = run_tap(a16, b16, dtype, metric)
    ref, bound = MR.scores(a16, b16), w * 2.0 ** -23 * MR.scores(np.abs(a16), np.abs(b16))
    assert idx.min() >= 0 and idx.max() < 197
    pick = lambda m: np.take_along_axis(m, idx[..., None].astype(np.int64), axis=-1)[..., 0]
    d = np.abs(score - pick(ref))
    print(f"match real values {'bf16' if dtype == BF16 else 'fp16'} metric={metric}: worst |d| / bound = {(d / pick(bound)).max():.3e}")
    assert (d <= pick(bound)).all()
    assert (pick(ref) >= ref.max(axis=-1) - 2 * pick(bound)).all()


# ---- 3 .. 6: through a context ----------------------------------------------------------------------------------------------------
def context(model, dtype, max_batch=3, forward=True, extra=0):
    cfg, flags = MODELS[model]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=max_batch, ln_eps=EPS, flags=flags | extra)
    ctx.load_weights(vit_ref.make_blob(cfg, 11, flags, EPS))
    images = S.make_images(cfg, 3, max_batch)
    return ctx, images, (ctx.forward(images) if forward else None)


@pytest.mark.parametrize("model", ["micro", "fold25"])
@TYPES
def test_prepare_pass(dtype, model):
    """The cosine operands against float64 x16 / ||x16||: half an ulp16 + 2^-20 |value| (one rounding behind fp32; test_gpu_swiglu.py)."""
    ctx, _, _ = context(model, dtype)
    feats = ctx.read_features(cls=False, patch=True, norm=vithip.FEAT_NORM)["patch"]
    x16 = MR.round16(feats, dtype)
    ref = x16 / np.sqrt((x16 * x16).sum(axis=-1, keepdims=True))
    got = np.stack([vithip.from16(ctx.match_operands(i), dtype) for i in range(3)]).astype(np.float64)
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin))) - mant)   # the spacing of the 16-bit type at |ref|
    ratio = np.abs(got - ref) / (0.5 * ulp + 2.0 ** -20 * np.abs(ref))
    print(f"match prepare {model} {'bf16' if dtype == BF16 else 'fp16'}: worst |d| / bound = {ratio.max():.3e}")
    assert ratio.max() <= 1.0
    dot = np.stack([ctx.match_operands(i, metric="dot") for i in range(3)])
    assert np.array_equal(dot, vithip.to16(feats, dtype))   # the DOT operand IS the rounded feature row
    ctx.close()


@TYPES
def test_prepare_pass_keeps_a_zero_row(dtype):
    """A model of zeros on images of zeros: every raw patch row is zero, stays zero, and scores 0 against everything."""
    cfg = MICRO
    blob = S.make_blob(cfg, 11, EPS).copy()
    blob[64:] = 0
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_OFF)
    ctx.load_weights(blob)
    ctx.forward(np.zeros_like(S.make_images(cfg, 3, 2)))
    assert not ctx.match_operands(1, norm=False).any()
    idx, score = ctx.match_patches([(0, 1)], norm=False)
    assert not idx.any() and not score.any() and not np.signbit(score).any()
    ctx.close()


def tap_on_features(ctx, pairs, dtype, norm, layer, metric):
    """vh_op_match on the context's rows: DOT on the rounded token features, COSINE on the operands read back."""
    if metric == "dot":
        f = ctx.read_layer_features(layer, cls=False, patch=True, norm=vithip.FEAT_NORM if norm else vithip.FEAT_RAW)["patch"]
        rows = MR.round16(f, dtype)
    else:
        rows = np.stack([vithip.from16(ctx.match_operands(i, norm, layer, metric), dtype) for i in range(ctx.features_dims()[0])]).astype(np.float64)
    p = np.asarray(pairs)
    return run_tap(rows[p[:, 0]], rows[p[:, 1]], dtype, COS if metric == "cosine" else DOT), rows


@pytest.mark.parametrize("model", list(MODELS))
@TYPES
def test_context_equals_the_tap(dtype, model):
    ctx, images, _ = context(model, dtype, forward=False)
    ctx.set_feature_layers([1])
    ctx.forward(images)
    pairs = [(0, 1), (1, 0), (2, 2), (0, 2), (0, 1)]   # a swapped pair, a == b, image 0 three times, a repeated pair
    for norm in (True, False):
        for layer in (-1, 1):
            for metric in ("cosine", "dot"):
                got = ctx.match_patches(pairs, norm, layer, metric)
                tap, rows = tap_on_features(ctx, pairs, dtype, norm, layer, metric)
                assert np.array_equal(got[0], tap[0]) and np.array_equal(R.bits(got[1]), R.bits(tap[1])), (norm, layer, metric)
                if metric == "cosine":   # a == b: the identity, or a key whose float64 score is within test 2's bound of the identity's
                    s = MR.scores(rows[2], rows[2])
                    bound = rows.shape[-1] * 2.0 ** -23 * MR.scores(np.abs(rows[2]), np.abs(rows[2]))
                    i = np.arange(s.shape[0])
                    assert (s[i, got[0][2]] >= s[i, i] - 2 * bound[i, got[0][2]]).all()
    both = ctx.match_patches([(0, 1), (1, 0)])[0]
    assert vithip.mutual_matches(both[0], both[1]).any()
    ctx.close()


@TYPES
def test_invariance(dtype):
    """A pair's bits do not depend on its place in the list, the forward's streams, a dense head or a bank; the logits see no match."""
    ctx, images, plain = context("fold25", dtype)
    one = ctx.match_patches([(2, 0)])
    five = ctx.match_patches([(0, 0), (1, 2), (0, 1), (2, 2), (2, 0)])
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(R.bits(a[1]), R.bits(b[1]))
    assert same(one, (five[0][4:], five[1][4:]))
    rng = np.random.default_rng(1)
    ctx.set_dense_head(rng.standard_normal((21, 256)).astype(np.float32))
    ctx.set_bank(rng.standard_normal((100, 256)).astype(np.float32))
    assert same(one, ctx.match_patches([(2, 0)]))
    ctx.set_streams(2)
    two = ctx.forward(images)
    assert same(one, ctx.match_patches([(2, 0)]))
    assert np.array_equal(R.bits(two), R.bits(plain)) and np.array_equal(R.bits(ctx.forward(images)), R.bits(plain))
    # the device entry point, asynchronous: the same bits, and an image outside the batch marks its pair without a read
    d_p, d_i, d_s = dev(np.array([2, 0, 3, 0], np.int32)), dev(np.zeros(50, np.int32)), dev(np.zeros(50, np.float32))
    ctx.match_patches_device(vithip.MatchDesc(vithip.FEAT_NORM, -1, COS, 2), d_p.ptr, d_i.ptr, d_s.ptr, sync=False)
    ctx.synchronize()
    i, s = d_i.to_numpy(np.int32, (2, 25)), d_s.to_numpy(np.float32, (2, 25))
    assert same(one, (i[:1], s[:1])) and (i[1] == -1).all() and np.isneginf(s[1]).all()
    for b in (d_p, d_i, d_s):
        b.free()
    ctx.close()


def test_refusals():
    ctx, images, _ = context("micro", BF16, forward=False, extra=vithip.FLAG_LN_FOLD_OFF)   # (no calibration forward at the load)
    with pytest.raises(vithip.VhError, match="match_patches: no forward has run"):
        ctx.match_patches([(0, 0)])
    ctx.forward(images[:2])
    for call, text in ((lambda: ctx.match_patches([(0, 2)]), "names image 2, outside 0..1"),
                       (lambda: ctx.match_patches([(0, 1)], layer=1), "layer 1 was not in the list"),
                       (lambda: ctx.match_patches([(0, 1)], layer=3), "layer 3 is not -1 or 1..2"),
                       (lambda: ctx.match_patches([(0, 1)], metric=2), "metric 2 is not"),
                       (lambda: ctx.match_patches([(0, 1)] * 13), "npairs 13 is outside 1..12"),
                       (lambda: ctx.match_patches_device(vithip.MatchDesc(0, -1, 0, 1), 0x1000, 0x2008, 0x3000), "not 16-byte aligned")):
        with pytest.raises(vithip.VhError, match="match_patches: .*" + text):
            call()
    ctx.close()
    tail = vithip.VitContext(FOLD25, dtype=BF16, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL)
    with pytest.raises(vithip.VhError, match="match_patches: a VH_FLAG_CLS_TAIL context"):
        tail.match_patches([(0, 0)])
    tail.close()
