"""GPU suite of the token features (include/vithip.h, "Token features").  The contract is written for bits, so nearly every
comparison below is equality: the raw rows are vh_debug_read(0), the normalised class-token rows are vh_debug_read(1), the mean
is the sequential fp32 chain over the call's own fp32 patch rows, the 16-bit outputs are the RNE of the fp32 ones.  The one
tolerance is the normalised patch rows against an fp64 LayerNorm: max|got - ref| <= 2^-18 max|ref| (features_ref.NORM_BOUND; a
lane-strided fp32 two-pass LayerNorm stays below 3.1e-7 of max|ref| for D 64..2048 on rows with |mean| <= sigma and a 300 sigma
outlier, the bound is 12 x that, and a dropped lo plane would cost 2^-9 / 2^-12 of |x|)."""
import ctypes as C

import numpy as np
import pytest

import features_ref as R
import oracle_lib as O
import vh_synth as S
import vithip
from tensor_ref import make_u8_images, u8_reference
from test_u8_input import DEFAULT_SCALE

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_UNSUPPORTED = 1, 3, 4
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
F32, F16, B16 = vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16
NORM, RAW = vithip.FEAT_NORM, vithip.FEAT_RAW
SEED, EPS = 11, 1e-6
KEYS = ("cls", "patch", "mean")

# name: (config, dtype, flags, does it fold)
CASES = {
    "fold_bf16": (R.FEAT_FOLD, BF16, 0, True),
    "fold_fp16": (R.FEAT_FOLD, FP16, 0, True),
    "fold_fp8": (R.FEAT_FOLD, FP8, 0, True),
    "fold_off_bf16": (R.FEAT_FOLD, BF16, vithip.FLAG_LN_FOLD_OFF, False),
    "mini_bf16": (S.CONFIGS["vit_mini"], BF16, 0, False),
}
ALL_CASES = list(CASES)


def make_ctx(case, max_batch=5):
    cfg, dtype, flags, folds = CASES[case]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=max_batch, flags=flags, ln_eps=EPS)
    ctx.load_weights(S.make_blob(cfg, SEED, EPS))
    assert ctx.ln_fold() == folds, case   # the path the case is meant to cover
    return ctx, cfg


def final_ln(cfg):
    t = S.make_tensors(cfg, SEED)
    return t["lnf.weight"], t["lnf.bias"]


def residual(ctx, cfg, batch):
    T, D = S.tokens(cfg), cfg["dim"]
    return ctx.debug_read(0, batch * T * D).reshape(batch, T, D)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(R.bits(a), R.bits(b))


def assert_same(fa, fb, keys=None):
    for k in keys or fa.keys():
        assert same_bits(fa[k], fb[k]), k


class Guarded:
    """A device buffer with 64 canary bytes in front of and behind the `nbytes` a call may write."""
    CANARY = 0xA5

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = vithip.DeviceBuffer.from_numpy(np.full(self.n + 128, self.CANARY, dtype=np.uint8))
        self.ptr = self.buf.ptr + 64

    def read(self, dtype, shape):
        raw = self.buf.to_numpy(np.uint8, (self.n + 128,))
        assert (raw[:64] == self.CANARY).all() and (raw[64 + self.n:] == self.CANARY).all(), "canary bytes overwritten"
        return raw[64:64 + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.to_numpy(np.uint8, (self.n + 128,)) == self.CANARY).all())

    def free(self):
        self.buf.free()


def read_device(ctx, want=KEYS, elem=F32, norm=NORM, how="sync"):
    """The device entry points into guarded buffers -> dict of numpy arrays (canaries checked)."""
    b, _, n, d = ctx.features_dims()
    dt = {F32: np.float32, F16: np.float16, B16: np.uint16}[elem]
    shape = {"cls": (b, d), "patch": (b, n, d), "mean": (b, d)}
    bufs = {k: Guarded(int(np.prod(shape[k])) * np.dtype(dt).itemsize) for k in want}
    desc = vithip.Features(*(bufs[k].ptr if k in bufs else None for k in KEYS), elem, norm)
    if how == "async":
        ctx.read_features_device_async(desc)
        ctx.synchronize()
    else:
        ctx.read_features_device(desc)
    out = {k: bufs[k].read(dt, shape[k]) for k in want}
    for g in bufs.values():
        g.free()
    return out


# ---- 1. RAW is the residual stream ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_raw_rows_are_the_residual_stream(case):
    ctx, cfg = make_ctx(case)
    images = S.make_images(cfg, 1, 3)
    for layers in (-1, 1):
        ctx.debug_set_layers(layers)
        ctx.forward(images)
        x = residual(ctx, cfg, 3)
        assert np.isfinite(x).all()
        f = ctx.read_features(cls=True, patch=True, mean=False, elem=F32, norm=RAW)
        assert same_bits(f["cls"], x[:, 0, :]) and same_bits(f["patch"], x[:, 1:, :]), layers
        assert_same(read_device(ctx, ("cls", "patch"), F32, RAW), f)
    ctx.close()


# ---- 2. NORM ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_normalised_rows_mean_and_cls(case):
    ctx, cfg = make_ctx(case)
    gamma, beta = final_ln(cfg)
    images = S.make_images(cfg, 2, 3)
    for layers in (-1, 1):
        ctx.debug_set_layers(layers)
        ctx.forward(images)
        x = residual(ctx, cfg, 3)
        f = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=NORM)
        assert same_bits(f["cls"], ctx.debug_read(1, 3 * cfg["dim"]).reshape(3, cfg["dim"]))
        ref = R.layernorm64(x[:, 1:, :], gamma, beta, EPS)
        err, top = float(np.abs(f["patch"] - ref).max()), float(np.abs(ref).max())
        print(f"{case} layers {layers}: max|patch - fp64 LayerNorm| = {err:.3e} = {err / top:.3e} max|ref| (bound {R.NORM_BOUND:.3e})")
        assert err <= R.NORM_BOUND * top
        assert same_bits(f["mean"], R.mean_chain(f["patch"]))
        # and the raw mean: the same chain over the raw rows
        g = ctx.read_features(cls=False, patch=True, mean=True, elem=F32, norm=RAW)
        assert same_bits(g["mean"], R.mean_chain(g["patch"]))
    ctx.close()


# ---- 3. element types -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "fold_fp8", "mini_bf16"])
@pytest.mark.parametrize("norm", [NORM, RAW], ids=["norm", "raw"])
def test_16bit_outputs_are_the_rne_of_the_fp32_outputs(case, norm):
    ctx, cfg = make_ctx(case)
    ctx.forward(S.make_images(cfg, 3, 3))
    f32 = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=norm)
    for elem in (F16, B16):
        f16 = ctx.read_features(cls=True, patch=True, mean=True, elem=elem, norm=norm)
        dev = read_device(ctx, KEYS, elem, norm)
        for k in KEYS:
            assert np.array_equal(R.bits(f16[k]), R.rne16(f32[k], elem)), (k, elem)
            assert same_bits(dev[k], f16[k]), (k, elem)
    ctx.close()


# ---- 4. independence: of the batch, of the outputs requested, of how the forward was launched -------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "mini_bf16"])
@pytest.mark.parametrize("norm", [NORM, RAW], ids=["norm", "raw"])
def test_outputs_do_not_depend_on_batch_request_or_launch(case, norm):
    ctx, cfg = make_ctx(case, max_batch=5)
    images = S.make_images(cfg, 4, 5)
    ctx.forward(images)
    full = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=norm)
    # image 2 alone, on a context sized for one image
    one, _ = make_ctx(case, max_batch=1)
    one.forward(images[2:3])
    alone = one.read_features(cls=True, patch=True, mean=True, elem=F32, norm=norm)
    one.close()
    for k in KEYS:
        assert same_bits(alone[k][0], full[k][2]), k
    # a mean-only and a patch-only call
    assert_same(ctx.read_features(cls=False, patch=False, mean=True, elem=F32, norm=norm), full, ["mean"])
    assert_same(ctx.read_features(cls=False, patch=True, mean=False, elem=F32, norm=norm), full, ["patch"])
    assert_same(read_device(ctx, ("mean",), F32, norm), full, ["mean"])
    # graph replay of the second of two steps, then two streams
    d_in = vithip.DeviceBuffer.from_numpy(images)
    d_out = vithip.DeviceBuffer(5 * cfg["classes"] * 4)
    ctx.set_graph(True)
    ctx.forward_device_async(d_in.ptr, 5, d_out.ptr, steps=2)
    assert_same(read_device(ctx, KEYS, F32, norm, how="async"), full)
    ctx.set_graph(False)
    ctx.set_streams(2)
    ctx.forward_device(d_in.ptr, 5, d_out.ptr)
    assert_same(read_device(ctx, KEYS, F32, norm), full)
    d_in.free()
    d_out.free()
    ctx.close()


# ---- 5. read-only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "fold_fp8", "mini_bf16"])
def test_reading_features_changes_nothing(case):
    ctx, cfg = make_ctx(case)
    images = S.make_images(cfg, 5, 4)
    logits = ctx.forward(images)
    guard = ctx.ln_guard() if CASES[case][3] else None
    first = read_device(ctx, KEYS, B16, NORM)      # (the canaries around every buffer are checked inside)
    second = read_device(ctx, KEYS, B16, NORM)
    assert_same(first, second)
    # a NULL pointer: that output is not written -- a buffer the call never saw stays as it was, the others match
    spare = Guarded(4 * S.tokens(cfg) * cfg["dim"] * 2)
    assert_same(read_device(ctx, ("cls", "mean"), B16, NORM), first, ["cls", "mean"])
    assert spare.untouched()
    spare.free()
    assert_same(ctx.read_features(cls=True, patch=True, mean=True, elem=B16, norm=NORM), first)
    if guard is not None:
        assert ctx.ln_guard() == guard
    again = ctx.forward(images)
    assert np.array_equal(again.view(np.uint32), logits.view(np.uint32))
    ctx.close()


# ---- 6. any input kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "mini_bf16"])
def test_features_after_a_u8_forward_equal_those_after_the_fp32_forward(case):
    ctx, cfg = make_ctx(case)
    ch = cfg["channels"]
    u8 = make_u8_images(2, cfg["image_size"], ch, seed=9)
    ctx.forward_u8(u8)
    a = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=NORM)
    ctx.forward(u8_reference(u8, np.full(ch, DEFAULT_SCALE), np.zeros(ch, np.float32)))
    assert_same(ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=NORM), a)
    ctx.close()


# ---- 7. the operator tap on synthetic planes --------------------------------------------------------------------------------
FORMS = {"bf16_planes": BF16, "fp16_planes": FP16, "fp8_planes": FP8, "fp32_rows": vithip.FEAT_FORM_F32}


@pytest.mark.parametrize("dim", [64, 192, 768, 1280, 2048])
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
def test_operator_tap(dim, form):
    fm = FORMS[form]
    rng = np.random.default_rng(dim + 7 * (fm + 2))
    gamma = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.02 * rng.standard_normal(dim)).astype(np.float32)
    d_g, d_b = vithip.DeviceBuffer.from_numpy(gamma), vithip.DeviceBuffer.from_numpy(beta)
    for tokens in (2, 5, 50):
        for batch in (1, 3):
            hi, lo, x = R.split_planes(R.rows_with_outlier(rng, batch, tokens, dim), fm)
            x = x.reshape(batch, tokens, dim)
            d_hi = vithip.DeviceBuffer.from_numpy(hi)
            d_lo = vithip.DeviceBuffer.from_numpy(lo) if lo is not None else None
            n_patch, n_mean = batch * (tokens - 1) * dim, batch * dim

            def run(elem, norm, want_patch=True, want_mean=True):
                es = 4 if elem == F32 else 2
                dt = {F32: np.float32, F16: np.float16, B16: np.uint16}[elem]
                gp, gm = Guarded(n_patch * es), Guarded(n_mean * es)
                vithip.op_token_features(d_hi.ptr, d_lo.ptr if d_lo else None, fm, batch, tokens, dim, d_g.ptr, d_b.ptr, EPS, elem, norm,
                                         gp.ptr if want_patch else None, gm.ptr if want_mean else None)
                out = (gp.read(dt, (batch, tokens - 1, dim)) if want_patch else gp.untouched(),
                       gm.read(dt, (batch, dim)) if want_mean else gm.untouched())
                gp.free()
                gm.free()
                return out

            where = (form, dim, tokens, batch)
            patch, mean = run(F32, RAW)
            assert same_bits(patch, x[:, 1:, :]), where
            assert same_bits(mean, R.mean_chain(patch)), where
            patch, mean = run(F32, NORM)
            ref = R.layernorm64(x[:, 1:, :], gamma, beta, EPS)
            assert np.abs(patch - ref).max() <= R.NORM_BOUND * np.abs(ref).max(), where
            assert same_bits(mean, R.mean_chain(patch)), where
            # either output alone gives the same bits and leaves the other buffer alone; 16-bit results are the RNE of these
            p_only, m_clean = run(F32, NORM, want_mean=False)
            p_clean, m_only = run(F32, NORM, want_patch=False)
            assert same_bits(p_only, patch) and same_bits(m_only, mean) and m_clean is True and p_clean is True, where
            p16, m16 = run(B16, NORM)
            assert np.array_equal(p16, R.rne16(patch, B16)) and np.array_equal(m16, R.rne16(mean, B16)), where
            d_hi.free()
            if d_lo:
                d_lo.free()
    d_g.free()
    d_b.free()


# ---- 8. refusals on a live context ------------------------------------------------------------------------------------------
def refused(ctx, fn, code, cls=None, patch=None, mean=None, elem=F32, norm=NORM):
    desc = vithip.Features(cls, patch, mean, elem, norm)
    rc = fn(ctx.h, C.byref(desc))
    assert rc == code, (rc, vithip.lib().vh_last_error(ctx.h))
    return vithip.lib().vh_last_error(ctx.h).decode()


def test_refusals_leave_the_outputs_untouched():
    L = vithip.lib()
    cfg = R.FEAT_FOLD
    T, D = S.tokens(cfg), cfg["dim"]
    blob = S.make_blob(cfg, SEED, EPS)
    images = S.make_images(cfg, 6, 2)
    host = np.full((2, T - 1, D), 7.5, dtype=np.float32)
    dev = Guarded(2 * (T - 1) * D * 4)
    msgs = []

    def both(ctx, code, **kw):
        """The refusal through the host call and through both device calls; no buffer is written."""
        msgs.append(refused(ctx, L.vh_read_features, code, **{k: (host.ctypes.data if v == "buf" else v) for k, v in kw.items()}))
        for fn in (L.vh_read_features_device, L.vh_read_features_device_async):
            refused(ctx, fn, code, **{k: (dev.ptr if v == "buf" else v) for k, v in kw.items()})
        assert (host == 7.5).all() and dev.untouched()

    # before any forward: a context without weights, then one whose weight load ran no calibration image (the fold is off)
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=2, ln_eps=EPS)
    both(ctx, VH_ERR_STATE, patch="buf")
    assert ctx.features_dims() == (0, T, T - 1, D)
    ctx.close()
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_OFF)
    ctx.load_weights(blob)
    both(ctx, VH_ERR_STATE, patch="buf")
    # a live context: the argument refusals
    ctx.forward(images)
    assert ctx.features_dims() == (2, T, T - 1, D)
    both(ctx, VH_ERR_INVALID, patch="buf", elem=vithip.ELEM_U8)
    both(ctx, VH_ERR_INVALID, patch="buf", norm=2)
    both(ctx, VH_ERR_INVALID)                                       # all three NULL
    for fn in (L.vh_read_features_device, L.vh_read_features_device_async):
        msgs.append(refused(ctx, fn, VH_ERR_INVALID, patch=dev.ptr + 8))   # misaligned device pointer
        assert fn(ctx.h, None) == VH_ERR_INVALID                           # null descriptor
    assert dev.untouched()
    # a ring on the context: its forwards belong to slots
    ctx.ring_create(2, 1)
    both(ctx, VH_ERR_STATE, patch="buf")
    assert L.vh_ring_destroy(ctx.h) == 0
    ok = ctx.read_features(cls=False, patch=True, mean=False)         # and the context reads again
    assert np.isfinite(ok["patch"]).all()
    ctx.close()
    # the class-token tail: the last layer leaves the other rows behind
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL)
    ctx.load_weights(blob)
    ctx.forward(images)
    both(ctx, VH_ERR_UNSUPPORTED, patch="buf")
    ctx.close()
    dev.free()
    distinct = set(msgs)
    assert len(distinct) >= 7, distinct   # no forward, elem, norm, all NULL, misaligned, ring, class-token tail


# ---- 9. end to end against the oracle: reported, asserted finite only -------------------------------------------------------
def test_features_against_the_oracle_end_to_end():
    """The tight checks are tests 1 and 2; the residual stream's parity with the oracle is asserted by the existing suite.  This
    one prints rel = max|d| / max|ref| of the normalised features beside the rel of the hidden state they are made from."""
    cfg = R.FEAT_FOLD
    blob = S.make_blob(cfg, SEED, EPS)
    images = S.make_images(cfg, 8, 3)
    gamma, beta = final_ln(cfg)
    T, D = S.tokens(cfg), cfg["dim"]
    _, hidden = O.vit_forward(cfg, blob, images, want_hidden=True, ln_eps=EPS)
    hidden = hidden.reshape(3, T, D)
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=3, ln_eps=EPS)
    ctx.load_weights(blob)
    assert ctx.ln_fold()
    ctx.forward(images)
    x = residual(ctx, cfg, 3)
    f = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=NORM)
    ctx.close()
    ref = R.layernorm64(hidden, gamma, beta, EPS)
    rel_hidden = float(np.abs(x - hidden).max() / np.abs(hidden).max())
    rel_patch = float(np.abs(f["patch"] - ref[:, 1:, :]).max() / np.abs(ref[:, 1:, :]).max())
    rel_cls = float(np.abs(f["cls"] - ref[:, 0, :]).max() / np.abs(ref[:, 0, :]).max())
    rel_mean = float(np.abs(f["mean"] - ref[:, 1:, :].mean(axis=1)).max() / np.abs(ref[:, 1:, :].mean(axis=1)).max())
    print(f"feat_fold fp16 b3 against the oracle: rel(hidden) = {rel_hidden:.3e}, rel(patch) = {rel_patch:.3e}, "
          f"rel(cls) = {rel_cls:.3e}, rel(mean) = {rel_mean:.3e}")
    assert all(np.isfinite(v) for v in (rel_hidden, rel_patch, rel_cls, rel_mean))
    assert all(np.isfinite(f[k]).all() for k in KEYS)
