"""GPU suite of the layer features (include/vithip.h, "Layer features").  As in test_gpu_features nearly every comparison is equality
of bits: a captured layer is the truncated forward's residual stream, the final state is vh_read_features, the channels-first
patch map is the rows output transposed, the mean is the sequential fp32 chain, 16-bit outputs are the RNE of the fp32 ones.  The
one tolerance is the existing one: normalised rows against an fp64 LayerNorm, max|got - ref| <= 2^-18 max|ref|
(features_ref.NORM_BOUND, derived in test_gpu_features' docstring; the kernels' arithmetic is the same device functions)."""
import ctypes as C

import numpy as np
import pytest

import features_ref as R
import layer_features_ref as LR
import vh_synth as S
import vit_ref as RR
import vithip
from layer_features_ref import Guarded

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_UNSUPPORTED = 1, 3, 4
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
F32, F16, B16 = vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16
NORM, RAW = vithip.FEAT_NORM, vithip.FEAT_RAW
ROWS, NCHW = vithip.FEAT_ROWS, vithip.FEAT_NCHW
SEED, EPS = 11, 1e-6
KEYS = ("cls", "patch", "mean", "reg")
LIST = [1, 3, 4]
REGS = 4

# 96^2 / 16: a 6 x 6 grid, NP = 36 (ragged against a 32-token tile), T = 37 (41 with four registers), four layers
FOLD4 = dict(R.FEAT_FOLD, layers=4)
MINI4 = dict(S.CONFIGS["vit_mini"], layers=4)
# name: (config, dtype, flags, does it fold)
CASES = {
    "fold_bf16": (FOLD4, BF16, 0, True),
    "fold_fp16": (FOLD4, FP16, 0, True),
    "fold_fp8": (FOLD4, FP8, 0, True),
    "fold_off_bf16": (FOLD4, BF16, vithip.FLAG_LN_FOLD_OFF, False),
    "mini_bf16": (MINI4, BF16, 0, False),
    "fold_reg4_bf16": (FOLD4, BF16, vithip.FLAG_REGISTERS(REGS), True),
}
ALL_CASES = list(CASES)
_blobs = {}


def model(case):
    """(config, blob, final LayerNorm gamma, beta, register tokens) of a case; made once."""
    if case not in _blobs:
        cfg, _, flags, _ = CASES[case]
        mflags = flags & vithip.FLAG_REGISTERS(31)
        t = RR.make_tensors(cfg, SEED, mflags)
        _blobs[case] = (cfg, RR.pack_blob(cfg, t, mflags, EPS), t["lnf.weight"], t["lnf.bias"], RR.registers_of(mflags))
    return _blobs[case]


def make_ctx(case, max_batch=5, layers=None):
    cfg, dtype, flags, folds = CASES[case]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=max_batch, flags=flags, ln_eps=EPS)
    ctx.load_weights(model(case)[1])
    assert ctx.ln_fold() == folds, case   # the path the case is meant to cover
    if layers is not None:
        ctx.set_feature_layers(layers)
        assert ctx.feature_layers() == list(layers)
    return ctx, cfg


def same_bits(a, b):
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(R.bits(a), R.bits(b))


def assert_same(fa, fb, keys=None):
    for k in keys or fa.keys():
        assert same_bits(fa[k], fb[k]), k


def read_device(ctx, layer, want=("cls", "patch"), elem=F32, norm=NORM, layout=ROWS, how="sync"):
    """The device entry points into guarded buffers -> dict of numpy arrays (canaries checked); a channels-first patch map comes
    back as [B, D, NP]."""
    b, _, n, d = ctx.features_dims()
    r = ctx.register_tokens()
    dt = LR.NP_DTYPE[elem]
    shape = {"cls": (b, d), "patch": (b, d, n) if layout == NCHW else (b, n, d), "mean": (b, d), "reg": (b, r, d)}
    bufs = {k: Guarded(int(np.prod(shape[k])) * np.dtype(dt).itemsize) for k in want}
    desc = vithip.LayerFeatures(*(bufs[k].ptr if k in bufs else None for k in KEYS), elem, norm, layer, layout)
    if how == "async":
        ctx.read_layer_features_device_async(desc)
        ctx.synchronize()
    else:
        ctx.read_layer_features_device(desc)
    out = {k: bufs[k].read(dt, shape[k]) for k in want}
    for g in bufs.values():
        g.free()
    return out


def truncated(case, images, k, max_batch=5):
    """What the existing calls give for layer k: a context that runs k layers, then vh_read_features and the residual stream."""
    ctx, cfg = make_ctx(case, max_batch)
    ctx.debug_set_layers(k)
    ctx.forward(images)
    b, t, _, d = ctx.features_dims()
    out = {"raw": ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=RAW),
           "norm": ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=NORM),
           "x": ctx.debug_read(0, b * t * d).reshape(b, t, d)}
    ctx.close()
    return out


# ---- 1. a captured layer is the truncated forward ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_captured_layers_are_the_truncated_forwards(case):
    ctx, cfg = make_ctx(case, layers=LIST)
    _, _, gamma, beta, regs = model(case)
    images = S.make_images(cfg, 1, 3)
    ctx.forward(images)
    for k in LIST:
        ref = truncated(case, images, k)
        raw = ctx.read_layer_features(k, cls=True, patch=True, reg=regs > 0, norm=RAW)
        assert np.isfinite(raw["patch"]).all()
        assert same_bits(raw["cls"], ref["raw"]["cls"]) and same_bits(raw["patch"], ref["raw"]["patch"]), k
        assert same_bits(raw["patch"], ref["x"][:, 1 + regs:, :]) and same_bits(raw["cls"], ref["x"][:, 0, :]), k
        if regs:
            assert same_bits(raw["reg"], ref["x"][:, 1:1 + regs, :]), k
        nrm = ctx.read_layer_features(k, cls=True, patch=True, reg=regs > 0, norm=NORM)
        assert same_bits(nrm["patch"], ref["norm"]["patch"]), k   # same kernel, same input
        for key in ("patch",) + (("reg",) if regs else ()):
            want = LR.outputs(ref["x"], 1 + regs, gamma, beta, EPS)[key]
            err, top = float(np.abs(nrm[key] - want).max()), float(np.abs(want).max())
            print(f"{case} layer {k} {key}: max|got - fp64 LayerNorm| = {err:.3e} = {err / top:.3e} max|ref| (bound {R.NORM_BOUND:.3e})")
            assert err <= R.NORM_BOUND * top, (k, key)
        assert_same(read_device(ctx, k, ("cls", "patch"), F32, RAW), raw, ["cls", "patch"])
    ctx.close()


# ---- 2. the final state is vh_read_features ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
@pytest.mark.parametrize("norm", [NORM, RAW], ids=["norm", "raw"])
def test_final_state_equals_read_features(case, norm):
    ctx, cfg = make_ctx(case, layers=LIST)
    ctx.forward(S.make_images(cfg, 2, 3))
    old = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=norm)
    for layer in (-1, cfg["layers"]):
        assert_same(ctx.read_layer_features(layer, cls=True, patch=True, mean=True, norm=norm), old)
        assert_same(read_device(ctx, layer, ("cls", "patch", "mean"), F32, norm), old)
    if norm == NORM:   # the class-token rows the head multiplied
        assert same_bits(old["cls"], ctx.debug_read(1, 3 * cfg["dim"]).reshape(3, cfg["dim"]))
    ctx.close()


# ---- 3. the register rows ---------------------------------------------------------------------------------------------------
def test_register_rows():
    case = "fold_reg4_bf16"
    ctx, cfg = make_ctx(case, layers=LIST)
    _, _, gamma, beta, regs = model(case)
    ctx.forward(S.make_images(cfg, 3, 3))
    b, t, n, d = ctx.features_dims()
    assert (t, n) == (37 + REGS, 36) and regs == REGS
    x = ctx.debug_read(0, b * t * d).reshape(b, t, d)
    with_reg = ctx.read_layer_features(-1, cls=True, patch=True, reg=True, norm=RAW)
    assert same_bits(with_reg["reg"], x[:, 1:1 + REGS, :]) and with_reg["reg"].shape == (3, REGS, d)
    assert_same(ctx.read_layer_features(-1, cls=True, patch=True, norm=RAW), with_reg, ["cls", "patch"])
    nrm = ctx.read_layer_features(-1, cls=True, patch=True, reg=True, norm=NORM)
    want = LR.outputs(x, 1 + REGS, gamma, beta, EPS)["reg"]
    assert np.abs(nrm["reg"] - want).max() <= R.NORM_BOUND * np.abs(want).max()
    assert_same(ctx.read_layer_features(-1, cls=True, patch=True, norm=NORM), nrm, ["cls", "patch"])
    assert_same(ctx.read_features(cls=True, patch=True, norm=NORM), nrm, ["cls", "patch"])
    # alone, through the device call, in 16 bits
    dev = read_device(ctx, -1, ("reg",), B16, NORM)
    assert np.array_equal(dev["reg"], R.rne16(nrm["reg"], B16))
    ctx.close()


# ---- 4. channels-first ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "fold_fp8", "mini_bf16", "fold_reg4_bf16"])
def test_nchw_is_the_rows_output_transposed(case):
    ctx, cfg = make_ctx(case, layers=LIST)
    ctx.forward(S.make_images(cfg, 4, 3))
    g = cfg["image_size"] // cfg["patch_size"]
    for layer in (3, -1):
        for norm in (NORM, RAW):
            for elem in (F32, F16, B16):
                rows = read_device(ctx, layer, ("cls", "patch", "mean"), elem, norm, ROWS)
                chw = read_device(ctx, layer, ("cls", "patch", "mean"), elem, norm, NCHW)
                where = (case, layer, norm, elem)
                assert same_bits(chw["patch"], LR.nchw(rows["patch"])), where
                assert same_bits(chw["cls"], rows["cls"]) and same_bits(chw["mean"], rows["mean"]), where
                only = read_device(ctx, layer, ("patch",), elem, norm, NCHW)
                assert same_bits(only["patch"], chw["patch"]), where
            host = ctx.read_layer_features(layer, cls=False, patch=True, norm=norm, nchw=True)["patch"]
            assert host.shape == (3, cfg["dim"], g, g)
            assert same_bits(LR.rows_of(host), ctx.read_layer_features(layer, cls=False, patch=True, norm=norm)["patch"])
    ctx.close()


FORMS = {"bf16_planes": BF16, "fp16_planes": FP16, "fp8_planes": FP8, "fp32_rows": vithip.FEAT_FORM_F32}


@pytest.mark.parametrize("dim", [64, 200, 768, 2048])
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
def test_operator_tap_nchw_and_register_rows(dim, form):
    fm = FORMS[form]
    rng = np.random.default_rng(dim + 7 * (fm + 2))
    gamma = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.02 * rng.standard_normal(dim)).astype(np.float32)
    d_g, d_b = vithip.DeviceBuffer.from_numpy(gamma), vithip.DeviceBuffer.from_numpy(beta)
    for n_patch in (1, 5, 31, 33, 36):
        for batch in (1, 3):
            for lead in (1, 5):
                tokens = lead + n_patch
                hi, lo, x = R.split_planes(R.rows_with_outlier(rng, batch, tokens, dim), fm)
                x = x.reshape(batch, tokens, dim)
                d_hi = vithip.DeviceBuffer.from_numpy(hi)
                d_lo = vithip.DeviceBuffer.from_numpy(lo) if lo is not None else None

                def run(elem, norm, layout, want_mean=True):
                    es, dt = np.dtype(LR.NP_DTYPE[elem]).itemsize, LR.NP_DTYPE[elem]
                    gp, gm = Guarded(batch * n_patch * dim * es), Guarded(batch * dim * es)
                    gr = Guarded(batch * (lead - 1) * dim * es) if lead > 1 else None
                    vithip.op_token_features2(d_hi.ptr, d_lo.ptr if d_lo else None, fm, batch, tokens, lead, dim, d_g.ptr, d_b.ptr, EPS, elem,
                                              norm, gp.ptr, layout, gm.ptr if want_mean else None, gr.ptr if gr else None)
                    out = (gp.read(dt, (batch, dim, n_patch) if layout == NCHW else (batch, n_patch, dim)),
                           gm.read(dt, (batch, dim)) if want_mean else gm.untouched(),
                           gr.read(dt, (batch, lead - 1, dim)) if gr else None)
                    for g in (gp, gm, gr):
                        if g:
                            g.free()
                    return out

                where = (form, dim, n_patch, batch, lead)
                want = LR.outputs(x, lead)
                # raw: the rows themselves, in both layouts; the mean is the chain over them whichever kernel wrote the patch rows
                p_rows, m_rows, r_rows = run(F32, RAW, ROWS)
                p_chw, m_chw, r_chw = run(F32, RAW, NCHW)
                assert same_bits(p_rows, want["patch"]) and same_bits(p_chw, LR.nchw(want["patch"])), where
                assert same_bits(m_rows, R.mean_chain(p_rows)) and same_bits(m_chw, m_rows), where
                if lead > 1:
                    assert same_bits(r_rows, want["reg"]) and same_bits(r_chw, want["reg"]), where
                # normalised: within the bound of the fp64 LayerNorm, and channels-first is bit for bit the transposed rows output
                p_rows, m_rows, r_rows = run(F32, NORM, ROWS)
                p_chw, m_chw, r_chw = run(F32, NORM, NCHW)
                ref = LR.outputs(x, lead, gamma, beta, EPS)
                assert np.abs(p_rows - ref["patch"]).max() <= R.NORM_BOUND * np.abs(ref["patch"]).max(), where
                assert same_bits(p_chw, LR.nchw(p_rows)), where
                assert same_bits(m_rows, R.mean_chain(p_rows)) and same_bits(m_chw, m_rows), where
                if lead > 1:
                    assert np.abs(r_rows - ref["reg"]).max() <= R.NORM_BOUND * np.abs(ref["reg"]).max(), where
                    assert same_bits(r_chw, r_rows), where
                # without the mean the other buffer stays as it was; 16-bit results are the RNE of the fp32 ones
                p_only, m_clean, _ = run(F32, NORM, NCHW, want_mean=False)
                assert same_bits(p_only, p_chw) and m_clean is True, where
                for elem in (B16, F16):
                    p16, m16, r16 = run(elem, NORM, NCHW)
                    assert np.array_equal(R.bits(p16), R.rne16(p_chw, elem)) and np.array_equal(R.bits(m16), R.rne16(m_chw, elem)), where
                    if lead > 1:
                        assert np.array_equal(R.bits(r16), R.rne16(r_chw, elem)), where
                d_hi.free()
                if d_lo:
                    d_lo.free()
    d_g.free()
    d_b.free()


# ---- 5. the mean of an intermediate layer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "fold_fp8", "mini_bf16", "fold_reg4_bf16"])
def test_mean_is_the_chain_over_the_calls_own_patch_rows(case):
    ctx, cfg = make_ctx(case, layers=LIST)
    ctx.forward(S.make_images(cfg, 5, 3))
    for layer in (1, 3):
        for norm in (NORM, RAW):
            f = ctx.read_layer_features(layer, cls=False, patch=True, mean=True, norm=norm)
            assert same_bits(f["mean"], R.mean_chain(f["patch"])), (layer, norm)
            assert_same(ctx.read_layer_features(layer, cls=False, patch=False, mean=True, norm=norm), f, ["mean"])
            h = ctx.read_layer_features(layer, cls=False, patch=True, mean=True, norm=norm, nchw=True)
            assert same_bits(h["mean"], f["mean"]), (layer, norm)
    ctx.close()


# ---- 6. nothing else moves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_logits_do_not_move_and_a_cleared_list_reads_nothing(case):
    ctx, cfg = make_ctx(case, layers=LIST)
    plain, _ = make_ctx(case)
    images = S.make_images(cfg, 6, 4)
    with_list = ctx.forward(images)
    assert np.array_equal(with_list.view(np.uint32), plain.forward(images).view(np.uint32))
    assert plain.feature_layers() == []
    plain.close()
    ctx.read_layer_features(1, cls=True, patch=True)
    ctx.set_feature_layers([])
    assert ctx.feature_layers() == []
    for layer, again in ((1, False), (1, True)):
        if again:
            assert np.array_equal(ctx.forward(images).view(np.uint32), with_list.view(np.uint32))
        with pytest.raises(vithip.VhError) as e:
            ctx.read_layer_features(layer, cls=True, patch=True)
        assert e.value.code == VH_ERR_STATE and "not in the list" in str(e.value)
    assert_same(ctx.read_layer_features(-1), ctx.read_features())   # the final state needs no list
    ctx.close()


# ---- 7. image independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "mini_bf16", "fold_reg4_bf16"])
def test_an_image_alone_gives_the_bits_it_gives_inside_a_batch(case):
    ctx, cfg = make_ctx(case, max_batch=5, layers=LIST)
    images = S.make_images(cfg, 4, 5)
    ctx.forward(images)
    one, _ = make_ctx(case, max_batch=1, layers=LIST)
    one.forward(images[2:3])
    regs = model(case)[4] > 0
    for layer in (1, 3):
        for norm in (NORM, RAW):
            full = ctx.read_layer_features(layer, cls=True, patch=True, mean=True, reg=regs, norm=norm)
            alone = one.read_layer_features(layer, cls=True, patch=True, mean=True, reg=regs, norm=norm)
            for k in full:
                assert same_bits(alone[k][0], full[k][2]), (layer, norm, k)
    one.close()
    ctx.close()


# ---- 8. enqueue forms: graph replay and several streams ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "mini_bf16"])
def test_graph_replay_and_streams_capture_the_same_rows(case):
    ctx, cfg = make_ctx(case, max_batch=5, layers=LIST)
    first, second = S.make_images(cfg, 7, 5), S.make_images(cfg, 8, 5)
    ctx.forward(second)
    want = {k: ctx.read_layer_features(k, cls=True, patch=True, mean=True, norm=NORM) for k in (1, 3, 4)}
    d_in = vithip.DeviceBuffer.from_numpy(first)
    d_out = vithip.DeviceBuffer(5 * cfg["classes"] * 4)
    ctx.set_graph(True)
    ctx.forward_device(d_in.ptr, 5, d_out.ptr)     # eager: the batch size's first forward
    ctx.forward_device(d_in.ptr, 5, d_out.ptr)     # captured and launched
    assert ctx.get_graph()[1] >= 1
    assert not same_bits(ctx.read_layer_features(1, cls=False, patch=True)["patch"], want[1]["patch"])   # (the first images' rows)
    vithip._check(vithip.lib().vh_memcpy_h2d(0, d_in.ptr, second.ctypes.data, second.nbytes))
    ctx.forward_device_async(d_in.ptr, 5, d_out.ptr)   # replayed: the same buffer now holds the second images
    for k in (1, 3, 4):
        assert_same(read_device(ctx, k, ("cls", "patch", "mean"), F32, NORM, how="async"), want[k])
    ctx.set_graph(False)
    for streams in (2, 4):
        ctx.set_streams(streams)
        ctx.forward_device(d_in.ptr, 5, d_out.ptr)
        for k in (1, 3, 4):
            assert_same(ctx.read_layer_features(k, cls=True, patch=True, mean=True, norm=NORM), want[k])
    d_in.free()
    d_out.free()
    ctx.close()


# ---- 9. repeatability -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "fold_fp8", "mini_bf16"])
def test_reading_twice_gives_the_same_bits_and_changes_nothing(case):
    ctx, cfg = make_ctx(case, layers=LIST)
    images = S.make_images(cfg, 5, 4)
    logits = ctx.forward(images)
    first = read_device(ctx, 3, ("cls", "patch", "mean"), B16, NORM, NCHW)      # (the canaries around every buffer are checked inside)
    second = read_device(ctx, 3, ("cls", "patch", "mean"), B16, NORM, NCHW)
    assert_same(first, second)
    spare = Guarded(4 * S.tokens(cfg) * cfg["dim"] * 2)
    assert_same(read_device(ctx, 3, ("cls", "mean"), B16, NORM, NCHW), first, ["cls", "mean"])
    assert spare.untouched()
    spare.free()
    again = ctx.forward(images)
    assert np.array_equal(again.view(np.uint32), logits.view(np.uint32))
    assert_same(read_device(ctx, 3, ("cls", "patch", "mean"), B16, NORM, NCHW), first)
    ctx.close()


# ---- 10. the Python helper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fold_bf16", "mini_bf16"])
def test_get_intermediate_layers(case):
    ctx, cfg = make_ctx(case)
    images = S.make_images(cfg, 9, 3)
    ctx.forward(images)
    with pytest.raises(vithip.VhError) as e:        # the list is set by the call; the forward before it captured nothing
        ctx.get_intermediate_layers(2, reshape=True, return_class_token=True)
    assert e.value.code == VH_ERR_STATE and ctx.feature_layers() == [3, 4]
    ctx.forward(images)
    got = ctx.get_intermediate_layers(2, reshape=True, return_class_token=True)
    g, d = cfg["image_size"] // cfg["patch_size"], cfg["dim"]
    assert isinstance(got, tuple) and len(got) == 2
    for (patch, cls), k in zip(got, (3, 4)):
        assert patch.shape == (3, d, g, g) and cls.shape == (3, d)
        ref = truncated(case, images, k)
        assert same_bits(LR.rows_of(patch), ref["norm"]["patch"]), k
        if k == 4:
            assert same_bits(cls, ref["norm"]["cls"])
    rows = ctx.get_intermediate_layers([2, 3], norm=False)
    assert ctx.feature_layers() == [3, 4] and rows[0].shape == (3, g * g, d)
    assert same_bits(rows[0], truncated(case, images, 3)["raw"]["patch"])
    ctx.close()


# ---- 11. refusals on live contexts ------------------------------------------------------------------------------------------
def refused(ctx, fn, code, **kw):
    d = dict(cls=None, patch=None, mean=None, reg=None, elem=F32, norm=NORM, layer=-1, patch_layout=ROWS)
    d.update(kw)
    desc = vithip.LayerFeatures(d["cls"], d["patch"], d["mean"], d["reg"], d["elem"], d["norm"], d["layer"], d["patch_layout"])
    rc = fn(ctx.h, C.byref(desc))
    assert rc == code, (rc, vithip.lib().vh_last_error(ctx.h))
    return vithip.lib().vh_last_error(ctx.h).decode()


def test_refusals_leave_the_outputs_untouched():
    L = vithip.lib()
    cfg = FOLD4
    T, D = S.tokens(cfg), cfg["dim"]
    blob = model("fold_bf16")[1]
    images = S.make_images(cfg, 6, 2)
    host = np.full((2, T - 1, D), 7.5, dtype=np.float32)
    dev = Guarded(2 * (T - 1) * D * 4)
    msgs = []

    def both(ctx, code, **kw):
        """The refusal through the host call and through both device calls; no buffer is written."""
        msgs.append(refused(ctx, L.vh_read_layer_features, code, **{k: (host.ctypes.data if v == "buf" else v) for k, v in kw.items()}))
        for fn in (L.vh_read_layer_features_device, L.vh_read_layer_features_device_async):
            refused(ctx, fn, code, **{k: (dev.ptr if v == "buf" else v) for k, v in kw.items()})
        assert (host == 7.5).all() and dev.untouched()

    def set_refused(ctx, code, layers):
        arr = (C.c_int * max(len(layers), 1))(*layers)
        assert L.vh_set_feature_layers(ctx.h, arr, len(layers)) == code, L.vh_last_error(ctx.h)
        msgs.append(L.vh_last_error(ctx.h).decode())

    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=2, ln_eps=EPS)
    both(ctx, VH_ERR_STATE, patch="buf")                                        # no forward has run
    ctx.load_weights(blob)
    ctx.set_feature_layers([1, 3])
    ctx.forward(images)
    both(ctx, VH_ERR_INVALID, patch="buf", elem=vithip.ELEM_U8)
    both(ctx, VH_ERR_INVALID, patch="buf", norm=2)
    both(ctx, VH_ERR_INVALID, patch="buf", patch_layout=2)
    both(ctx, VH_ERR_INVALID)                                                   # all four NULL
    for layer in (0, -2, 5):
        both(ctx, VH_ERR_INVALID, patch="buf", layer=layer)
    both(ctx, VH_ERR_INVALID, reg="buf")                                        # no register tokens on this context
    both(ctx, VH_ERR_STATE, patch="buf", layer=2)                               # not in the list
    for fn in (L.vh_read_layer_features_device, L.vh_read_layer_features_device_async):
        msgs.append(refused(ctx, fn, VH_ERR_INVALID, patch=dev.ptr + 8))        # misaligned device pointer
        assert fn(ctx.h, None) == VH_ERR_INVALID                                # null descriptor
    assert dev.untouched()
    # the last forward did not reach the layer
    ctx.debug_set_layers(2)
    ctx.forward(images)
    both(ctx, VH_ERR_STATE, patch="buf", layer=3)
    both(ctx, VH_ERR_STATE, patch="buf", layer=4)
    assert np.isfinite(ctx.read_layer_features(1)["patch"]).all()               # (layer 1 was reached and captured)
    ctx.debug_set_layers(-1)
    ctx.forward(images)
    # the list itself
    for bad in ([0], [5], [2, 2], [3, 1], list(range(1, 10))):
        set_refused(ctx, VH_ERR_INVALID, bad)
    assert ctx.feature_layers() == [1, 3]                                       # the previous list stays in force
    assert np.isfinite(ctx.read_layer_features(3)["patch"]).all()
    # a ring on the context: its forwards belong to slots
    ctx.ring_create(2, 1)
    both(ctx, VH_ERR_STATE, patch="buf")
    set_refused(ctx, VH_ERR_STATE, [1])
    assert L.vh_ring_destroy(ctx.h) == 0
    assert np.isfinite(ctx.read_layer_features(3)["patch"]).all()               # and the context reads again
    ctx.close()
    # the class-token tail: the last layer leaves the other rows behind
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL)
    ctx.load_weights(blob)
    ctx.forward(images)
    both(ctx, VH_ERR_UNSUPPORTED, patch="buf")
    set_refused(ctx, VH_ERR_UNSUPPORTED, [1])
    ctx.close()
    dev.free()
    distinct = set(msgs)
    # no forward, elem, norm, layout, all NULL, layer range, reg, not listed, misaligned, not reached, 4 kinds of bad list, ring x 2, tail x 2
    assert len(distinct) >= 17, distinct
