"""GPU parity of the two CLIP switches, VH_FLAG_PRE_LN and VH_FLAG_QUICK_GELU: the QuickGELU epilogues through the GEMM taps
(16-bit and e4m3 results), the activation itself on a dense grid against the accuracy limit stated with it in gemm_epilogue.h,
the pre-LayerNorm kernel through its tap, whole forwards on every LayerNorm path against tests/vit_ref.py (the C oracle has
neither switch), the fp8 statistics, the Hugging Face fixtures, bit invariance, and the CLIP ViT-B/32 / ViT-L/14 shapes.
Tolerances are the project's own: test_gpu_vit's model bounds (fp16 1e-3, bf16 1e-2), one 16-bit ulp for operators and
test_gpu_fp8's `1.5 x emulation + 1e-3`."""
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as H
import oracle_lib as O
import vh_synth as S
import vit_ref as R
from vh_testlib import _KEEP, _release_buffers, dev, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
DT = [BF16, FP16]
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}   # test_gpu_ops.ULP
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
PRE, QUICK = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU
COMBOS = [(PRE | QUICK, "pre_ln+quick_gelu"), (PRE, "pre_ln"), (QUICK, "quick_gelu")]
LN_PATHS = [(0, "default"), (vithip.FLAG_LN_FOLD_OFF, "fold_off"), (vithip.FLAG_LN_FOLD_ON, "fold_on")]
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "clip", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
# the activation's accuracy limit per result type: the larger of the erf fit's documented absolute error (gemm_epilogue.h) and a
# quarter of the type's unit in the last place at the value
ERF_ABS = {FP16: 7.7e-6, BF16: 3.4e-5, FP8: 5.7e-4}
MANT = {FP16: 10, BF16: 7, FP8: 3}
MIN_EXP = {FP16: -14, BF16: -126, FP8: -6}


def _cfg(image, patch, dim, heads, mlp, layers, classes=40):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


MICRO = S.CONFIGS["vit_micro"]                  # dim 128: the plain LayerNorm path whatever the flags say
MID = _cfg(64, 8, 256, 4, 512, 3)               # 65 tokens, head dim 64, dims multiples of 256: fold + split residual
HD80 = _cfg(64, 8, 1280, 16, 2560, 2)           # the ViT-H/14 block (head dim 80) at depth 2
CLIP_B32 = _cfg(224, 32, 768, 12, 3072, 12, classes=512)    # 50 tokens
CLIP_L14 = _cfg(224, 14, 1024, 16, 4096, 24, classes=768)   # 257 tokens


def rnd16(a, dt):
    return O.round_bf16(a) if dt == BF16 else O.round_fp16(a)


def ulp_at(v, dt):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** MIN_EXP[dt])))
    return 2.0 ** (e - MANT[dt])


def qgelu64(v):
    return R.quick_gelu(np.asarray(v, dtype=np.float64))


def assert_close16(got, ref, dt, extra=0.0):
    tol = ULP[dt] * np.abs(ref) * 1.01 + extra + 1e-30
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} outside 1 ulp; worst {np.abs(got - ref).max():.3e}"


def _forward(cfg, blob, images, dt, flags, layers=-1, eps=1e-6):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags, ln_eps=eps)
    ctx.load_weights(blob)
    if layers >= 0:
        ctx.debug_set_layers(layers)
    got = ctx.forward(images)
    fold = ctx.ln_fold()
    ctx.close()
    return got, fold


# ---- the QuickGELU epilogues through the GEMM taps --------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2, 5, 6, 7])
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gemm_bias_qgelu(dt, variant):
    # whole tiles, ragged rows and ragged columns: the staged, direct and guarded forms of the epilogue, canary rows around the result
    for (M, N, K) in ((512, 512, 256), (300, 260, 128), (256 * 3 + 57, 768, 256)):
        a = rnd16(S.fill(M * K, 61, 1, 0).reshape(M, K) * 2.0, dt)
        w = rnd16(S.fill(N * K, 61, 2, 1, 0.1).reshape(N, K), dt)
        bias = S.fill(N, 61, 3, 1, 0.5)
        pre = O.linear(a, w, bias)
        buf = dev(np.full((M + 2, N), 0x7B7B, np.uint16))
        vithip.op_gemm(dev(vithip.to16(a, dt)).ptr, dev(vithip.to16(w, dt)).ptr, dev(bias).ptr, buf.ptr + N * 2, M, N, K,
                       vithip.EPI_BIAS_QGELU, dt, variant=variant)
        raw = buf.to_numpy(np.uint16, (M + 2, N))
        assert (raw[0] == 0x7B7B).all() and (raw[-1] == 0x7B7B).all(), (M, N, K)
        assert_close16(vithip.from16(raw[1:-1], dt), qgelu64(pre).astype(np.float32), dt, extra=4e-5 * np.abs(pre).max())


@pytest.mark.parametrize("variant", [1, 5, 6])
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gemm_lnfold_qgelu(dt, variant):
    # test_gpu_ops' LNFOLD_GELU case with the other activation: statistics from the row-statistics tap, W' c d from the fold tap
    M, N, K = 256 * 2 + 40, 512, 256
    x = S.fill(M * K, 62, 1, 0).reshape(M, K) * 1.5 + 0.2
    w, b = S.fill(N * K, 62, 2, 1, 0.08).reshape(N, K), S.fill(N, 62, 3, 1, 0.3)
    g, be = 1.0 + S.fill(K, 62, 4, 1, 0.05), S.fill(K, 62, 5, 1, 0.02)
    w16, c, d = vithip.DeviceBuffer(N * K * 2), vithip.DeviceBuffer(N * 4), vithip.DeviceBuffer(N * 4)
    _KEEP.extend([w16, c, d])
    vithip.op_fold_ln(dev(w).ptr, dev(b).ptr, dev(g).ptr, dev(be).ptr, N, K, 1.0, w16.ptr, c.ptr, d.ptr, dt)
    x16, st = vithip.DeviceBuffer(M * K * 2), vithip.DeviceBuffer(M * 8)
    _KEEP.extend([x16, st])
    vithip.op_rowstats_cast(dev(x).ptr, M, K, 1e-6, x16.ptr, st.ptr, dt)
    out = dev(np.zeros((M, N), np.uint16))
    vithip.op_gemm_ex(x16.ptr, w16.ptr, d.ptr, out.ptr, M, N, K, vithip.EPI_LNFOLD_QGELU, dt, aux_ptr=c.ptr, stats_ptr=st.ptr,
                      variant=variant)
    got = vithip.from16(out.to_numpy(np.uint16, (M, N)), dt)
    x64, xr = x.astype(np.float64), rnd16(x, dt).astype(np.float64)
    mean, rstd = x64.mean(1), 1.0 / np.sqrt(x64.var(1) + 1e-6)
    wr = rnd16(g[None, :] * w, dt).astype(np.float64)
    lin = rstd[:, None] * (xr @ wr.T - mean[:, None] * wr.sum(1)[None, :]) + ((w.astype(np.float64) * be[None, :]).sum(1) + b)[None, :]
    assert_close16(got, qgelu64(lin).astype(np.float32), dt, extra=5e-5 * np.abs(lin).max())


def _operands8(M, N, K, seed):
    a = O.quant_e4m3(S.fill(M * K, seed, 1, 0).reshape(M, K) * 2.0)
    w8, wq, sc = O.quantize_rows(S.fill(N * K, seed, 2, 1, 0.1).reshape(N, K))
    return a, vithip.to_e4m3(a), w8, wq, sc, S.fill(N, seed, 3, 1, 0.5)


@pytest.mark.parametrize("variant", [5, 6])
def test_gemm_fp8_qgelu_e4m3_output(variant):
    # BIAS_QGELU (whole and ragged tiles) and LNFOLD_QGELU on e4m3 operands, e4m3 results: within one e4m3 step of the float64
    # function's rounding, nearly all bytes identical (test_gpu_fp8's criterion for the GELU forms)
    for (M, N, K) in ((512, 512, 256), (256 + 70, 264, 256)):
        a, a8, w8, wq, sc, bias = _operands8(M, N, K, 63)
        pre = (O.linear(a, wq) * sc[None, :] + bias[None, :]).astype(np.float64)
        out = dev(np.zeros((M, N), np.uint8))
        vithip.op_gemm_fp8(dev(a8).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPI_BIAS_QGELU, variant)
        got8, want8 = vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), O.quant_e4m3(qgelu64(pre).astype(np.float32))
        step = np.maximum(np.abs(want8), 2.0 ** -6) * 2.0 ** -3 + 1e-12
        assert np.isfinite(got8).all() and np.all(np.abs(got8 - want8) <= step * 1.001), (M, N, K)
        print(f"\n[clip] fp8 BIAS_QGELU {M}x{N}x{K} variant {variant}: identical bytes {(got8 == want8).mean():.4f}")
        assert (got8 == want8).mean() >= 0.97
    M, N, K = 256 * 2 + 31, 512, 256
    a, a8, w8, wq, sc, bias = _operands8(M, N, K, 64)
    st = np.stack([S.fill(M, 65, 1, 1, 0.1), 1.0 + np.abs(S.fill(M, 65, 2, 0))], axis=1).astype(np.float32)
    cvec = S.fill(N, 65, 3, 1, 0.1)
    out = dev(np.zeros((M, N), np.uint8))
    vithip.op_gemm_fp8_ex(dev(a8).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPI_LNFOLD_QGELU,
                          c_ptr=dev(cvec).ptr, stats_ptr=dev(st).ptr, variant=variant)
    pre = (O.linear(a, wq) * sc[None, :]).astype(np.float64)
    lin = st[:, 1:2] * (pre - st[:, 0:1] * cvec[None, :]) + bias[None, :]
    got8, want8 = vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), O.quant_e4m3(qgelu64(lin).astype(np.float32))
    step = np.maximum(np.abs(want8), 2.0 ** -6) * 2.0 ** -3 + 1e-12
    assert np.isfinite(got8).all() and np.all(np.abs(got8 - want8) <= step * 1.001)
    assert (got8 == want8).mean() >= 0.97, (got8 == want8).mean()


# ---- the activation itself ----------------------------------------------------------------------------------------------------

def _sweep_check(v32, got, dt, label):
    """v32: the epilogue's fp32 pre-activation values; got: the stored results as fp32.  The stored value is the function's value
    rounded to the result type: half a unit in the last place for that rounding plus the limit on the function's own error."""
    ref = qgelu64(v32.astype(np.float64))
    u = ulp_at(ref, dt)
    limit = np.maximum(ERF_ABS[dt], 0.25 * u)
    err = np.abs(got.astype(np.float64) - ref)
    fn_err = np.maximum(err - 0.5 * u, 0.0)   # what is left for the function once the result rounding is taken off
    worst = int(np.argmax(fn_err - limit))
    print(f"\n[clip] activation sweep {label}: {v32.size} inputs in [{v32.min():.3g}, {v32.max():.3g}], max |stored - f64| "
          f"{err.max():.3e}, max excess over the result rounding {fn_err.max():.3e} (limit at that input "
          f"{limit.flat[int(np.argmax(fn_err))]:.3e})")
    assert np.isfinite(got).all(), label
    assert np.all(fn_err <= limit * 1.0001), (label, float(v32.flat[worst]), float(got.flat[worst]), float(ref.flat[worst]))


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_activation_sweep_16bit(dt):
    # pre-activation = a_m * 1 + bias_n in fp32: a_m a 16-bit value on a 1/16 grid over [-30, 30] (plus far-out and non-finite
    # rows), bias_n = n / 512 fills the gaps: 320 columns x 970 rows, about 2e-3 apart
    K, N = 128, 320
    grid = np.arange(-30.0, 30.0 + 1e-9, 1.0 / 16.0)
    far = np.array([-60000.0, -1000.0, -100.0, 100.0, 1000.0, 60000.0] if dt == FP16 else [-3e38, -1e30, -1e4, -100.0, 100.0, 1e4, 1e30, 3e38])
    special = np.array([np.inf, -np.inf, np.nan])
    rows = rnd16(np.concatenate([grid, far, special]).astype(np.float32), dt)
    M = rows.size
    a = np.zeros((M, K), np.float32)
    a[:, 0] = rows
    w = np.zeros((N, K), np.float32)
    w[:, 0] = 1.0
    bias = (np.arange(N) / 512.0).astype(np.float32)
    v32 = rows[:, None] + bias[None, :]            # one fp32 addition, as the epilogue's acc + bias
    nfin = grid.size + far.size
    for variant in (1, 5):
        out = dev(np.zeros((M, N), np.uint16))
        vithip.op_gemm(dev(vithip.to16(a, dt)).ptr, dev(vithip.to16(w, dt)).ptr, dev(bias).ptr, out.ptr, M, N, K,
                       vithip.EPI_BIAS_QGELU, dt, variant=variant)
        got = vithip.from16(out.to_numpy(np.uint16, (M, N)), dt)
        _sweep_check(v32[:nfin], got[:nfin], dt, f"{NAME[dt]} variant {variant}")
        neg_far = v32[:nfin] < -200.0
        assert np.all(got[:nfin][neg_far] == 0.0)      # large negative inputs go to -0 / 0, never to NaN
        assert np.all(got[nfin] == np.inf)             # +inf -> +inf
        assert np.isnan(got[nfin + 1]).all()           # -inf * sigmoid(-inf) = -inf * 0: NaN, as the defining expression
        assert np.isnan(got[nfin + 2]).all()           # NaN -> NaN


def test_activation_sweep_e4m3():
    # fp8 operands, e4m3 results: a_m every e4m3 value up to 32 in magnitude, bias_n = n / 256 over a span of 2 (the widest gap)
    K, N = 256, 512
    tab = vithip.e4m3_table()
    vals = np.unique(tab[np.isfinite(tab) & (np.abs(tab) <= 32.0)]).astype(np.float32)
    M = vals.size
    a = np.zeros((M, K), np.float32)
    a[:, 0] = vals
    w8 = np.zeros((N, K), np.uint8)
    w8[:, 0] = vithip.to_e4m3(np.ones(1, np.float32))[0]
    sc = np.ones(N, np.float32)
    bias = (np.arange(N) / 256.0).astype(np.float32)
    v32 = vals[:, None] + bias[None, :]
    out = dev(np.zeros((M, N), np.uint8))
    vithip.op_gemm_fp8(dev(vithip.to_e4m3(a)).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPI_BIAS_QGELU, 5)
    _sweep_check(v32, vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), FP8, "e4m3")


# ---- the pre-LayerNorm kernel through its tap -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 768, 1280, 2048])
@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: NAME[d])
def test_pre_layernorm_tap(dt, dim):
    rows, eps = 203, 1e-5
    x = S.fill(rows * dim, 71, dim, 0).reshape(rows, dim) * 2.0
    x[::3] += 40.0                                   # rows with a large mean: the statistics are two-pass
    x[5] *= 300.0
    gm, bt = 1.0 + S.fill(dim, 71, 2, 1, 0.05), S.fill(dim, 71, 3, 1, 0.02)
    X, G, B = dev(x), dev(gm), dev(bt)
    esz, lsz = (1, 2) if dt == FP8 else (2, 1)
    y32, hi, lo, st = (dev(np.full(n, 0xFF, np.uint8)) for n in (rows * dim * 4, rows * dim * esz, rows * dim * lsz, rows * 8))
    vithip.op_pre_layernorm(X.ptr, rows, dim, G.ptr, B.ptr, eps, y32.ptr, hi.ptr, lo.ptr, st.ptr, dt)
    y = y32.to_numpy(np.float32, (rows, dim))
    ref = R.layernorm(x.astype(np.float64), gm.astype(np.float64), bt.astype(np.float64), eps)
    e = float(np.abs(y - ref).max())
    print(f"\n[clip] pre_layernorm {NAME[dt]} dim {dim}: max |y32 - f64| {e:.3e}")
    assert np.isfinite(y).all() and e <= 2e-5 * np.abs(ref).max()
    # the planes and layer 0's statistics are what the row-statistics kernel makes of y32, bit for bit
    hi2, lo2, st2 = (dev(np.zeros(n, np.uint8)) for n in (rows * dim * esz, rows * dim * lsz, rows * 8))
    vithip.op_rowstats_split(y32.ptr, rows, dim, eps, hi2.ptr, lo2.ptr, st2.ptr, dt)
    for a, b, n in ((hi, hi2, rows * dim * esz), (lo, lo2, rows * dim * lsz), (st, st2, rows * 8)):
        assert np.array_equal(a.to_numpy(np.uint8, (n,)), b.to_numpy(np.uint8, (n,)))
    y64 = y.astype(np.float64)
    stats = st.to_numpy(np.float32, (rows, 2))
    assert np.allclose(stats[:, 0], y64.mean(1), atol=1e-5) and np.allclose(stats[:, 1], 1.0 / np.sqrt(y64.var(1) + eps), rtol=1e-5)
    # every output is optional: y32 alone in place (the plain path), the operand copy alone (the non-split fold)
    x_inplace = dev(x)
    vithip.op_pre_layernorm(x_inplace.ptr, rows, dim, G.ptr, B.ptr, eps, x_inplace.ptr, None, None, None, dt)
    assert np.array_equal(x_inplace.to_numpy(np.float32, (rows, dim)), y)
    hi3, st3 = dev(np.zeros(rows * dim * esz, np.uint8)), dev(np.zeros(rows * 8, np.uint8))
    vithip.op_pre_layernorm(X.ptr, rows, dim, G.ptr, B.ptr, eps, None, hi3.ptr, None, st3.ptr, dt)
    assert np.array_equal(hi3.to_numpy(np.uint8, (rows * dim * esz,)), hi.to_numpy(np.uint8, (rows * dim * esz,)))
    assert np.array_equal(st3.to_numpy(np.uint8, (rows * 8,)), st.to_numpy(np.uint8, (rows * 8,)))


# ---- whole forwards -----------------------------------------------------------------------------------------------------------

_REF = {}


def _model(name, cfg, flags, seed=3, batch=3, eps=1e-5):
    key = (name, flags)
    if key not in _REF:
        blob, images = R.make_blob(cfg, seed, flags, eps), S.make_images(cfg, seed + 1, batch)
        _REF[key] = (blob, images, R.forward(cfg, blob, images, flags, eps).astype(np.float32))
    return _REF[key]


MODELS = [("micro", MICRO), ("mid", MID)]


@pytest.mark.parametrize("flags,fname", COMBOS, ids=[c[1] for c in COMBOS])
@pytest.mark.parametrize("name,cfg", MODELS, ids=[m[0] for m in MODELS])
def test_models_match_clip_ref_on_every_layernorm_path(name, cfg, flags, fname):
    blob, images, ref = _model(name, cfg, flags)
    for dt in DT:
        for lnf, label in LN_PATHS:
            got, fold = _forward(cfg, blob, images, dt, flags | lnf, eps=1e-5)
            e = rel(got, ref)
            print(f"\n[clip] {name} {fname} {NAME[dt]} {label} (fold {fold}): logits {e:.3e}")
            assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], label, e)
            if cfg["dim"] % 256 == 0 and lnf != vithip.FLAG_LN_FOLD_OFF:
                assert fold, label


@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: NAME[d])
def test_debug_read_after_zero_layers_returns_the_pre_layernormed_rows(dt):
    cfg, flags = MID, PRE | QUICK
    blob, images, _ = _model("mid", cfg, flags)
    _, want = R.forward(cfg, blob, images, flags, 1e-5, n_layers=0, want_hidden=True)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags, ln_eps=1e-5)
    ctx.load_weights(blob)
    ctx.debug_set_layers(0)
    ctx.forward(images)
    rows = ctx.debug_read(0, want.size).reshape(want.shape)
    ctx.close()
    e = rel(rows, want)
    print(f"\n[clip] rows after the pre-LayerNorm {NAME[dt]}: {e:.3e}")
    # the patch GEMM multiplies 16-bit operands: the rows carry that rounding, amplified by 1 / sigma of the embedded row
    assert np.isfinite(rows).all() and e <= (1e-2 if dt != FP16 else 2e-3)
    assert abs(float(rows.mean())) < 0.1 and 0.5 < float(rows.std()) < 2.0   # normalised, not the raw embedding (sigma 0.03)


@pytest.mark.parametrize("flags,fname", COMBOS, ids=[c[1] for c in COMBOS])
def test_fp8_forwards_track_the_emulation(flags, fname):
    cfg = MID
    blob, images, ref32 = _model("mid", cfg, flags)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    emu = {}
    for lnf, label in LN_PATHS:
        got, folded = _forward(cfg, blob, images, FP8, flags | lnf, eps=1e-5)
        if folded not in emu:
            emu[folded] = R.forward(cfg, blob, images, flags, 1e-5, fp8="folded" if folded else "plain")
        r_emu32, r_gpu32, r_gpuemu = rms(emu[folded], ref32), rms(got, ref32), rms(got, emu[folded])
        print(f"\n[clip fp8] mid {fname} {label} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
        assert np.isfinite(got).all()
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3, label
        assert r_gpuemu <= 1.5 * r_emu32 + 1e-3, label


@pytest.mark.parametrize("name,cfg", MODELS, ids=[m[0] for m in MODELS])
def test_weight_only_e4m3(name, cfg):
    flags = PRE | QUICK
    blob, images, _ = _model(name, cfg, flags)
    blob_q = R.weight_only_e4m3_blob(cfg, blob, flags)
    got, _ = _forward(cfg, blob, images, FP16, flags | vithip.FLAG_W8_E4M3, eps=1e-5)
    host_quantised, _ = _forward(cfg, blob_q, images, FP16, flags, eps=1e-5)
    e = rel(got, R.forward(cfg, blob_q, images, flags, 1e-5))
    print(f"\n[clip] {name} fp16 weight-only e4m3 vs its own fp64 model: {e:.3e}")
    assert np.isfinite(got).all() and np.array_equal(got, host_quantised)
    assert e <= MODEL_TOL[FP16], e


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_clip_fixture_logits_match_the_hugging_face_fp64_logits(path):
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    wseed, iseed, batch, flags = [int(v) for v in g["meta"]]
    eps = float(g["ln_eps"])
    tensors = H.make_clip_tensors(cfg, wseed, flags) if int(g["zero_bias"]) else R.make_tensors(cfg, wseed, flags)
    blob, images = R.pack_blob(cfg, tensors, flags, eps), S.make_images(cfg, iseed, batch)
    for dt in DT:
        got, _ = _forward(cfg, blob, images, dt, flags, eps=eps)
        e = rel(got, g["logits_f64"])
        print(f"\n[clip] fixture {os.path.basename(path)} {NAME[dt]}: logits vs the fp64 golden {e:.3e}")
        assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], e)


def test_the_three_fixtures_exist():
    assert len(GOLDEN) == 3, GOLDEN


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_same_bits_across_batch_streams_graph_replay_and_the_class_token_tail_to_rounding(dt):
    cfg, flags = MID, PRE | QUICK
    blob, _, _ = _model("mid", cfg, flags)
    images = S.make_images(cfg, 8, 7)
    ref = R.forward(cfg, blob, images, flags, 1e-5).astype(np.float32)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=7, flags=flags, ln_eps=1e-5)
    ctx.load_weights(blob)
    one = ctx.forward(images[:1])
    seven = ctx.forward(images)
    assert np.isfinite(seven).all() and np.array_equal(seven[:1], one)
    ctx.set_streams(2)
    assert np.array_equal(ctx.forward(images), seven)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert np.array_equal(ctx.forward(images), seven)
    ctx.set_streams(2)
    for _ in range(3):
        assert np.array_equal(ctx.forward(images), seven)
    ctx.set_graph(False)
    ctx.close()
    # the class-token tail (head dim 64, folded path): the small fc1 launch with the QuickGELU code; logits to rounding
    base, _ = _forward(cfg, blob, images, dt, flags | vithip.FLAG_LN_FOLD_ON, eps=1e-5)
    tail, _ = _forward(cfg, blob, images, dt, flags | vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL, eps=1e-5)
    print(f"\n[clip] class-token tail {NAME[dt]}: tail vs full {rel(tail, base):.3e}, tail vs vit_ref {rel(tail, ref):.3e}")
    assert np.isfinite(tail).all() and rel(tail, ref) <= MODEL_TOL[dt] and rel(tail, base) <= MODEL_TOL[dt]


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_hd80_with_both_flags_and_the_tiled_hidden_activation(dt):
    # the ViT-H/14 block at depth 2 with enough rows for the persistent GEMM form: fc1's QuickGELU result leaves in the tiled
    # layout (debug tap 3); the first images against vit_ref, the whole batch against VH_H_TILED=0, bit for bit
    cfg, flags, n = HD80, PRE | QUICK, 420
    blob, images = R.make_blob(cfg, 3, flags, 1e-5), S.make_images(cfg, 4, n)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=n, flags=flags, ln_eps=1e-5)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    tiled = int(ctx.debug_read(3, 1)[0])
    ctx.close()
    ref = R.forward(cfg, blob, images[:3], flags, 1e-5).astype(np.float32)
    print(f"\n[clip] hd80 b{n} {NAME[dt]}: h tiled {tiled}, logits {rel(got[:3], ref):.3e}")
    assert tiled == 1
    assert np.isfinite(got).all() and rel(got[:3], ref) <= MODEL_TOL[dt]
    os.environ["VH_H_TILED"] = "0"
    try:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=n, flags=flags, ln_eps=1e-5)
    finally:
        del os.environ["VH_H_TILED"]
    ctx.load_weights(blob)
    plain = ctx.forward(images)
    assert int(ctx.debug_read(3, 1)[0]) == 0
    ctx.close()
    assert np.array_equal(plain, got)


def test_hd80_fp8_with_both_flags_tiled_e4m3_hidden_activation():
    cfg, flags, n = HD80, PRE | QUICK, 420
    blob, images = R.make_blob(cfg, 3, flags, 1e-5), S.make_images(cfg, 4, n)
    outs = []
    for tiled_env in (None, "0"):
        if tiled_env is not None:
            os.environ["VH_H_TILED"] = tiled_env
        try:
            ctx = vithip.VitContext(cfg, dtype=FP8, max_batch=n, flags=flags, ln_eps=1e-5)
        finally:
            os.environ.pop("VH_H_TILED", None)
        ctx.load_weights(blob)
        outs.append(ctx.forward(images))
        assert int(ctx.debug_read(3, 1)[0]) == (1 if tiled_env is None else 0)
        ctx.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


# ---- blob: seeded tensors, header bits ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,fname", COMBOS, ids=[c[1] for c in COMBOS])
def test_seeded_weights_are_clip_refs_blob_and_the_header_bits_are_checked(flags, fname, tmp_path):
    cfg = MICRO
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags, ln_eps=1e-5)
    ctx.init_weights_seeded(17)
    blob = ctx.export_weights()
    assert np.array_equal(blob, R.make_blob(cfg, 17, flags, 1e-5))      # pre_ln.* from tensor ids 5 and 6; bits in the header
    path = str(tmp_path / "m.vhblob")
    ctx.save_weights_file(path)
    assert vithip.blob_file_flags(path) == flags
    images = S.make_images(cfg, 2, 2)
    want = ctx.forward(images)
    ctx.load_weights_file(path)
    assert np.array_equal(ctx.forward(images), want) and np.array_equal(ctx.export_weights(), blob)
    ctx.close()
    # a context with other model bits refuses the blob and the file, naming the bit
    for other in (0, PRE, QUICK, PRE | QUICK):
        if other == flags:
            continue
        c2 = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=other, ln_eps=1e-5)
        mine = R.make_blob(cfg, 17, other, 1e-5)
        if mine.nbytes == blob.nbytes:   # same size (the pre-LN bit agrees): only the QuickGELU bit tells them apart
            with pytest.raises(vithip.VhError, match="QuickGELU"):
                c2.load_weights(blob)
            with pytest.raises(vithip.VhError, match="QuickGELU"):
                c2.load_weights_file(path)
        else:
            with pytest.raises(vithip.VhError):
                c2.load_weights(blob)
            forged = mine.copy()          # the right size with the other model's bits
            forged[52:56] = blob[52:56]
            with pytest.raises(vithip.VhError, match="pre-LayerNorm"):
                c2.load_weights(forged)
        c2.load_weights(mine)             # and its own blob loads
        c2.close()


def test_stage_timing_knows_the_pre_layernorm_stage():
    cfg, flags = MID, PRE | QUICK
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=4, flags=flags, ln_eps=1e-5)
    ctx.init_weights_seeded(1)
    din, dout = vithip.DeviceBuffer(4 * 64 * 64 * 3 * 4), vithip.DeviceBuffer(4 * cfg["classes"] * 4)
    _KEEP.extend([din, dout])
    ctx.fill_input_seeded(1, 4, din.ptr)
    ctx.set_stage_timing("pre_layernorm")
    ctx.forward_device_async(din.ptr, 4, dout.ptr, steps=3)
    ctx.synchronize()
    avg_ms, min_ms, n = ctx.get_stage_timing()
    ctx.set_stage_timing(None)
    prof = ctx.profile_forward(din.ptr, 4, dout.ptr)
    ctx.close()
    assert n == 3 and avg_ms > 0 and prof["pre_layernorm"][1] == 1 and prof["ln_stats"][1] == 2 * cfg["layers"] - 1


# ---- the CLIP shapes ------------------------------------------------------------------------------------------------------------
# Nobody had measured these shapes: each test runs the SAME shape with neither flag against the C oracle and asserts the CLIP
# context's error at no more than 1.25 x that run's (the switches add no 16-bit rounding point; the factor allows for the
# scatter across images, 7.7e-4 .. 9.0e-4 on ViT-H/14), and at the project's model bound.  Measured values: profiles/clip_gpu_tests.txt.

@pytest.mark.parametrize("name,cfg,batch", [("clip_vit_b32_224", CLIP_B32, 3), ("clip_vit_l14_224", CLIP_L14, 2)])
def test_clip_shapes_against_clip_ref_fp32(name, cfg, batch):
    flags, eps = PRE | QUICK, 1e-5
    blob_c, images = R.make_blob(cfg, 0, flags, eps), S.make_images(cfg, 1, batch)
    ref_c = R.forward(cfg, blob_c, images, flags, eps, dtype=np.float32)
    blob_p = O.make_blob(cfg, 0, eps)
    ref_p = O.vit_forward(cfg, blob_p, images, ln_eps=eps)
    for dt in (FP16, BF16):
        got_c, _ = _forward(cfg, blob_c, images, dt, flags, eps=eps)
        got_p, _ = _forward(cfg, blob_p, images, dt, 0, eps=eps)
        e_c, e_p = rel(got_c, ref_c), rel(got_p, ref_p)
        print(f"\n[clip] {name} {NAME[dt]} b{batch}: CLIP flags vs vit_ref fp32 {e_c:.3e}; no flag vs the oracle {e_p:.3e}; ratio {e_c / e_p:.2f}")
        assert np.isfinite(got_c).all() and np.isfinite(got_p).all()
        assert e_c <= 1.25 * e_p, (NAME[dt], e_c, e_p)
        assert e_c <= MODEL_TOL[dt], (NAME[dt], e_c)
