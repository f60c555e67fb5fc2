"""GPU suite of SigLIP's two switches, VH_FLAG_TANH_GELU and VH_FLAG_MAP_HEAD: the tanh-GELU epilogues through the GEMM taps (16-bit
and e4m3 results, direct and LN-fold codes) and the activation itself on test_gpu_clip's grid against the limits stated with the
QuickGELU form in gemm_epilogue.h; the one-pass kernel of the attention-pooling head through vh_op_map_pool against float64 with
canaries around every output; whole forwards against the three Hugging Face fixtures; the head's stages; bit invariance across batch,
streams, graph replay and the u8 ring; forged blobs; token features.  Tolerances: the project's model bounds (fp16 1e-3, bf16 1e-2,
fp8 `1.5 x emulation + 1e-3`), one 16-bit ulp for operators, and for the kernel MAP_BOUND, which tests/test_siglip.py measures.
The taps here store row-major on random data; the LAYOUTS of the two tanh codes -- the tiled hidden activation with 16-bit and e4m3
results, a tile range, canaries per element -- are held by the exact suite (tests/test_gpu_gemm_exact.py) on exact pre-activations."""
import glob
import os

import numpy as np
import pytest

import features_ref as FR
import hf_state_dicts as HF
import oracle_lib as O
import vh_synth as S
import vit_ref as R
from layer_features_ref import Guarded
from tensor_ref import make_u8_images, u8_reference
from test_siglip import MAP_BOUND, fixture_blob, load_fixture
from test_u8_input import DEFAULT_SCALE
from vh_testlib import _KEEP, _release_buffers, dev, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
DT = [BF16, FP16]
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8", vithip.FEAT_FORM_F32: "f32"}
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}   # test_gpu_ops.ULP
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
NO_CLS, POOL, MAP, TANH = vithip.FLAG_NO_CLS, vithip.FLAG_POOL, vithip.FLAG_MAP_HEAD, vithip.FLAG_TANH_GELU
F32, NORM, RAW = vithip.ELEM_F32, vithip.FEAT_NORM, vithip.FEAT_RAW
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "siglip", "*.npz")))
EPS = HF.MAP_EPS
# the activation's accuracy limit per result type (test_gpu_clip's): the larger of the erf fit's documented absolute
# error and a quarter of the type's unit in the last place at the value
ERF_ABS = {FP16: 7.7e-6, BF16: 3.4e-5, FP8: 5.7e-4}
MANT = {FP16: 10, BF16: 7, FP8: 3}
MIN_EXP = {FP16: -14, BF16: -126, FP8: -6}
A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=256)   # fold + split residual
B = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=128)   # the fp32 residual path
MAPF = NO_CLS | MAP | TANH


def rnd16(a, dt):
    return O.round_bf16(a) if dt == BF16 else O.round_fp16(a)


def ulp_at(v, dt):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** MIN_EXP[dt])))
    return 2.0 ** (e - MANT[dt])


def tgelu64(v):
    return R.tanh_gelu(np.asarray(v, dtype=np.float64))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(FR.bits(a), FR.bits(b))


def assert_close16(got, ref, dt, extra=0.0):
    tol = ULP[dt] * np.abs(ref) * 1.01 + extra + 1e-30
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} outside 1 ulp; worst {np.abs(got - ref).max():.3e}"


def context(cfg, dt, flags, max_batch=5, seed=5, extra=0):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=max_batch, flags=flags | extra, ln_eps=EPS)
    ctx.load_weights(R.make_blob(cfg, seed, flags, EPS))
    return ctx


# ---- 1. the tanh-GELU epilogues through the GEMM taps, and the activation itself --------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2, 5, 6, 7])
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gemm_bias_tgelu(dt, variant):
    # whole tiles, ragged rows and ragged columns: the staged, direct and guarded forms of the epilogue, canary rows around the result
    for (M, N, K) in ((512, 512, 256), (300, 260, 128), (256 * 3 + 57, 768, 256)):
        a = rnd16(S.fill(M * K, 61, 1, 0).reshape(M, K) * 2.0, dt)
        w = rnd16(S.fill(N * K, 61, 2, 1, 0.1).reshape(N, K), dt)
        bias = S.fill(N, 61, 3, 1, 0.5)
        pre = O.linear(a, w, bias)
        buf = dev(np.full((M + 2, N), 0x7B7B, np.uint16))
        vithip.op_gemm(dev(vithip.to16(a, dt)).ptr, dev(vithip.to16(w, dt)).ptr, dev(bias).ptr, buf.ptr + N * 2, M, N, K,
                       vithip.EPILOGUE_BIAS_TGELU, dt, variant=variant)
        raw = buf.to_numpy(np.uint16, (M + 2, N))
        assert (raw[0] == 0x7B7B).all() and (raw[-1] == 0x7B7B).all(), (M, N, K)
        assert_close16(vithip.from16(raw[1:-1], dt), tgelu64(pre).astype(np.float32), dt, extra=4e-5 * np.abs(pre).max())


@pytest.mark.parametrize("variant", [1, 5, 6])
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gemm_lnfold_tgelu(dt, variant):
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
    vithip.op_gemm_ex(x16.ptr, w16.ptr, d.ptr, out.ptr, M, N, K, vithip.EPILOGUE_LNFOLD_TGELU, dt, aux_ptr=c.ptr, stats_ptr=st.ptr, variant=variant)
    got = vithip.from16(out.to_numpy(np.uint16, (M, N)), dt)
    x64, xr = x.astype(np.float64), rnd16(x, dt).astype(np.float64)
    mean, rstd = x64.mean(1), 1.0 / np.sqrt(x64.var(1) + 1e-6)
    wr = rnd16(g[None, :] * w, dt).astype(np.float64)
    lin = rstd[:, None] * (xr @ wr.T - mean[:, None] * wr.sum(1)[None, :]) + ((w.astype(np.float64) * be[None, :]).sum(1) + b)[None, :]
    assert_close16(got, tgelu64(lin).astype(np.float32), dt, extra=5e-5 * np.abs(lin).max())


def _operands8(M, N, K, seed):
    a = O.quant_e4m3(S.fill(M * K, seed, 1, 0).reshape(M, K) * 2.0)
    w8, wq, sc = O.quantize_rows(S.fill(N * K, seed, 2, 1, 0.1).reshape(N, K))
    return a, vithip.to_e4m3(a), w8, wq, sc, S.fill(N, seed, 3, 1, 0.5)


@pytest.mark.parametrize("variant", [5, 6])
def test_gemm_fp8_tgelu_e4m3_output(variant):
    # BIAS_TGELU (whole and ragged tiles) and LNFOLD_TGELU on e4m3 operands, e4m3 results: test_gpu_clip's criterion for the QuickGELU forms
    for (M, N, K) in ((512, 512, 256), (256 + 70, 264, 256)):
        a, a8, w8, wq, sc, bias = _operands8(M, N, K, 63)
        pre = (O.linear(a, wq) * sc[None, :] + bias[None, :]).astype(np.float64)
        out = dev(np.zeros((M, N), np.uint8))
        vithip.op_gemm_fp8(dev(a8).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPILOGUE_BIAS_TGELU, variant)
        got8, want8 = vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), O.quant_e4m3(tgelu64(pre).astype(np.float32))
        step = np.maximum(np.abs(want8), 2.0 ** -6) * 2.0 ** -3 + 1e-12
        assert np.isfinite(got8).all() and np.all(np.abs(got8 - want8) <= step * 1.001), (M, N, K)
        assert (got8 == want8).mean() >= 0.97
    M, N, K = 256 * 2 + 31, 512, 256
    a, a8, w8, wq, sc, bias = _operands8(M, N, K, 64)
    st = np.stack([S.fill(M, 65, 1, 1, 0.1), 1.0 + np.abs(S.fill(M, 65, 2, 0))], axis=1).astype(np.float32)
    cvec = S.fill(N, 65, 3, 1, 0.1)
    out = dev(np.zeros((M, N), np.uint8))
    vithip.op_gemm_fp8_ex(dev(a8).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPILOGUE_LNFOLD_TGELU,
                          c_ptr=dev(cvec).ptr, stats_ptr=dev(st).ptr, variant=variant)
    pre = (O.linear(a, wq) * sc[None, :]).astype(np.float64)
    lin = st[:, 1:2] * (pre - st[:, 0:1] * cvec[None, :]) + bias[None, :]
    got8, want8 = vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), O.quant_e4m3(tgelu64(lin).astype(np.float32))
    step = np.maximum(np.abs(want8), 2.0 ** -6) * 2.0 ** -3 + 1e-12
    assert np.isfinite(got8).all() and np.all(np.abs(got8 - want8) <= step * 1.001)
    assert (got8 == want8).mean() >= 0.97, (got8 == want8).mean()


def _sweep_check(v32, got, dt, label):
    """v32: the epilogue's fp32 pre-activation values; got: the stored results as fp32.  The stored value is the function's value
    rounded to the result type: half a unit in the last place for that rounding plus the limit on the function's own error."""
    ref = tgelu64(v32.astype(np.float64))
    u = ulp_at(ref, dt)
    limit = np.maximum(ERF_ABS[dt], 0.25 * u)
    err = np.abs(got.astype(np.float64) - ref)
    fn_err = np.maximum(err - 0.5 * u, 0.0)
    worst = int(np.argmax(fn_err - limit))
    print(f"\n[siglip] activation sweep {label}: {v32.size} inputs in [{v32.min():.3g}, {v32.max():.3g}], max |stored - f64| "
          f"{err.max():.3e}, max excess over the result rounding {fn_err.max():.3e} (limit at that input "
          f"{limit.flat[int(np.argmax(fn_err))]:.3e})")
    assert np.isfinite(got).all(), label
    assert np.all(fn_err <= limit * 1.0001), (label, float(v32.flat[worst]), float(got.flat[worst]), float(ref.flat[worst]))


@pytest.mark.parametrize("epi", ["direct", "fold"])
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_activation_sweep_16bit(dt, epi):
    # test_gpu_clip's grid: pre-activation = a_m * 1 + bias_n in fp32, a_m a 16-bit value on a 1/16 grid over [-30, 30] (plus far-out
    # and non-finite rows), bias_n = n / 512: 320 columns x 970 rows, about 2e-3 apart.  fold: the LN-fold code with mean 0, rstd 1, c 0
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
    v32 = rows[:, None] + bias[None, :]            # one fp32 addition (fold: fmaf(1, acc, fmaf(-0, 0, bias)), the same value)
    nfin = grid.size + far.size
    st = np.tile(np.array([0.0, 1.0], np.float32), (M, 1))
    for variant in (1, 5):
        out = dev(np.zeros((M, N), np.uint16))
        if epi == "direct":
            vithip.op_gemm(dev(vithip.to16(a, dt)).ptr, dev(vithip.to16(w, dt)).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPILOGUE_BIAS_TGELU, dt,
                           variant=variant)
        else:
            vithip.op_gemm_ex(dev(vithip.to16(a, dt)).ptr, dev(vithip.to16(w, dt)).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPILOGUE_LNFOLD_TGELU, dt,
                              aux_ptr=dev(np.zeros(N, np.float32)).ptr, stats_ptr=dev(st).ptr, variant=variant)
        got = vithip.from16(out.to_numpy(np.uint16, (M, N)), dt)
        _sweep_check(v32[:nfin], got[:nfin], dt, f"{NAME[dt]} {epi} variant {variant}")
        neg_far = v32[:nfin] < -200.0
        assert np.all(got[:nfin][neg_far] == 0.0)      # large negative inputs go to -0 / 0, never to NaN
        assert np.all(got[nfin] == np.inf)             # +inf -> +inf
        assert np.isnan(got[nfin + 1]).all()           # -inf * 0: NaN, as the defining expression
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
    vithip.op_gemm_fp8(dev(vithip.to_e4m3(a)).ptr, dev(w8).ptr, dev(sc).ptr, dev(bias).ptr, out.ptr, M, N, K, vithip.EPILOGUE_BIAS_TGELU, 5)
    _sweep_check(v32, vithip.from_e4m3(out.to_numpy(np.uint8, (M, N))), FP8, "e4m3")


# ---- 2. the kernel alone ----------------------------------------------------------------------------------------------------------
FORMS = {"bf16_planes": BF16, "fp16_planes": FP16, "fp8_planes": FP8, "fp32_rows": vithip.FEAT_FORM_F32}


@pytest.mark.parametrize("dim", HF.MAP_DIMS)
def test_map_pool_kernel_against_float64(dim):
    """vh_op_map_pool on the inputs of hf_state_dicts.map_pool_cases, every case in all four input forms, canaries around the output: finite,
    and max |z - z64| / max |z64| within MAP_BOUND of the case's class (4 x the float32 statement's error, tests/test_siglip.py)."""
    worst = {}
    for heads, NP, lead, batch, order in HF.map_pool_cases(dim):
        x, gamma, beta, qk = HF.map_pool_inputs(dim, heads, NP, lead, batch, order)
        d_g, d_b, d_q = dev(gamma), dev(beta), dev(qk)
        for form, fm in FORMS.items():
            hi, lo, xr = FR.split_planes(x.reshape(-1, dim), fm)
            d_hi, d_lo = dev(hi), dev(lo) if lo is not None else None
            g = Guarded(batch * heads * dim * 4)
            vithip.op_map_pool(d_hi.ptr, d_lo.ptr if d_lo else None, fm, batch, lead + NP, lead, dim, d_g.ptr, d_b.ptr, EPS, d_q.ptr, heads, g.ptr)
            got = g.read(np.float32, (batch, heads, dim))                                 # (the canaries are checked here)
            g.free()
            z64, _ = HF.map_z64(xr.reshape(x.shape), gamma, beta, qk, lead)
            assert np.isfinite(got).all(), (dim, heads, NP, lead, batch, order, form)
            e = float(np.abs(got - z64).max() / np.abs(z64).max())
            worst[order] = max(worst.get(order, 0.0), e)
            assert e <= MAP_BOUND[order], (dim, heads, NP, lead, batch, order, form, e)
        for b in _KEEP:
            b.free()
        del _KEEP[:]
    print(f"\n[siglip] map_pool dim {dim}: " + ", ".join(f"{k} {v:.3e} (bound {MAP_BOUND[k]:g})" for k, v in sorted(worst.items())))


# ---- 3. parity with the transformers fixtures -----------------------------------------------------------------------------------
def _fixture(path):
    z, cfg, wseed, iseed, batch, flags, classifier, eps = load_fixture(path)
    blob, _ = fixture_blob(cfg, wseed, classifier, eps)
    return z, cfg, flags, blob, S.make_images(cfg, iseed, batch), eps


@pytest.mark.parametrize("lnf", [0, vithip.FLAG_LN_FOLD_OFF], ids=["default", "fold_off"])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p).split("_s")[0] for p in GOLDEN])
def test_fixture_outputs(path, dt, lnf):
    z, cfg, flags, blob, images, eps = _fixture(path)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags | lnf, ln_eps=eps)
    ctx.load_weights(blob)
    got, fold = ctx.forward(images), ctx.ln_fold()
    ctx.close()
    e = rel(got, z["output"])
    print(f"\n[siglip] {os.path.basename(path).split('_s')[0]} {NAME[dt]} (fold {fold}): output {e:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and e <= MODEL_TOL[dt], e
    assert fold == (cfg["dim"] % 256 == 0 and not lnf)


@pytest.mark.parametrize("lnf", [0, vithip.FLAG_LN_FOLD_OFF], ids=["default", "fold_off"])
@pytest.mark.parametrize("path", [p for p in GOLDEN if "_a_" in os.path.basename(p)], ids=lambda p: os.path.basename(p).split("_s")[0])
def test_fp8_forwards_track_the_emulation(path, lnf):
    z, cfg, flags, blob, images, eps = _fixture(path)
    ref32 = z["output"].astype(np.float32)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    ctx = vithip.VitContext(cfg, dtype=FP8, max_batch=len(images), flags=flags | lnf, ln_eps=eps)
    ctx.load_weights(blob)
    got, folded = ctx.forward(images), ctx.ln_fold()
    ctx.close()
    emu = R.forward(cfg, blob, images, flags, eps, fp8="folded" if folded else "plain")
    r_emu32, r_gpu32, r_gpuemu = rms(emu, ref32), rms(got, ref32), rms(got, emu)
    print(f"\n[siglip fp8] {os.path.basename(path).split('_s')[0]} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
    assert np.isfinite(got).all()
    assert r_gpu32 <= 1.5 * r_emu32 + 1e-3 and r_gpuemu <= 1.5 * r_emu32 + 1e-3


# ---- 4. the head's stages -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [TANH, 0, vithip.FLAG_QUICK_GELU], ids=["tanh", "erf", "quick"])
@pytest.mark.parametrize("cfg,dt", [(A, BF16), (A, FP8), (B, FP16)], ids=["a_bf16", "a_fp8", "b_fp16"])
def test_head_stages(cfg, dt, act):
    """Tap 1 (u) against the float64 head of the context's OWN final rows (debug tap 0): the bound is 4 x the error of the float32
    statement hf_state_dicts.map_head32 on those rows, as for the kernel.  The logits are the fp32 head of tap 1, bit for bit."""
    flags, batch, D, H = NO_CLS | MAP | act, 3, cfg["dim"], cfg["heads"]
    ctx = context(cfg, dt, flags)
    logits = ctx.forward(S.make_images(cfg, 7, batch))
    _, T, _, _ = ctx.features_dims()
    x = ctx.debug_read(0, batch * T * D).reshape(batch, T, D)
    u = ctx.debug_read(1, batch * D).reshape(batch, D)
    ctx.close()
    t = R.unpack_blob(cfg, R.make_blob(cfg, 5, flags, EPS), flags)
    t64 = {k: v.astype(np.float64) for k, v in t.items()}
    y64 = R.layernorm(x.astype(np.float64), t64["lnf.weight"], t64["lnf.bias"], EPS)
    u64 = R.map_head(y64, t64, H, R.activation(flags), EPS)
    e32 = rel(HF.map_head32(x, t, H, flags, EPS), u64)
    e = rel(u, u64)
    print(f"\n[siglip] head stages {NAME[dt]} dim {D}: tap 1 vs float64 {e:.3e}; the float32 statement {e32:.3e} (bound 4 x)")
    assert np.isfinite(u).all() and e <= 4.0 * e32, (e, e32)
    head = dev(np.zeros((batch, cfg["classes"]), np.float32))
    vithip.op_head_f32(dev(u).ptr, dev(t["head.weight"]).ptr, dev(t["head.bias"]).ptr, head.ptr, batch, cfg["classes"], D)
    assert same_bits(head.to_numpy(np.float32, (batch, cfg["classes"])), logits)


# ---- 5. the same logit bits on every route into a forward -------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dt", [(A, BF16), (A, FP8), (B, FP16)], ids=["a_bf16", "a_fp8", "b_fp16"])
def test_same_logit_bits_alone_in_a_batch_across_streams_and_graph_replay(cfg, dt):
    images = S.make_images(cfg, 8, 5)
    ctx = context(cfg, dt, MAPF)
    five = ctx.forward(images)
    assert np.isfinite(five).all()
    one = context(cfg, dt, MAPF, max_batch=1)
    assert same_bits(one.forward(images[2:3]), five[2:3])                             # image 2 alone at max_batch 1
    one.close()
    assert same_bits(ctx.forward(images[1:4]), five[1:4])
    ctx.set_streams(2)
    assert same_bits(ctx.forward(images), five)
    D = cfg["dim"]
    tap = ctx.debug_read(1, 5 * D)                                                    # the parts wrote their own slices of the head's input
    ctx.set_streams(1)
    ctx.forward(images)
    assert same_bits(ctx.debug_read(1, 5 * D), tap)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert same_bits(ctx.forward(images), five)
    ctx.set_streams(2)
    for _ in range(3):
        assert same_bits(ctx.forward(images), five)
    ctx.set_graph(False)
    ctx.close()


def test_same_logit_bits_through_the_u8_ring():
    u8 = make_u8_images(5, A["image_size"], 3, seed=3)
    ctx = context(A, BF16, MAPF)
    want = ctx.forward(u8_reference(u8, np.full(3, DEFAULT_SCALE), np.zeros(3, np.float32)))
    assert np.isfinite(want).all() and same_bits(ctx.forward_u8(u8), want)
    ctx.ring_create_u8(2, 5)
    try:
        ctx.ring_submit_u8(u8)
        ctx.ring_submit_u8(u8[:2])
        assert same_bits(ctx.ring_collect(), want) and same_bits(ctx.ring_collect(), want[:2])
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)
    ctx.close()


# ---- 6. a blob of another model is refused ----------------------------------------------------------------------------------------
def _forge(blob, flags_bits):
    out = blob.copy()
    bits = int(out[52:56].view(np.uint32)[0])
    out[52:56] = np.array([(bits & 1) | flags_bits], np.uint32).view(np.uint8)       # (bit 0: a file's checksum mark stays)
    return out


def _header_bits(flags):
    return int(R.blob_header(B, flags)[52:56].view(np.uint32)[0])


@pytest.mark.parametrize("flags", [NO_CLS | POOL(vithip.POOL_AVG_NORM) | TANH, MAPF], ids=["tanh", "map_tanh"])
def test_a_blob_with_other_siglip_bits_is_refused(flags, tmp_path):
    """A tanh blob and an erf blob are identical in size: only the header tells them apart.  A same-size blob or file whose bit 19 or
    21 differs from the context's is refused with the bit's own message, and the refused loads change nothing."""
    cfg = B
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags, ln_eps=EPS)
    ctx.init_weights_seeded(17)
    blob = ctx.export_weights()
    assert np.array_equal(blob, R.make_blob(cfg, 17, flags, EPS))                   # the seeded map.* tensors have their ids; the bits in the header
    path, bad = str(tmp_path / "m.vhblob"), str(tmp_path / "forged.vhblob")
    ctx.save_weights_file(path)
    assert vithip.blob_file_flags(path) == flags
    images = S.make_images(cfg, 2, 2)
    want = ctx.forward(images)
    ctx.load_weights_file(path)
    assert same_bits(ctx.forward(images), want)
    file_bytes = np.fromfile(path, np.uint8)
    forged = [(flags ^ TANH, rf"header bit 21 \(tanh GELU\) is {0 if flags & TANH else 1}, the context's VH_FLAG_TANH_GELU is {1 if flags & TANH else 0}")]
    if flags & MAP:   # the same size with bit 19 cleared (a legal word needs a pool mode then: bits 16 .. 17 speak first) and with both cleared
        forged.append(((flags ^ MAP) | POOL(vithip.POOL_AVG_NORM), "pooling mode 1, the context's VH_FLAG_POOL says 0"))
        forged.append((flags ^ MAP, r"header bit 19 \(attention-pooling head\) is 0, the context's VH_FLAG_MAP_HEAD is 1"))
    for f, msg in forged:
        with pytest.raises(vithip.VhError, match=msg) as e:
            ctx.load_weights(_forge(blob, _header_bits(f)))
        assert e.value.code == 1
        if R.legal(cfg, f):                                                          # (a file's header must describe a legal model to get that far)
            _forge(file_bytes, _header_bits(f)).tofile(bad)
            with pytest.raises(vithip.VhError):
                ctx.load_weights_file(bad)
    assert same_bits(ctx.forward(images), want)                                       # the refused loads changed nothing
    ctx.close()
    other = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags ^ TANH, ln_eps=EPS)   # and the other way round
    with pytest.raises(vithip.VhError, match="tanh GELU"):
        other.load_weights(blob)
    with pytest.raises(vithip.VhError, match="tanh GELU"):
        other.load_weights_file(path)
    other.load_weights(_forge(blob, _header_bits(flags ^ TANH)))                      # its own bits: the same tensors load
    assert not same_bits(other.forward(images), want)                                 # and it is another function
    other.close()


# ---- 7. features on the new contexts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dt", [(A, BF16), (A, FP8), (B, BF16)], ids=["a_bf16", "a_fp8", "b_bf16"])
def test_features_equal_the_no_class_token_behaviour(cfg, dt):
    """patch / mean of a MAP context are those of the NO_CLS | POOL(AVG_NORM) context with the same backbone, bit for bit (the head does
    not touch the rows), and obey the same statements: raw = tap 0, normalised within NORM_BOUND of float64, mean = the fp32 chain."""
    batch, D = 3, cfg["dim"]
    images = S.make_images(cfg, 7, batch)
    t = R.make_tensors(cfg, 5, MAPF)
    base_flags = NO_CLS | POOL(vithip.POOL_AVG_NORM) | TANH
    ctx = context(cfg, dt, MAPF)
    ctx.forward(images)
    base = vithip.VitContext(cfg, dtype=dt, max_batch=5, flags=base_flags, ln_eps=EPS)
    base.load_weights(R.pack_blob(cfg, t, base_flags, EPS))
    base.forward(images)
    _, T, NP, _ = ctx.features_dims()
    assert T == NP
    x = ctx.debug_read(0, batch * T * D).reshape(batch, T, D)
    for norm in (RAW, NORM):
        got = ctx.read_features(cls=False, patch=True, mean=True, elem=F32, norm=norm)
        want = base.read_features(cls=False, patch=True, mean=True, elem=F32, norm=norm)
        assert same_bits(got["patch"], want["patch"]) and same_bits(got["mean"], want["mean"])
        assert same_bits(got["mean"], FR.mean_chain(got["patch"]))
    assert same_bits(ctx.read_features(cls=False, patch=True, elem=F32, norm=RAW)["patch"], x)
    ref = FR.layernorm64(x, t["lnf.weight"], t["lnf.bias"], EPS)
    assert float(np.abs(got["patch"] - ref).max()) <= FR.NORM_BOUND * float(np.abs(ref).max())
    assert same_bits(got["mean"], base.debug_read(1, batch * D).reshape(batch, D))       # the base context's head input; this one's is u
    with pytest.raises(vithip.VhError, match="without a class token"):
        ctx.read_features(cls=True, patch=False)
    ctx.close()
    base.close()
