"""GPU suite of the register tokens (include/vithip.h, VH_FLAG_REGISTERS): the token assembly bit for bit -- through a context
after zero layers (the fp32 rows of every path) and through the two taps for the split planes and their row statistics --, whole
models against the Hugging Face fixtures and tests/vit_ref.py on every LayerNorm path, the token features shifted by R, the
other routes into a forward (batch split, streams, graph replay, 8-bit ring, tensors, torch), the class-token tail, the
pre-LayerNorm, a real DINOv2-S/14-reg shape and the refusals.  Tolerances are the project's own: test_gpu_vit's model bounds
(fp16 1e-3, bf16 1e-2) and test_gpu_fp8's `1.5 x emulation + 1e-3`; everything else is equality of bits."""
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import features_ref as FR
import hf_state_dicts as H
import vh_synth as S
import vit_ref as R
from tensor_ref import make_u8_images, u8_reference
from test_u8_input import DEFAULT_SCALE
from vh_testlib import _KEEP, _release_buffers, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
PRE, REG = vithip.FLAG_PRE_LN, vithip.FLAG_REGISTERS
LN_PATHS = [(0, "default"), (vithip.FLAG_LN_FOLD_ON, "fold_on"), (vithip.FLAG_LN_FOLD_OFF, "fold_off")]
F32, F16, B16 = vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "reg", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-6


def _cfg(image, patch, dim, heads, mlp, layers, classes=40):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


# 16 patches per image: batch 20 gives 320 patch-GEMM rows = two row tiles with a ragged second, wave tiles spanning four images
D128 = _cfg(32, 8, 128, 2, 256, 2)           # the fp32 residual (EPI_PATCH) whatever the flags say
D256 = _cfg(32, 8, 256, 4, 512, 2)           # dims multiples of 256: fold + split residual (EPI_PATCH_SPLIT), head dim 64
MODELS = {"d128": D128, "d256": D256}
DINO_S14_REG = _cfg(224, 14, 384, 6, 1536, 12, classes=1000)   # 256 patches + class token + 4 registers = 261 tokens


def dev(a):
    b = vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    _KEEP.append(b)
    return b


def bits(a):
    return FR.bits(a)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def blobs(cfg, regs, seed=5, flags=0):
    """The seeded tensors with R register rows, their blob, and the blob of the R = 0 model that holds the same tensors."""
    t = R.make_tensors(cfg, seed, REG(regs) | flags)
    return t, R.pack_blob(cfg, t, REG(regs) | flags), R.pack_blob(cfg, t, flags)


def context(cfg, dt, batch, blob, flags=0, eps=EPS):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch, flags=flags, ln_eps=eps)
    ctx.load_weights(blob)
    return ctx


def hidden(ctx, batch):
    _, T, _, D = ctx.features_dims()
    return ctx.debug_read(0, batch * T * D).reshape(batch, T, D)


# ---- 1. the embedded rows, exact ------------------------------------------------------------------------------------------------
_ROWS0 = {}


def _rows_without_registers(model, dt, batch, blob0, images):
    key = (model, dt, batch)
    if key not in _ROWS0:
        ctx = context(MODELS[model], dt, batch, blob0)
        ctx.debug_set_layers(0)
        ctx.forward(images)
        _ROWS0[key] = hidden(ctx, batch)
        ctx.close()
    return _ROWS0[key]


@pytest.mark.parametrize("batch", [3, 20])
@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: NAME[d])
@pytest.mark.parametrize("model", ["d128", "d256"])
@pytest.mark.parametrize("regs", [1, 4, 16])
def test_embedded_rows_are_the_rows_without_registers_and_the_register_tensor(regs, model, dt, batch):
    cfg = MODELS[model]
    t, blob, blob0 = blobs(cfg, regs)
    images = S.make_images(cfg, 6, batch)
    want = _rows_without_registers(model, dt, batch, blob0, images)
    ctx = context(cfg, dt, batch, blob, REG(regs))
    assert ctx.register_tokens() == regs
    ctx.debug_set_layers(0)
    ctx.forward(images)
    NP = S.tokens(cfg) - 1
    assert ctx.features_dims() == (batch, NP + 1 + regs, NP, cfg["dim"])
    x = hidden(ctx, batch)
    ctx.close()
    assert np.isfinite(x).all()
    assert same_bits(x[:, 0], want[:, 0])                                            # cls + pos[0]
    assert same_bits(x[:, 1 + regs:], want[:, 1:])                                    # patch p: the bits of row 1 + p without registers
    assert same_bits(x[:, 1:1 + regs], np.broadcast_to(t["reg"], (batch, regs, cfg["dim"])).copy())   # reg[r], no position row


def _assembly_operands(batch, regs, dt, D=256, NP=16, K=192, seed=31):
    a = vithip.to16(S.fill(batch * NP * K, seed, 1, 0).reshape(batch * NP, K), dt)
    w = vithip.to16(S.fill(D * K, seed, 2, 1, 0.05).reshape(D, K), dt)
    bias, pos = S.fill(D, seed, 3, 1, 0.1), S.fill((NP + 1) * D, seed, 4, 1, 0.3).reshape(NP + 1, D)
    cls, reg = S.fill(D, seed, 5, 1, 0.5), (S.fill(regs * D, seed, 6, 1, 0.7) + 0.25).reshape(regs, D)
    return a, w, bias, pos, cls, reg


def _split_embed(batch, lead, dt, a, w, bias, pos, cls, reg, D=256, NP=16, pad_rows=5):
    """PATCH_SPLIT GEMM + lead-row kernel through the taps -> (hi bits [B, T, D], lo bytes [B, T, D], partials [D/64, prow, 2])."""
    T, K = NP + lead, a.shape[1]
    prow = batch * T + pad_rows
    hi, lo = dev(np.full((batch * T, D), 0x7B7B, np.uint16)), dev(np.full((batch * T, D), 0x7B, np.uint8))
    part = dev(np.full((D // 64, prow, 2), -777.0, np.float32))
    vithip.op_gemm_lead(dev(a).ptr, dev(w).ptr, dev(bias).ptr, hi.ptr, batch * NP, D, K, vithip.EPI_PATCH_SPLIT, dt, dev(pos).ptr, NP, lead,
                        out16_ptr=lo.ptr, partials_ptr=part.ptr, prow=prow)
    after_gemm = hi.to_numpy(np.uint16, (batch, T, D))
    assert (after_gemm[:, :lead] == 0x7B7B).all() and not (after_gemm[:, lead:] == 0x7B7B).all(-1).any()   # the patch rows and only those
    vithip.op_lead_rows(hi.ptr, dev(cls).ptr, dev(pos).ptr, dev(reg).ptr if lead > 1 else None, lead, batch, T, D, lo_ptr=lo.ptr,
                        partials_ptr=part.ptr, prow=prow, dtype=dt)
    p = part.to_numpy(np.float32, (D // 64, prow, 2))
    assert (p[:, batch * T:] == -777.0).all() and not (p[:, :batch * T] == -777.0).any()   # every real row once, no padding row
    return hi.to_numpy(np.uint16, (batch, T, D)), lo.to_numpy(np.uint8, (batch, T, D)), p, part, prow


@pytest.mark.parametrize("batch", [3, 20])
@pytest.mark.parametrize("dt", [BF16, FP16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("regs", [1, 4, 16])
def test_split_planes_and_row_statistics_of_the_assembly(regs, dt, batch):
    D, NP, lead = 256, 16, 1 + regs
    a, w, bias, pos, cls, reg = _assembly_operands(batch, regs, dt)
    hi, lo, p, part, prow = _split_embed(batch, lead, dt, a, w, bias, pos, cls, reg)
    hi0, lo0, p0, _, _ = _split_embed(batch, 1, dt, a, w, bias, pos, cls, None)
    T, T0 = NP + lead, NP + 1
    pr = lambda q, B, Tq: q[:, :B * Tq].reshape(D // 64, B, Tq, 2)
    # class row and patch rows: the bytes of the R = 0 assembly, planes and partial sums
    assert np.array_equal(hi[:, 0], hi0[:, 0]) and np.array_equal(lo[:, 0], lo0[:, 0])
    assert np.array_equal(hi[:, lead:], hi0[:, 1:]) and np.array_equal(lo[:, lead:], lo0[:, 1:])
    assert same_bits(pr(p, batch, T)[:, :, 0], pr(p0, batch, T0)[:, :, 0]) and same_bits(pr(p, batch, T)[:, :, lead:], pr(p0, batch, T0)[:, :, 1:])
    # register rows: what the kernel writes for a class row holding those numbers (cls = reg[r], pos[0] = 0), i.e. hi = T(x),
    # lo = lo8(x - hi) as the header defines them, and the fixed-order sums of x and x^2 per 64 columns
    zero = np.zeros_like(pos)
    for r in range(regs):
        h1, l1 = dev(np.zeros((batch * T0, D), np.uint16)), dev(np.zeros((batch * T0, D), np.uint8))
        p1 = dev(np.zeros((D // 64, batch * T0, 2), np.float32))
        vithip.op_lead_rows(h1.ptr, dev(reg[r]).ptr, dev(zero).ptr, None, 1, batch, T0, D, lo_ptr=l1.ptr, partials_ptr=p1.ptr,
                            prow=batch * T0, dtype=dt)
        assert np.array_equal(hi[:, 1 + r], h1.to_numpy(np.uint16, (batch, T0, D))[:, 0])
        assert np.array_equal(lo[:, 1 + r], l1.to_numpy(np.uint8, (batch, T0, D))[:, 0])
        assert same_bits(pr(p, batch, T)[:, :, 1 + r], p1.to_numpy(np.float32, (D // 64, batch, T0, 2))[:, :, 0])
        hv = vithip.to16(reg[r], dt)
        assert np.array_equal(hi[0, 1 + r], hv) and np.array_equal(lo[0, 1 + r], vithip.to_lo8(reg[r] - vithip.from16(hv, dt), dt))
    # the first LayerNorm statistics over ALL T rows of every image, from those partial sums
    st = dev(np.zeros((prow, 2), np.float32))
    vithip.op_finalize_stats(part.ptr, D // 64, prow, D, EPS, st.ptr)
    stats = st.to_numpy(np.float32, (prow, 2))[:batch * T].reshape(batch, T, 2)
    a64, w64 = vithip.from16(a, dt).astype(np.float64), vithip.from16(w, dt).astype(np.float64)
    x = R.assemble((a64 @ w64.T + bias).reshape(batch, NP, D), cls.astype(np.float64), pos.astype(np.float64), reg.astype(np.float64))
    x[:, 0] = (cls + pos[0]).astype(np.float64)                                      # (the fp32 sum the kernel forms)
    assert np.isfinite(stats).all()
    assert np.allclose(stats[..., 0], x.mean(-1), atol=1e-5) and np.allclose(stats[..., 1], 1.0 / np.sqrt(x.var(-1) + EPS), rtol=1e-5)


@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: NAME[d])
def test_guards_are_finite_on_the_folded_path(dt):
    _, blob, _ = blobs(D256, 4)
    ctx = context(D256, dt, 20, blob, REG(4) | vithip.FLAG_LN_FOLD_ON)
    got = ctx.forward(S.make_images(D256, 6, 20))
    ratio, thresh, tripped = ctx.ln_guard()
    ctx.close()
    assert np.isfinite(got).all() and np.isfinite(ratio) and 0 < ratio < thresh and not tripped


# ---- 2. model parity --------------------------------------------------------------------------------------------------------------
def load_fixture(path):
    z = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in z["config"])))
    wseed, iseed, batch, regs = (int(v) for v in z["meta"])
    t = R.make_tensors(cfg, wseed, REG(regs))
    sd = H.dinov2_state_dict(cfg, t, wseed)
    mcfg = dict(cfg, registers=regs)
    blob = vithip.blob_from_dinov2_state_dict(sd, mcfg, float(z["ln_eps"]), head=(t["head.weight"], t["head.bias"]))
    return z, cfg, mcfg, regs, blob, S.make_images(cfg, iseed, batch), float(z["ln_eps"])


_FIX = {}


def fixture(path):
    if path not in _FIX:
        z, cfg, mcfg, regs, blob, images, eps = load_fixture(path)
        logits = R.forward(cfg, blob, images, REG(regs), eps, np.float64)
        _FIX[path] = (z, cfg, mcfg, regs, blob, images, eps, logits)
    return _FIX[path]


def test_fixtures_are_present():
    assert len(GOLDEN) == 2, GOLDEN


@pytest.mark.parametrize("lnf,label", LN_PATHS, ids=[p[1] for p in LN_PATHS])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:9] for p in GOLDEN])
def test_fixture_features_and_logits_on_every_layernorm_path(path, dt, lnf, label):
    z, cfg, mcfg, regs, blob, images, eps, ref_logits = fixture(path)
    ctx = context(mcfg, dt, len(images), blob, lnf, eps)      # the count from the model dict
    assert ctx.register_tokens() == regs
    got = ctx.forward(images)
    fold = ctx.ln_fold()
    f = ctx.read_features(cls=True, patch=True, mean=False, norm=vithip.FEAT_NORM)
    ctx.close()
    last = z["last_hidden_state"]
    e_l, e_c, e_p = rel(got, ref_logits), rel(f["cls"], last[:, 0]), rel(f["patch"], last[:, 1 + regs:])
    print(f"\n[reg] {os.path.basename(path)[:9]} {NAME[dt]} {label} (fold {fold}): logits {e_l:.3e} cls {e_c:.3e} patch {e_p:.3e}")
    assert np.isfinite(got).all() and np.isfinite(f["patch"]).all()
    assert e_l <= MODEL_TOL[dt] and e_c <= MODEL_TOL[dt] and e_p <= MODEL_TOL[dt], (e_l, e_c, e_p)
    if cfg["dim"] % 256 == 0 and lnf != vithip.FLAG_LN_FOLD_OFF:
        assert fold


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:9] for p in GOLDEN])
def test_fp8_forwards_track_the_emulation(path):
    z, cfg, mcfg, regs, blob, images, eps, ref64 = fixture(path)
    ref32 = ref64.astype(np.float32)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    emu = {}
    for lnf, label in LN_PATHS:
        ctx = context(mcfg, FP8, len(images), blob, lnf, eps)
        got, folded = ctx.forward(images), ctx.ln_fold()
        ctx.close()
        if folded not in emu:
            emu[folded] = R.forward(cfg, blob, images, REG(regs), eps, fp8="folded" if folded else "plain")
        r_emu32, r_gpu32, r_gpuemu = rms(emu[folded], ref32), rms(got, ref32), rms(got, emu[folded])
        print(f"\n[reg fp8] {os.path.basename(path)[:9]} {label} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
        assert np.isfinite(got).all()
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3, label
        assert r_gpuemu <= 1.5 * r_emu32 + 1e-3, label


# ---- 3. token features, shifted by R ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dt,regs", [("d256", BF16, 4), ("d256", FP8, 1), ("d128", FP16, 16)],
                         ids=["d256_bf16_r4", "d256_fp8_r1", "d128_fp16_r16"])
def test_features_skip_the_register_rows(model, dt, regs):
    cfg = MODELS[model]
    _, blob, _ = blobs(cfg, regs)
    ctx = context(cfg, dt, 3, blob, REG(regs))
    ctx.forward(S.make_images(cfg, 7, 3))
    x = hidden(ctx, 3)
    raw = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=vithip.FEAT_RAW)
    assert same_bits(raw["cls"], x[:, 0]) and same_bits(raw["patch"], x[:, 1 + regs:])       # the debug tap's rows 1 + R ..
    assert raw["patch"].shape == (3, S.tokens(cfg) - 1, cfg["dim"])
    assert same_bits(raw["mean"], FR.mean_chain(raw["patch"]))                               # the serial chain over exactly NP rows
    nrm = ctx.read_features(cls=True, patch=True, mean=True, elem=F32, norm=vithip.FEAT_NORM)
    assert same_bits(nrm["cls"], ctx.debug_read(1, 3 * cfg["dim"]).reshape(3, cfg["dim"]))
    assert same_bits(nrm["mean"], FR.mean_chain(nrm["patch"]))
    t = R.unpack_blob(cfg, blob, REG(regs))
    ref = FR.layernorm64(x[:, 1 + regs:], t["lnf.weight"], t["lnf.bias"], EPS)
    assert float(np.abs(nrm["patch"] - ref).max()) <= FR.NORM_BOUND * float(np.abs(ref).max())
    for norm, f32 in ((vithip.FEAT_RAW, raw), (vithip.FEAT_NORM, nrm)):
        for elem in (F16, B16):
            f16 = ctx.read_features(cls=True, patch=True, mean=True, elem=elem, norm=norm)
            for k in ("cls", "patch", "mean"):
                assert np.array_equal(bits(f16[k]), FR.rne16(f32[k], elem)), (k, elem, norm)
    ctx.close()


# ---- 4. the other routes into a forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, FP16], ids=lambda d: NAME[d])
def test_same_logit_bits_across_batch_split_streams_and_graph_replay(dt):
    cfg, regs = D256, 4
    _, blob, _ = blobs(cfg, regs)
    images = S.make_images(cfg, 8, 7)
    ctx = context(cfg, dt, 7, blob, REG(regs))
    seven = ctx.forward(images)
    assert np.isfinite(seven).all()
    assert same_bits(ctx.forward(images[:1]), seven[:1]) and same_bits(ctx.forward(images[2:5]), seven[2:5])
    ctx.set_streams(4)
    assert same_bits(ctx.forward(images), seven)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert same_bits(ctx.forward(images), seven)
    ctx.set_streams(4)
    for _ in range(3):
        assert same_bits(ctx.forward(images), seven)
    ctx.set_graph(False)
    ctx.close()


@pytest.mark.parametrize("model", ["d128", "d256"])
def test_same_logit_bits_through_the_u8_ring_and_an_nchw_tensor(model):
    cfg, regs = MODELS[model], 4
    _, blob, _ = blobs(cfg, regs)
    u8 = make_u8_images(5, cfg["image_size"], 3, seed=3)
    ctx = context(cfg, BF16, 5, blob, REG(regs))
    want = ctx.forward(u8_reference(u8, np.full(3, DEFAULT_SCALE), np.zeros(3, np.float32)))
    assert np.isfinite(want).all()
    assert same_bits(ctx.forward_u8(u8), want)
    assert same_bits(ctx.forward_tensor(np.ascontiguousarray(u8.transpose(0, 3, 1, 2)), vithip.LAYOUT_NCHW), want)
    nchw16 = np.ascontiguousarray(u8.transpose(0, 3, 1, 2)).astype(np.float16)
    assert same_bits(ctx.forward_tensor(nchw16, vithip.LAYOUT_NCHW), ctx.forward(nchw16.transpose(0, 2, 3, 1).astype(np.float32)))
    ctx.ring_create_u8(2, 5)
    try:
        ctx.ring_submit_u8(u8)
        ctx.ring_submit_u8(u8[:2])
        assert same_bits(ctx.ring_collect(), want) and same_bits(ctx.ring_collect(), want[:2])
    finally:
        vithip.lib().vh_ring_destroy(ctx.h)
    ctx.close()


TORCH_SCRIPT = r"""
import torch                      # before libvithip.so is loaded: one HIP runtime in the process (INTEGRATION.md)
import numpy as np
import vh_synth as S, vit_ref as R, vithip
cfg = dict(image_size=32, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=40, registers=4)
ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_FP16, max_batch=3)
ctx.load_weights(R.make_blob(cfg, 5, R.FLAG_REGISTERS(4)))
assert ctx.register_tokens() == 4
images = S.make_images(cfg, 9, 3)
want = ctx.forward(images)
x = torch.from_numpy(np.ascontiguousarray(images.transpose(0, 3, 1, 2)))
for t in (x, x.to(torch.device("cuda", 0))):
    got = ctx.forward_torch(t)
    assert got.device.type == t.device.type and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
print("forward_torch with registers ok")
"""


def test_forward_torch_with_an_nchw_tensor():
    """In a process of its own, as tests/test_gpu_tensor_input.py does and for its reason: torch brings a HIP runtime of its own
    and has to be imported before libvithip.so is loaded."""
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    root = os.path.dirname(HERE)
    path = os.pathsep.join([HERE, os.path.join(root, "vit-fpga_amd", "python")])
    env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", TORCH_SCRIPT], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "forward_torch with registers ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("dt", [BF16, FP16], ids=lambda d: NAME[d])
def test_class_token_tail_with_registers_agrees_to_the_model_bound(dt):
    cfg, regs = D256, 4          # head dim 64
    _, blob, _ = blobs(cfg, regs)
    images = S.make_images(cfg, 8, 7)
    ref = R.forward(cfg, blob, images, REG(regs)).astype(np.float32)
    outs = []
    for extra in (0, vithip.FLAG_CLS_TAIL):
        ctx = context(cfg, dt, 7, blob, REG(regs) | vithip.FLAG_LN_FOLD_ON | extra)
        outs.append(ctx.forward(images))
        ctx.close()
    base, tail = outs
    print(f"\n[reg] class-token tail {NAME[dt]}: tail vs full {rel(tail, base):.3e}, tail vs vit_ref {rel(tail, ref):.3e}")
    assert np.isfinite(tail).all() and not np.array_equal(tail, base)     # (another attention kernel: rounding, not bits)
    assert rel(tail, ref) <= MODEL_TOL[dt] and rel(tail, base) <= MODEL_TOL[dt] and rel(base, ref) <= MODEL_TOL[dt]


@pytest.mark.parametrize("dt", [BF16, FP16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("model", ["d128", "d256"])
def test_pre_layernorm_with_registers_matches_reg_ref(model, dt):
    cfg, regs, flags = MODELS[model], 4, PRE | REG(4)
    blob = R.make_blob(cfg, 5, flags)
    images = S.make_images(cfg, 8, 3)
    _, rows = R.forward(cfg, blob, images, flags, want_hidden=True, n_layers=0)
    ref = R.forward(cfg, blob, images, flags).astype(np.float32)
    for lnf, label in LN_PATHS:
        ctx = context(cfg, dt, 3, blob, flags | lnf)
        got = ctx.forward(images)
        ctx.debug_set_layers(0)
        ctx.forward(images)
        x0 = hidden(ctx, 3).reshape(rows.shape)
        ctx.close()
        print(f"\n[reg] pre-LN {model} {NAME[dt]} {label}: logits {rel(got, ref):.3e}, normalised embedded rows {rel(x0, rows):.3e}")
        assert np.isfinite(got).all() and rel(got, ref) <= MODEL_TOL[dt], label
        assert rel(x0, rows) <= (1e-2 if dt != FP16 else 2e-3)       # test_gpu_clip's bound for the rows after the pre-LayerNorm


# ---- 5. a real shape ------------------------------------------------------------------------------------------------------------------
def test_dinov2_s14_reg_224_fp16_against_reg_ref_fp32():
    cfg, regs, n = DINO_S14_REG, 4, 2
    blob, images = R.make_blob(cfg, 0, REG(regs)), S.make_images(cfg, 1, n)
    ref = R.forward(cfg, blob, images, REG(regs), dtype=np.float32)
    ctx = context(dict(cfg, registers=regs), FP16, n, blob)
    got = ctx.forward(images)
    dims = ctx.features_dims()
    ctx.close()
    per = np.abs(got - ref).max(1) / np.abs(ref).max()
    print(f"\n[reg] DINOv2-S/14-reg 224 fp16 b{n} (261 tokens): per-image {' '.join(f'{x:.2e}' for x in per)}")
    assert dims == (n, 261, 256, 384) and np.isfinite(got).all() and per.max() <= MODEL_TOL[FP16], per


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_blob_with_another_register_count_is_refused(tmp_path):
    cfg = D128
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=REG(4))
    ctx.init_weights_seeded(17)
    blob = ctx.export_weights()
    assert np.array_equal(blob, R.make_blob(cfg, 17, REG(4)))                      # reg from tensor id 7; the count in the header
    path = str(tmp_path / "m.vhblob")
    ctx.save_weights_file(path)
    assert vithip.blob_file_flags(path) == REG(4)
    images = S.make_images(cfg, 2, 2)
    want = ctx.forward(images)
    ctx.load_weights_file(path)
    assert same_bits(ctx.forward(images), want)
    for other in (0, 3, 5):
        with pytest.raises(vithip.VhError):
            ctx.load_weights(R.make_blob(cfg, 17, REG(other)))                     # another size
        forged = blob.copy()                                                       # the right size with another count
        forged[52:56] = np.array([REG(other)], np.uint32).view(np.uint8)
        with pytest.raises(vithip.VhError, match=f"{other} register tokens"):
            ctx.load_weights(forged)
    assert same_bits(ctx.forward(images), want)                                    # the refused loads changed nothing
    ctx.close()
    c0 = vithip.VitContext(cfg, dtype=FP16, max_batch=2)
    with pytest.raises(vithip.VhError):
        c0.load_weights_file(path)
    c0.close()
