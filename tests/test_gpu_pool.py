"""GPU suite of the pooled heads and of models without a class token (include/vithip.h, VH_FLAG_POOL / VH_FLAG_NO_CLS).  The
contract is written for bits, so nearly everything below is equality: the assembly without row 0 against the class-token context of
the same tensors, the head's input (debug tap 1) against the token features of the same forward, the one-pass pool kernel against
the two-kernel mean of vh_op_token_features2, the logits against the fp32 head of tap 1, and the routes into a forward against each
other.  The tolerances are the project's own: test_gpu_vit's model bounds (fp16 1e-3, bf16 1e-2 of max|ref|) against the
transformers fixtures, test_gpu_fp8's `1.5 x emulation + 1e-3`, and features_ref.NORM_BOUND for a normalised row against fp64."""
import glob
import os

import numpy as np
import pytest

import features_ref as FR
import hf_state_dicts as H
import vh_synth as S
import vit_ref as R
from test_gpu_features import Guarded
from tensor_ref import make_u8_images, u8_reference
from test_u8_input import DEFAULT_SCALE
from vh_testlib import _KEEP, _release_buffers, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
REG, NO_CLS, POOL = vithip.FLAG_REGISTERS, vithip.FLAG_NO_CLS, vithip.FLAG_POOL
CLS, AVG_NORM, AVG_FCNORM, CLS_AVG = vithip.POOL_CLS, vithip.POOL_AVG_NORM, vithip.POOL_AVG_FCNORM, vithip.POOL_CLS_AVG
F32 = vithip.ELEM_F32
NORM, RAW = vithip.FEAT_NORM, vithip.FEAT_RAW
VH_ERR_UNSUPPORTED = 4
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "pool", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
EPS = 1e-6
BATCHES, MAX_BATCH = (1, 3, 5), 5

# NP 25: ragged against 4-row workgroups, 16-row tiles and any rows-per-group; dims multiples of 256: fold + split residual, fp8-eligible
A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=8)
B = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=8)   # NP 16, the fp32 residual path
Cc = dict(image_size=16, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=8)  # NP 4: T = 4 under NO_CLS
# name: (config, dtype, LayerNorm flag, does the residual live as planes)
PATHS = {"a_bf16": (A, BF16, 0, True), "a_fp16": (A, FP16, 0, True), "a_fp8": (A, FP8, 0, True),
         "a_fold_off": (A, BF16, vithip.FLAG_LN_FOLD_OFF, False), "b_bf16": (B, BF16, 0, False)}
MODES = {"avg_norm": POOL(AVG_NORM), "avg_fcnorm": POOL(AVG_FCNORM), "cls_avg": POOL(CLS_AVG),
         "nocls_avg_norm_r4": NO_CLS | POOL(AVG_NORM) | REG(4), "nocls_avg_fcnorm": NO_CLS | POOL(AVG_FCNORM)}


def dev(a):
    b = vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    _KEEP.append(b)
    return b


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(FR.bits(a), FR.bits(b))


def tensors_for(cfg, flags, seed=5):
    """The seeded tensors of the class-token model with this register count, reshaped for `flags`: without `cls` and pos[0] under
    NO_CLS, with a [C][2 D] head under CLS_AVG -- so that contexts of different flags hold the SAME model otherwise."""
    t = R.make_tensors(cfg, seed, flags & R.FLAG_REGISTERS_MASK)
    if R.pool_of(flags) == CLS_AVG:
        t["head.weight"] = R.make_tensors(cfg, seed, POOL(CLS_AVG))["head.weight"]
    return R.without_cls(t) if flags & NO_CLS else t


def context(cfg, dt, flags, max_batch=MAX_BATCH, seed=5, extra=0):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=max_batch, flags=flags | extra, ln_eps=EPS)
    ctx.load_weights(R.pack_blob(cfg, tensors_for(cfg, flags, seed), flags, EPS))
    return ctx


def hidden(ctx, batch):
    _, T, _, D = ctx.features_dims()
    return ctx.debug_read(0, batch * T * D).reshape(batch, T, D)


# ---- 1. the assembly without row 0 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regs", [0, 4])
@pytest.mark.parametrize("model,dt", [("a", BF16), ("a", FP8), ("b", FP16), ("c", BF16)], ids=["a_bf16", "a_fp8", "b_fp16", "c_bf16"])
def test_embedded_rows_are_the_class_token_contexts_patch_rows_and_the_register_tensor(model, dt, regs):
    cfg = {"a": A, "b": B, "c": Cc}[model]
    NP, D = S.tokens(cfg) - 1, cfg["dim"]
    with_cls, without = context(cfg, dt, REG(regs)), context(cfg, dt, NO_CLS | POOL(AVG_NORM) | REG(regs))
    reg = tensors_for(cfg, REG(regs)).get("reg")
    for c in (with_cls, without):
        c.debug_set_layers(0)
    for batch in BATCHES:
        images = S.make_images(cfg, 6, batch)
        with_cls.forward(images)
        got = without.forward(images)
        assert np.isfinite(got).all()
        assert without.features_dims() == (batch, NP + regs, NP, D)
        want, x = hidden(with_cls, batch), hidden(without, batch)
        assert same_bits(x[:, regs:], want[:, 1 + regs:]), batch                    # patch p + pos[p]: the bits of the class-token model
        if regs:
            assert same_bits(x[:, :regs], np.broadcast_to(reg, (batch, regs, D)).copy())     # reg[r], no position row
    with_cls.close()
    without.close()


@pytest.mark.parametrize("batch", [3, 5])
@pytest.mark.parametrize("dt", [BF16, FP16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("regs", [0, 4])
def test_split_planes_and_row_statistics_without_row_0(regs, dt, batch):
    """The split path through the taps, as tests/test_gpu_registers.py checks the register assembly: the PATCH_SPLIT epilogue with
    lead = R (0 included) given the position table one row early -- here simply the class-token model's [NP + 1][D] table -- and the
    all-register form of the lead-row kernel write the planes and partial sums of the class-token assembly's rows 1 .. ."""
    D, NP, K, seed = 256, 25, 192, 31
    a = vithip.to16(S.fill(batch * NP * K, seed, 1, 0).reshape(batch * NP, K), dt)
    w = vithip.to16(S.fill(D * K, seed, 2, 1, 0.05).reshape(D, K), dt)
    bias, pos = S.fill(D, seed, 3, 1, 0.1), S.fill((NP + 1) * D, seed, 4, 1, 0.3).reshape(NP + 1, D)
    cls, reg = S.fill(D, seed, 5, 1, 0.5), (S.fill(max(regs, 1) * D, seed, 6, 1, 0.7) + 0.25).reshape(max(regs, 1), D)

    def embed(lead, no_cls):
        T = NP + lead
        prow = batch * T + 5
        hi, lo = dev(np.full((batch * T, D), 0x7B7B, np.uint16)), dev(np.full((batch * T, D), 0x7B, np.uint8))
        part = dev(np.full((D // 64, prow, 2), -777.0, np.float32))
        vithip.op_gemm_lead(dev(a).ptr, dev(w).ptr, dev(bias).ptr, hi.ptr, batch * NP, D, K, vithip.EPI_PATCH_SPLIT, dt, dev(pos).ptr, NP, lead,
                            out16_ptr=lo.ptr, partials_ptr=part.ptr, prow=prow)
        if lead:
            vithip.op_lead_rows(hi.ptr, None if no_cls else dev(cls).ptr, None if no_cls else dev(pos).ptr, dev(reg).ptr if regs else None, lead,
                                batch, T, D, lo_ptr=lo.ptr, partials_ptr=part.ptr, prow=prow, dtype=dt)
        p = part.to_numpy(np.float32, (D // 64, prow, 2))
        assert (p[:, batch * T:] == -777.0).all() and not (p[:, :batch * T] == -777.0).any()   # every real row once, no padding row
        return hi.to_numpy(np.uint16, (batch, T, D)), lo.to_numpy(np.uint8, (batch, T, D)), p[:, :batch * T].reshape(D // 64, batch, T, 2)

    hi0, lo0, p0 = embed(1 + regs, False)
    hi, lo, p = embed(regs, True)
    assert np.array_equal(hi, hi0[:, 1:]) and np.array_equal(lo, lo0[:, 1:]) and same_bits(p, np.ascontiguousarray(p0[:, :, 1:]))


# ---- 2. the head's input, for bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("mode", list(MODES))
def test_head_input_is_the_token_features_of_the_same_forward(mode, path):
    cfg, dt, lnf, planes = PATHS[path]
    flags = MODES[mode]
    pool, D, Cn = R.pool_of(flags), cfg["dim"], cfg["classes"]
    W = R.head_width(cfg, flags)
    ctx = context(cfg, dt, flags, extra=lnf)
    assert ctx.ln_fold() == planes
    t = tensors_for(cfg, flags)
    d_g, d_b, d_w, d_hb = dev(t["lnf.weight"]), dev(t["lnf.bias"]), dev(t["head.weight"]), dev(t["head.bias"])
    plain = context(cfg, dt, flags & ~vithip.FLAG_POOL_MASK, extra=lnf) if pool == CLS_AVG else None   # POOL_CLS, the same tensors but the head
    for batch in BATCHES:
        images = S.make_images(cfg, 7, batch)
        logits = ctx.forward(images)
        tap = ctx.debug_read(1, batch * W).reshape(batch, W)
        assert np.isfinite(logits).all() and np.isfinite(tap).all()
        nmean = ctx.read_features(cls=False, patch=False, mean=True, elem=F32, norm=NORM)["mean"]
        if pool == AVG_NORM:
            assert same_bits(tap, nmean), batch
        elif pool == AVG_FCNORM:
            raw = ctx.read_features(cls=False, patch=False, mean=True, elem=F32, norm=RAW)["mean"]
            out = dev(np.zeros((batch, D), np.float32))
            vithip.op_layernorm_f32(dev(raw).ptr, batch, D, D, d_g.ptr, d_b.ptr, EPS, out.ptr)
            assert same_bits(tap, out.to_numpy(np.float32, (batch, D))), batch
        else:
            plain.forward(images)
            assert same_bits(np.ascontiguousarray(tap[:, :D]), plain.debug_read(1, batch * D).reshape(batch, D)), batch
            assert same_bits(np.ascontiguousarray(tap[:, D:]), nmean), batch
        out = dev(np.zeros((batch, Cn), np.float32))
        vithip.op_head_f32(dev(tap).ptr, d_w.ptr, d_hb.ptr, out.ptr, batch, Cn, W)
        assert same_bits(logits, out.to_numpy(np.float32, (batch, Cn))), batch
        assert same_bits(ctx.debug_read(1, batch * W).reshape(batch, W), tap)         # the read-outs left the head's input alone
    ctx.close()
    if plain:
        plain.close()


# ---- 3. the kernel alone ----------------------------------------------------------------------------------------------------
FORMS = {"bf16_planes": BF16, "fp16_planes": FP16, "fp8_planes": FP8, "fp32_rows": vithip.FEAT_FORM_F32}


@pytest.mark.parametrize("dim", [64, 128, 768, 1280, 2048])
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
def test_pool_kernel_gives_the_bits_of_the_two_kernel_mean(dim, form):
    fm = FORMS[form]
    rng = np.random.default_rng(dim + 7 * (fm + 2))
    gamma = (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.02 * rng.standard_normal(dim)).astype(np.float32)
    d_g, d_b = dev(gamma), dev(beta)
    for NP in (1, 2, 17, 50):
        for lead in (0, 1, 5):
            for batch in (1, 3):
                tokens = NP + lead
                x32 = (rng.standard_normal((batch, tokens, dim)) + rng.uniform(-0.8, 0.8, (batch, tokens, 1))).astype(np.float32)
                x32[batch - 1, lead + min(1, NP - 1), dim // 3] = np.float32(300.0)    # one 300 sigma element in a patch row
                hi, lo, _ = FR.split_planes(x32.reshape(batch * tokens, dim), fm)
                d_hi, d_lo = dev(hi), dev(lo) if lo is not None else None
                # the comparison run: vh_op_token_features2 needs lead >= 1, so lead = 0 gets one dummy row in front of every image
                if lead == 0:
                    pad = np.concatenate([np.full((batch, 1, dim), 7.0, np.float32), x32], 1)
                    h2, l2, _ = FR.split_planes(pad.reshape(batch * (tokens + 1), dim), fm)
                    r_hi, r_lo, r_tokens, r_lead = dev(h2), dev(l2) if l2 is not None else None, tokens + 1, 1
                else:
                    r_hi, r_lo, r_tokens, r_lead = d_hi, d_lo, tokens, lead
                for norm in (RAW, NORM):
                    g = Guarded(batch * dim * 4)
                    vithip.op_pool_rows(d_hi.ptr, d_lo.ptr if d_lo else None, fm, batch, tokens, lead, dim, d_g.ptr, d_b.ptr, EPS, norm, g.ptr)
                    got = g.read(np.float32, (batch, dim))                            # (the canaries around the output are checked here)
                    g.free()
                    ref = dev(np.zeros((batch, dim), np.float32))
                    vithip.op_token_features2(r_hi.ptr, r_lo.ptr if r_lo else None, fm, batch, r_tokens, r_lead, dim, d_g.ptr, d_b.ptr, EPS, F32, norm,
                                              None, vithip.FEAT_ROWS, ref.ptr, None)
                    assert same_bits(got, ref.to_numpy(np.float32, (batch, dim))), (form, dim, NP, lead, batch, norm)
                for b in _KEEP[2:]:
                    b.free()
                del _KEEP[2:]


# ---- 4. parity with the transformers fixtures -------------------------------------------------------------------------------
_FIX = {}


def fixture(path):
    if path not in _FIX:
        z = np.load(path)
        cfg = dict(zip(CFG_KEYS, (int(v) for v in z["config"])))
        wseed, iseed, batch, flags = (int(v) for v in z["meta"])
        blob = R.pack_blob(cfg, H.fixture_tensors(str(z["kind"]), cfg, flags, wseed), flags, float(z["ln_eps"]))
        if str(z["kind"]) == "dinov2":   # (the LayerScale is folded by the converter)
            sd = H.dinov2_classifier_state_dict(cfg, H.fixture_tensors("dinov2", cfg, flags, wseed), wseed)
            blob = vithip.blob_from_dinov2_state_dict(sd, dict(cfg, registers=R.registers_of(flags)), float(z["ln_eps"]), pool=CLS_AVG)
        images = S.make_images(cfg, iseed, batch)
        _FIX[path] = (z, cfg, flags, blob, images, float(z["ln_eps"]), R.forward(cfg, blob, images, flags, float(z["ln_eps"]), np.float64))
    return _FIX[path]


def test_fixtures_are_present():
    assert len(GOLDEN) == 4, GOLDEN


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p).split("_s")[0] for p in GOLDEN])
def test_fixture_logits_and_head_inputs(path, dt):
    z, cfg, flags, blob, images, eps, _ = fixture(path)
    ctx = vithip.VitContext(dict(cfg, registers=R.registers_of(flags)), dtype=dt, max_batch=len(images), flags=flags & ~R.FLAG_REGISTERS_MASK, ln_eps=eps)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    tap = ctx.debug_read(1, len(images) * R.head_width(cfg, flags)).reshape(len(images), -1)
    ctx.close()
    e_l, e_h = rel(got, z["logits"]), rel(tap, z["head_input"])
    print(f"\n[pool] {os.path.basename(path).split('_s')[0]} {NAME[dt]}: logits {e_l:.3e} head input {e_h:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and np.isfinite(tap).all()
    assert e_l <= MODEL_TOL[dt] and e_h <= MODEL_TOL[dt], (e_l, e_h)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p).split("_s")[0] for p in GOLDEN])
def test_fp8_forwards_track_the_emulation(path):
    z, cfg, flags, blob, images, eps, ref64 = fixture(path)
    ref32 = ref64.astype(np.float32)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    ctx = vithip.VitContext(dict(cfg, registers=R.registers_of(flags)), dtype=FP8, max_batch=len(images), flags=flags & ~R.FLAG_REGISTERS_MASK, ln_eps=eps)
    ctx.load_weights(blob)
    got, folded = ctx.forward(images), ctx.ln_fold()
    tap = ctx.debug_read(1, len(images) * R.head_width(cfg, flags)).reshape(len(images), -1)
    ctx.close()
    emu, emu_h = R.forward(cfg, blob, images, flags, eps, fp8="folded" if folded else "plain", want_head=True)
    assert np.isfinite(got).all() and np.isfinite(tap).all()
    # the same criterion for the logits and for the head's input, each against its own fixture vector
    for what, g, e, ref in (("logits", got, emu, ref32), ("head input", tap, emu_h, z["head_input"].astype(np.float32))):
        r_emu32, r_gpu32, r_gpuemu = rms(e, ref), rms(g, ref), rms(g, e)
        print(f"\n[pool fp8] {os.path.basename(path).split('_s')[0]} (folded {folded}) {what}: rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3 and r_gpuemu <= 1.5 * r_emu32 + 1e-3, what


# ---- 5. the same logit bits on every route into a forward -------------------------------------------------------------------
ROUTE_MODES = ["nocls_avg_norm_r4", "cls_avg", "avg_fcnorm"]


@pytest.mark.parametrize("mode", ROUTE_MODES)
def test_same_logit_bits_alone_in_a_batch_across_streams_and_graph_replay(mode):
    flags = MODES[mode]
    images = S.make_images(A, 8, 5)
    ctx = context(A, BF16, flags)
    five = ctx.forward(images)
    assert np.isfinite(five).all()
    one = context(A, BF16, flags, max_batch=1)
    assert same_bits(one.forward(images[2:3]), five[2:3])                             # image 2 alone at max_batch 1
    one.close()
    assert same_bits(ctx.forward(images[1:4]), five[1:4])
    ctx.set_streams(2)
    assert same_bits(ctx.forward(images), five)
    W = R.head_width(A, flags)
    tap = ctx.debug_read(1, 5 * W)                                                    # the parts wrote their own slices of the head's input
    ctx.set_streams(1)
    ctx.forward(images)
    assert same_bits(ctx.debug_read(1, 5 * W), tap)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert same_bits(ctx.forward(images), five)
    ctx.set_streams(2)
    for _ in range(3):
        assert same_bits(ctx.forward(images), five)
    ctx.set_graph(False)
    ctx.close()


@pytest.mark.parametrize("mode", ROUTE_MODES)
def test_same_logit_bits_through_the_u8_ring(mode):
    flags = MODES[mode]
    u8 = make_u8_images(5, A["image_size"], 3, seed=3)
    ctx = context(A, BF16, flags)
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


# ---- 5b. a blob of another model is refused ---------------------------------------------------------------------------------
def _forge(blob, flags):
    out = blob.copy()
    bits = int(out[52:56].view(np.uint32)[0])
    out[52:56] = np.array([(bits & 1) | flags], np.uint32).view(np.uint8)            # (bit 0: a file's checksum mark stays)
    return out


@pytest.mark.parametrize("mode", ["avg_norm", "nocls_avg_fcnorm_r4"])
def test_a_blob_with_other_pool_or_class_token_bits_is_refused(mode, tmp_path):
    """The header bits are the only thing that tells an AVG_NORM blob from an AVG_FCNORM blob (same size, same shapes): a blob whose
    bits 15 or 16 .. 17 differ from the context's is refused with the bit's own message, through vh_load_weights and
    vh_load_weights_file, and the refused loads change nothing."""
    flags = {"avg_norm": POOL(AVG_NORM), "nocls_avg_fcnorm_r4": NO_CLS | POOL(AVG_FCNORM) | REG(4)}[mode]
    cfg, pool, regs = B, R.pool_of(flags), flags & R.FLAG_REGISTERS_MASK
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags, ln_eps=EPS)
    ctx.init_weights_seeded(17)
    blob = ctx.export_weights()
    assert np.array_equal(blob, R.make_blob(cfg, 17, flags))                         # the seeded tensors keep their ids; the bits in the header
    path, bad = str(tmp_path / "m.vhblob"), str(tmp_path / "forged.vhblob")
    ctx.save_weights_file(path)
    assert vithip.blob_file_flags(path) == flags
    images = S.make_images(cfg, 2, 2)
    want = ctx.forward(images)
    ctx.load_weights_file(path)
    assert same_bits(ctx.forward(images), want)
    file_bytes = np.fromfile(path, np.uint8)
    other_pool = AVG_FCNORM if pool == AVG_NORM else AVG_NORM
    forged = [((flags & ~vithip.FLAG_POOL_MASK) | POOL(other_pool), f"pooling mode {other_pool}, the context's VH_FLAG_POOL says {pool}"),
              (flags ^ NO_CLS, rf"header bit 15 \(no class token\) is {0 if flags & NO_CLS else 1}, the context's VH_FLAG_NO_CLS is {1 if flags & NO_CLS else 0}")]
    for f, msg in forged:                                                             # the right size, another model
        with pytest.raises(vithip.VhError, match=msg) as e:
            ctx.load_weights(_forge(blob, f))
        assert e.value.code == 1
        _forge(file_bytes, f).tofile(bad)
        with pytest.raises(vithip.VhError, match=msg):
            ctx.load_weights_file(bad)
    sizes = [regs | POOL(CLS_AVG), regs | POOL(AVG_NORM) if flags & NO_CLS else regs | NO_CLS | POOL(AVG_NORM)]
    for f in sizes:                                                                   # another size: a [C][2 D] head, a class token more / less
        other = R.make_blob(cfg, 17, f)
        assert other.nbytes != blob.nbytes
        with pytest.raises(vithip.VhError, match="bytes"):
            ctx.load_weights(other)
        other.tofile(bad)
        with pytest.raises(vithip.VhError, match="bytes"):
            ctx.load_weights_file(bad)
    assert same_bits(ctx.forward(images), want)                                       # the refused loads changed nothing
    ctx.close()
    plain = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=regs, ln_eps=EPS)   # and the other way round: a POOL_CLS context
    if not flags & NO_CLS:
        with pytest.raises(vithip.VhError, match="pooling mode 1, the context's VH_FLAG_POOL says 0"):
            plain.load_weights_file(path)
    else:
        with pytest.raises(vithip.VhError, match="bytes"):
            plain.load_weights_file(path)
    plain.close()


# ---- 6. features on the new contexts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("regs", [0, 4])
@pytest.mark.parametrize("path", ["a_bf16", "a_fp8", "b_bf16"])
def test_features_of_a_context_without_a_class_token(path, regs):
    cfg, dt, lnf, _ = PATHS[path]
    flags = NO_CLS | POOL(AVG_NORM) | REG(regs)
    NP, D, batch = S.tokens(cfg) - 1, cfg["dim"], 3
    g = cfg["image_size"] // cfg["patch_size"]
    ctx = context(cfg, dt, flags, extra=lnf)
    ctx.forward(S.make_images(cfg, 7, batch))
    x = hidden(ctx, batch)
    # cls is refused, nothing enqueued, nothing written: host form and device form
    for fn in (lambda: ctx.read_features(cls=True, patch=False), lambda: ctx.read_layer_features(-1, cls=True, patch=False)):
        with pytest.raises(vithip.VhError, match="without a class token") as e:
            fn()
        assert e.value.code == VH_ERR_UNSUPPORTED
    gc, gp = Guarded(batch * D * 4), Guarded(batch * NP * D * 4)
    with pytest.raises(vithip.VhError, match="without a class token"):
        ctx.read_features_device(vithip.Features(gc.ptr, gp.ptr, None, F32, RAW))
    assert gc.untouched() and gp.untouched()
    gc.free()
    gp.free()
    with pytest.raises(ValueError, match="without a class token"):
        ctx.get_intermediate_layers(1, return_class_token=True)
    raw = ctx.read_layer_features(-1, cls=False, patch=True, mean=True, reg=regs > 0, elem=F32, norm=RAW)
    assert same_bits(raw["patch"], x[:, regs:]) and same_bits(raw["mean"], FR.mean_chain(raw["patch"]))
    if regs:
        assert same_bits(raw["reg"], x[:, :regs])
    else:
        with pytest.raises(vithip.VhError, match="without register tokens"):
            ctx.read_layer_features(-1, cls=False, patch=False, reg=True)
    nchw = ctx.read_layer_features(-1, cls=False, patch=True, elem=F32, norm=RAW, nchw=True)["patch"]
    assert same_bits(nchw, np.ascontiguousarray(x[:, regs:].transpose(0, 2, 1)).reshape(batch, D, g, g))
    nrm = ctx.read_features(cls=False, patch=True, mean=True, elem=F32, norm=NORM)
    t = tensors_for(cfg, flags)
    ref = FR.layernorm64(x[:, regs:], t["lnf.weight"], t["lnf.bias"], EPS)
    assert float(np.abs(nrm["patch"] - ref).max()) <= FR.NORM_BOUND * float(np.abs(ref).max())
    assert same_bits(nrm["mean"], FR.mean_chain(nrm["patch"]))
    assert same_bits(nrm["mean"], ctx.debug_read(1, batch * D).reshape(batch, D))         # and that is what the head multiplied
    ctx.close()


@pytest.mark.parametrize("mode", ["avg_norm", "cls_avg"])
def test_cls_feature_of_a_pooled_context_stays_the_normalised_class_token(mode):
    flags = MODES[mode]
    ctx = context(A, BF16, flags)
    ctx.forward(S.make_images(A, 7, 3))
    x = hidden(ctx, 3)
    f = ctx.read_features(cls=True, patch=False, mean=False, elem=F32, norm=NORM)
    t = tensors_for(A, flags)
    ref = FR.layernorm64(x[:, :1], t["lnf.weight"], t["lnf.bias"], EPS)[:, 0]
    assert float(np.abs(f["cls"] - ref).max()) <= FR.NORM_BOUND * float(np.abs(ref).max())
    assert same_bits(ctx.read_features(cls=True, patch=False, elem=F32, norm=RAW)["cls"], x[:, 0])
    ctx.close()
