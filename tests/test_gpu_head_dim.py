"""GPU parity at head dims other than 64: the attention kernel of kernels_attn_hd.hip through its own tap vh_op_attention_hd at
every supported head dim and token count, inside whole forwards of models with head dims 32 ... 128 on every LayerNorm path,
the head-dim golden fixtures, bit invariance across batch, streams and graph replay, and ViT-H/14-224, against the CPU oracle.
Tolerances are the existing ones: ATT_TOL of test_gpu_ops for the operator, test_gpu_vit's model-level bounds (fp16 1e-3,
bf16 1e-2) and test_gpu_fp8's statistics.  The configurations are defined here (not in vh_synth.CONFIGS, whose every entry
other tests run)."""
import glob
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O
import vh_synth as S
import vit_ref as R
from vh_testlib import _release_buffers, dev, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
DT = [BF16, FP16]
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
ATT_TOL = {BF16: 1.2e-2, FP16: 1.5e-3}   # test_gpu_ops.ATT_TOL: P and O are rounded to 16 bit
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}     # test_gpu_vit.TOL (bf16: a regression bound, not the north star's tolerance)
HEAD_DIMS = [32, 48, 64, 80, 96, 112, 128]
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "headdim", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


def _cfg(image, patch, dim, heads, mlp, layers, classes=40):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


# dims that are multiples of 256: the LayerNorm fold and the split residual apply
HD80_D1280 = _cfg(64, 8, 1280, 16, 2560, 2)    # 65 tokens
HD96_D768 = _cfg(64, 16, 768, 8, 1536, 2)      # 17 tokens
HD128_D256 = _cfg(96, 16, 256, 2, 512, 2)      # 37 tokens
HD32_D256 = _cfg(64, 8, 256, 8, 512, 2)        # 65 tokens
# dim 320: none of them applies (the plain LayerNorm path whatever the flags say)
HD80_D320 = _cfg(64, 16, 320, 4, 640, 2)
VIT_H14_224 = _cfg(224, 14, 1280, 16, 5120, 32, classes=1000)   # 257 tokens


def rnd16(a, dt):
    return O.round_bf16(a) if dt == BF16 else O.round_fp16(a)


def q_scale(hd):
    """head_dim^-1/2 * log2(e) as the library folds it into Wq / bq (vh_kernels.h attention_q_scale)."""
    return np.float32(1.4426950408889634 / np.sqrt(np.float64(hd)))


def prescale_q(qkv, D, hd, dt):
    """q columns x q_scale(hd) rounded to 16 bit as the q|k|v GEMM delivers them; the oracle gets the same q back in its own
    convention (it scales by hd^-1/2 itself and works in base e) -- test_gpu_ops.prescale_q."""
    pre = qkv.copy()
    pre[:, :D] = rnd16(pre[:, :D] * q_scale(hd), dt)
    ref_in = pre.astype(np.float64)
    ref_in[:, :D] /= np.float64(q_scale(hd))
    return pre, ref_in.astype(np.float32)


def make_qkv(batch, tokens, heads, hd, dt, seed):
    D = heads * hd
    qkv = rnd16((S.fill(batch * tokens * 3 * D, seed, tokens + hd, 0) * 1.5).reshape(batch * tokens, 3 * D), dt)
    return prescale_q(qkv, D, hd, dt)


def run_hd(pre, batch, tokens, heads, hd, dt):
    D = heads * hd
    out = dev(np.full(batch * tokens * D * 2, 0xFF, dtype=np.uint8))   # an unwritten element reads back as NaN
    vithip.op_attention_hd(dev(vithip.to16(pre, dt)).ptr, batch, tokens, heads, hd, out.ptr, dt)
    return vithip.from16(out.to_numpy(np.uint16, (batch * tokens, D)), dt)


# ---- operator level ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_attention_hd_tap_matches_the_oracle(hd, dt):
    # one tile, tile edges (31 / 32 / 33), one wave to a full workgroup, several query slabs, the ViT-B / ViT-H / 336 / 448 token
    # counts; heads x batch > 1 everywhere so head and image bases are exercised
    for tokens, batch, heads in ((1, 2, 2), (2, 1, 3), (31, 2, 2), (32, 1, 2), (33, 2, 1), (197, 2, 2), (257, 1, 3),
                                 (577, 1, 2), (1025, 1, 2)):
        pre, qkv = make_qkv(batch, tokens, heads, hd, dt, 31)
        ref = O.attention(qkv, batch, tokens, heads, dh=hd)
        got = run_hd(pre, batch, tokens, heads, hd, dt)
        assert np.isfinite(got).all(), (hd, tokens)
        assert rel(got, ref) <= ATT_TOL[dt], (hd, tokens, batch, heads, rel(got, ref))


@pytest.mark.parametrize("hd", [48, 80, 128])
def test_attention_hd_tap_at_4097_tokens(hd):
    batch, tokens, heads = 1, 4097, 2
    for dt in DT:
        pre, qkv = make_qkv(batch, tokens, heads, hd, dt, 32)
        ref = O.attention(qkv, batch, tokens, heads, dh=hd)
        got = run_hd(pre, batch, tokens, heads, hd, dt)
        assert np.isfinite(got).all() and rel(got, ref) <= ATT_TOL[dt], (hd, NAME[dt], rel(got, ref))


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
@pytest.mark.parametrize("hd", [32, 80, 112, 128])
def test_attention_hd_spiked_scores_force_rescale_in_a_late_tile(hd, dt):
    # test_gpu_long_sequence's spiked case at other head dims: query 5 meets key 1000 (tile 31) with a score far above its
    # tile-0 shift, so the deferred rescale runs in a late key tile; query 40's larger score sits early (key 3)
    batch, heads, tokens, D = 1, 1, 1025, hd
    qkv = (S.fill(tokens * 3 * D, 11, 1, 0) * 0.5).reshape(tokens, 3 * D)
    spike = 4.0 * np.sqrt(64.0 / hd)   # the same score at every head dim
    qkv[5, :D] = spike
    qkv[1000, D:2 * D] = spike
    qkv[40, :D] = -0.75 * spike
    qkv[3, D:2 * D] = -0.75 * spike
    qkv = rnd16(qkv, dt)
    pre, qkv = prescale_q(qkv, D, hd, dt)
    ref = O.attention(qkv, batch, tokens, heads, dh=hd)
    got = run_hd(pre, batch, tokens, heads, hd, dt)
    assert np.isfinite(got).all()
    assert rel(got, ref) <= ATT_TOL[dt]
    # query 5 attends essentially only to key 1000
    ulp = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    assert np.abs(got[5] - qkv[1000, 2 * D:]).max() <= 2 * ulp * np.abs(qkv[1000, 2 * D:]).max() + 1e-6


@pytest.mark.parametrize("hd", [48, 80, 128])
def test_attention_hd_e4m3_output(hd):
    # bf16 in, e4m3 out (the VH_DTYPE_FP8 contexts' instantiation)
    for tokens, batch, heads in ((257, 2, 2), (33, 1, 3)):
        D = heads * hd
        pre, qkv = make_qkv(batch, tokens, heads, hd, BF16, 33)
        ref = O.attention(qkv, batch, tokens, heads, dh=hd)
        o8 = dev(np.zeros(batch * tokens * D, dtype=np.uint8))
        vithip.op_attention_hd(dev(vithip.to16(pre, BF16)).ptr, batch, tokens, heads, hd, o8.ptr, FP8)
        got = vithip.from_e4m3(o8.to_numpy(np.uint8, (batch * tokens, D)))
        want = O.quant_e4m3(ref)
        assert np.isfinite(got).all()
        # the oracle rounded to e4m3: equal except where bf16 P / O rounding moved a value across an e4m3 rounding boundary
        assert (got == want).mean() >= 0.75, float((got == want).mean())
        # bf16 P/O rounding inside the kernel (ATT_TOL) plus half an e4m3 step on the way out (test_gpu_fp8)
        assert np.all(np.abs(got - ref) <= 2.0 ** -4 * np.abs(ref) + ATT_TOL[BF16] * np.abs(ref).max())


STREAM64 = os.path.join(HERE, "golden", "attn_stream", "stream64_parent.npz")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: NAME[d])
def test_attention_hd_at_head_dim_64_is_the_streaming_kernel_bit_for_bit(dt):
    # Head dim 64 is an instantiation of the one streaming kernel; the 64-wide kernel it replaced had a source file of its own.
    # The fixture (golden/make_golden_attn_stream.py) holds that kernel's stored bytes: both taps, and the dispatcher from 641
    # tokens on, reproduce them, and stay inside the operator's tolerance against the oracle.
    g = np.load(STREAM64)
    din = BF16 if dt == FP8 else dt                  # VH_DTYPE_FP8: bf16 in, e4m3 out
    width, bits = (1, np.uint8) if dt == FP8 else (2, np.uint16)
    for i, (tokens, batch, heads) in enumerate(g["cases"].tolist()):
        pre, qkv = make_qkv(batch, tokens, heads, 64, din, int(g["seed"][0]))
        qbits = vithip.to16(pre, din)
        assert _sha(qbits) == str(g[f"in_sha256_{NAME[dt]}"][i]), ("the input generator drifted", tokens)
        q = dev(qbits)
        shape = (batch * tokens, heads * 64)

        def stored(call):
            o = dev(np.full(shape[0] * shape[1] * width, 0xFF, dtype=np.uint8))
            call(o)
            return o.to_numpy(bits, shape)

        taps = [("stream", stored(lambda o: vithip.op_attention_stream(q.ptr, batch, tokens, heads, o.ptr, dt))),
                ("hd", stored(lambda o: vithip.op_attention_hd(q.ptr, batch, tokens, heads, 64, o.ptr, dt)))]
        if tokens >= 641:
            taps.append(("dispatch", stored(lambda o: vithip.op_attention(q.ptr, batch, tokens, heads, o.ptr, dt))))
        for tap, got in taps:
            assert _sha(got) == str(g[f"out_sha256_{NAME[dt]}"][i]), (tap, tokens)
            if i < int(g["stored"][0]):
                want = g[f"out_{NAME[dt]}_{tokens}"]
                assert np.array_equal(got, want), (tap, tokens, int((got != want).sum()))
        ref = O.attention(qkv, batch, tokens, heads, dh=64)
        if dt == FP8:
            # test_attention_hd_e4m3_output's bound with e4m3's subnormal range added (the outputs of 4097 keys are small):
            # half an e4m3 step is 2^-4 |x| for normal values and 2^-10 below 2^-6 (subnormal spacing 2^-9), on top of the
            # bf16 P / O rounding inside the kernel (ATT_TOL)
            got = vithip.from_e4m3(taps[0][1])
            assert np.isfinite(got).all()
            half_step = np.maximum(2.0 ** -4 * np.abs(ref), 2.0 ** -10)
            assert np.all(np.abs(got - ref) <= half_step + ATT_TOL[BF16] * np.abs(ref).max()), tokens
        else:
            got = vithip.from16(taps[0][1], dt)
            assert rel(got, ref) <= ATT_TOL[dt], (tokens, rel(got, ref))


# ---- model level -------------------------------------------------------------------------------------------------------

def _forward(cfg, blob, images, dt, flags=0, max_batch=None):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=max_batch or len(images), flags=flags)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    fold = ctx.ln_fold()
    hm = int(ctx.debug_read(4, 1)[0])
    ctx.close()
    return got, fold, hm


FLAGS = [(0, "default"), (vithip.FLAG_LN_FOLD_OFF, "fold_off"), (vithip.FLAG_LN_FOLD_ON, "fold_on")]
MODELS = [("hd80_d1280", HD80_D1280), ("hd96_d768", HD96_D768), ("hd128_d256", HD128_D256), ("hd32_d256", HD32_D256),
          ("hd80_d320", HD80_D320)]
_REF = {}


def _model(name, cfg):
    if name not in _REF:
        blob, images = O.make_blob(cfg, 3), S.make_images(cfg, 4, 3)
        _REF[name] = (blob, images, O.vit_forward(cfg, blob, images))
    return _REF[name]


@pytest.mark.parametrize("name,cfg", MODELS, ids=[m[0] for m in MODELS])
def test_models_match_the_oracle_on_every_layernorm_path(name, cfg):
    blob, images, ref = _model(name, cfg)
    for dt in DT:
        for flags, label in FLAGS:
            got, fold, hm = _forward(cfg, blob, images, dt, flags)
            e = rel(got, ref)
            print(f"\n[headdim] {name} {NAME[dt]} {label} (fold {fold}): logits {e:.3e}")
            assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], label, e)
            assert hm == 0
            if cfg["dim"] % 256 == 0 and flags != vithip.FLAG_LN_FOLD_OFF:
                assert fold, label


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_hd80_with_the_tiled_hidden_activation(dt):
    # enough rows for the persistent GEMM form: the MLP hidden activation is tiled (debug tap 3) while q|k|v and the attention
    # output stay row-major (tap 4); the first images against the oracle, the whole batch against VH_H_TILED=0
    cfg = HD80_D1280
    n = 420
    blob, images = O.make_blob(cfg, 3), S.make_images(cfg, 4, n)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=n)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    tiled, hm = int(ctx.debug_read(3, 1)[0]), int(ctx.debug_read(4, 1)[0])
    ctx.close()
    print(f"\n[headdim] hd80_d1280 b{n} {NAME[dt]}: h tiled {tiled}, q|k|v head-major {hm}")
    assert tiled == 1 and hm == 0
    ref = O.vit_forward(cfg, blob, images[:3])
    assert np.isfinite(got).all() and rel(got[:3], ref) <= MODEL_TOL[dt], rel(got[:3], ref)
    os.environ["VH_H_TILED"] = "0"
    try:
        ctx = vithip.VitContext(cfg, dtype=dt, max_batch=n)
    finally:
        del os.environ["VH_H_TILED"]
    ctx.load_weights(blob)
    plain = ctx.forward(images)
    assert int(ctx.debug_read(3, 1)[0]) == 0
    ctx.close()
    assert np.array_equal(plain, got)


@pytest.mark.parametrize("name,cfg", [("hd128_d256", HD128_D256), ("hd96_d768", HD96_D768)])
def test_fp8_forwards_track_the_emulation(name, cfg):
    # test_any_patch's test_tiny_patch14_fp8_forward_tracks_the_emulation criterion (dims multiples of 128)
    blob, images, ref32 = _model(name, cfg)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    emu = {}
    for flags, label in FLAGS:
        got, folded, _ = _forward(cfg, blob, images, FP8, flags)
        if folded not in emu:
            emu[folded] = O.vit_forward(cfg, blob, images, fp8="folded" if folded else True)
        r_emu32, r_gpu32, r_gpuemu = rms(emu[folded], ref32), rms(got, ref32), rms(got, emu[folded])
        print(f"\n[headdim fp8] {name} {label} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} "
              f"gpu-emu {r_gpuemu:.3e}")
        assert np.isfinite(got).all()
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3, label
        assert r_gpuemu <= 1.5 * r_emu32 + 1e-3, label
        assert rel(got, ref32) <= 0.25, label


@pytest.mark.parametrize("name,cfg", [("hd80_d320", HD80_D320), ("hd128_d256", HD128_D256)])
def test_weight_only_e4m3(name, cfg):
    blob, images, _ = _model(name, cfg)
    blob_q = R.weight_only_e4m3_blob(cfg, blob)
    got, _, _ = _forward(cfg, blob, images, FP16, vithip.FLAG_W8_E4M3)
    host_quantised, _, _ = _forward(cfg, blob_q, images, FP16)
    e = rel(got, O.vit_forward(cfg, blob_q, images))
    print(f"\n[headdim] {name} fp16 weight-only e4m3 vs its own fp32 model: {e:.3e}")
    assert np.isfinite(got).all() and np.array_equal(got, host_quantised)
    assert e <= MODEL_TOL[FP16], e


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_headdim_fixture_logits_match_the_golden_fp64_logits(path):
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    wseed, iseed, batch = [int(v) for v in g["meta"]]
    blob, images = S.make_blob(cfg, wseed), S.make_images(cfg, iseed, batch)
    for dt in DT:
        got, _, _ = _forward(cfg, blob, images, dt)
        e = rel(got, g["logits_f64"])
        print(f"\n[headdim] fixture {os.path.basename(path)} {NAME[dt]}: logits vs fp64 golden {e:.3e}")
        assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], e)


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_same_bits_across_batch_streams_graph_replay_and_the_class_token_tail(dt):
    cfg = HD80_D1280
    blob = _model("hd80_d1280", cfg)[0]
    images = S.make_images(cfg, 8, 7)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=7)
    ctx.load_weights(blob)
    one = ctx.forward(images[:1])
    seven = ctx.forward(images)
    assert int(ctx.debug_read(4, 1)[0]) == 0   # q|k|v row-major at head dim 80
    assert np.isfinite(seven).all()
    assert np.array_equal(seven[:1], one)
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
    # VH_FLAG_CLS_TAIL falls back to the full last layer at head dim 80: the default launch sequence, the same bits
    base, _, _ = _forward(cfg, blob, images, dt, vithip.FLAG_LN_FOLD_ON)
    tail, _, _ = _forward(cfg, blob, images, dt, vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL)
    assert np.array_equal(tail, base)


# ---- ViT-H/14 ------------------------------------------------------------------------------------------------------------

_H = {}


def _vit_h():
    if not _H:
        blob, images = O.make_blob(VIT_H14_224, 0), S.make_images(VIT_H14_224, 1, 4)
        _H.update(blob=blob, images=images, ref=O.vit_forward(VIT_H14_224, blob, images))
    return _H


# 32 layers, deeper than ViT-L/16-384: measured 7.7e-4 .. 9.0e-4 per image on these 4 images, inside
# the north star's 1e-3, which is asserted
VIT_H_FP16_TOL = 1e-3


def test_vit_h14_224_fp16_matches_the_oracle():
    d = _vit_h()
    got, _, _ = _forward(VIT_H14_224, d["blob"], d["images"], FP16)
    assert np.isfinite(got).all()
    per = np.abs(got - d["ref"]).max(1) / np.abs(d["ref"]).max()
    print(f"\n[headdim] ViT-H/14-224 fp16 b4: logits {rel(got, d['ref']):.3e}, per-image {' '.join(f'{x:.2e}' for x in per)}")
    assert per.max() <= VIT_H_FP16_TOL, per


def test_vit_h14_224_bf16_regression_bound():
    d = _vit_h()
    got, _, _ = _forward(VIT_H14_224, d["blob"], d["images"], BF16)
    e = rel(got, d["ref"])
    print(f"\n[headdim] ViT-H/14-224 bf16 b4: logits {e:.3e}")
    assert np.isfinite(got).all() and e <= MODEL_TOL[BF16], e
