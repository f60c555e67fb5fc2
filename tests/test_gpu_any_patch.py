"""GPU parity at any patch size: the padded patch embedding (im2col_pad_kernel + permute_patch_pad_kernel, the patch GEMM on
the patch vector zero-padded to a multiple of 64) through its own tap vh_op_im2col_padded, inside whole forwards of patch-14
models against the CPU oracle and the patch-14 golden fixture, and across batch, streams and graph replay.
Tolerances are the existing ones: test_gpu_vit's model-level bounds (fp16 1e-3, bf16 1e-2) and test_gpu_fp8's statistics.
The patch-14 configurations are defined here (not in vh_synth.CONFIGS, whose every entry other tests run)."""
import glob
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
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}     # test_gpu_vit.TOL (bf16: a regression bound, not the north star's tolerance)
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "patch14", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


def _cfg(image, patch, dim, heads, mlp, layers, classes=40, channels=3):
    return dict(image_size=image, patch_size=patch, channels=channels, dim=dim, heads=heads, mlp_dim=mlp, layers=layers,
                classes=classes)


TINY_P14 = _cfg(112, 14, 256, 4, 512, 2)                          # 65 tokens, patch vector 588 -> 640
VIT_B14_224 = _cfg(224, 14, 768, 12, 3072, 12, classes=1000)      # 257 tokens
DINO_S14_518 = _cfg(518, 14, 384, 6, 1536, 12, classes=1000)      # 1370 tokens: the K/V-streaming attention
VIT_L14_224 = _cfg(224, 14, 1024, 16, 4096, 24, classes=1000)     # 257 tokens


def rnd16(a, dt):
    return O.round_bf16(a) if dt == BF16 else O.round_fp16(a)


# ---- the operator tap ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_im2col_padded_tap_is_the_rounded_oracle_im2col_and_zero_columns(dt):
    for image, patch, ch, extra in ((56, 14, 3, None), (224, 14, 3, None), (42, 14, 1, None), (35, 7, 3, None),
                                    (64, 16, 3, 0), (64, 16, 3, 64)):
        kp = patch * patch * ch
        kpad = -(-kp // 64) * 64 if extra is None else kp + extra
        batch, g = 3, image // patch
        rows = batch * g * g
        x = (S.fill(batch * image * image * ch, 41, image + ch, 0) * 3.0).reshape(batch, image, image, ch)
        want = np.zeros((rows, kpad), dtype=np.uint16)
        want[:, :kp] = vithip.to16(rnd16(O.im2col(x, patch), dt), dt)
        out = dev(np.full(rows * kpad * 2, 0xFF, dtype=np.uint8))   # an unwritten column reads back as NaN
        vithip.op_im2col_padded(dev(x).ptr, batch, image, patch, ch, kpad, out.ptr, dt)
        got = out.to_numpy(np.uint16, (rows, kpad))
        assert np.array_equal(got, want), (image, patch, ch, kpad, int((got != want).sum()))
        if (image, patch, ch, extra) == (64, 16, 3, 0):
            plain = dev(np.full(rows * kpad * 2, 0xFF, dtype=np.uint8))
            vithip.op_im2col(dev(x).ptr, batch, image, patch, ch, plain.ptr, dt)
            assert np.array_equal(plain.to_numpy(np.uint16, (rows, kpad)), got)


# ---- a tiny patch-14 model -----------------------------------------------------------------------------------------------

def _forward(cfg, blob, images, dt, flags=0):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    fold = ctx.ln_fold()
    ctx.close()
    return got, fold


FLAGS = [(0, "default"), (vithip.FLAG_LN_FOLD_OFF, "fold_off"), (vithip.FLAG_LN_FOLD_ON, "fold_on")]
_TINY = {}


def _tiny():
    if not _TINY:
        blob, images = O.make_blob(TINY_P14, 3), S.make_images(TINY_P14, 4, 3)
        _TINY.update(blob=blob, images=images, ref=O.vit_forward(TINY_P14, blob, images))
    return _TINY


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_tiny_patch14_forward_matches_the_oracle_on_every_layernorm_path(dt):
    d = _tiny()
    for flags, label in FLAGS + [(vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL, "fold_on+cls_tail")]:
        got, _ = _forward(TINY_P14, d["blob"], d["images"], dt, flags)
        e = rel(got, d["ref"])
        print(f"\n[patch14] tiny {NAME[dt]} {label}: logits {e:.3e}")
        assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], label, e)


def test_tiny_patch14_fp8_forward_tracks_the_emulation():
    # test_gpu_fp8.test_logits_track_the_fp8_emulation_and_the_fp32_forward's statistics
    d = _tiny()
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    emu = {}
    for flags, label in FLAGS:
        got, folded = _forward(TINY_P14, d["blob"], d["images"], FP8, flags)
        if folded not in emu:
            emu[folded] = O.vit_forward(TINY_P14, d["blob"], d["images"], fp8="folded" if folded else True)
        r_emu32, r_gpu32, r_gpuemu = rms(emu[folded], d["ref"]), rms(got, d["ref"]), rms(got, emu[folded])
        print(f"\n[patch14 fp8] tiny {label} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} "
              f"gpu-emu {r_gpuemu:.3e}")
        assert np.isfinite(got).all()
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3, label
        assert r_gpuemu <= 1.5 * r_emu32 + 1e-3, label
        assert rel(got, d["ref"]) <= 0.25, label


def test_tiny_patch14_weight_only_e4m3():
    d = _tiny()
    blob_q = R.weight_only_e4m3_blob(TINY_P14, d["blob"])
    got, _ = _forward(TINY_P14, d["blob"], d["images"], FP16, vithip.FLAG_W8_E4M3)
    host_quantised, _ = _forward(TINY_P14, blob_q, d["images"], FP16)
    e = rel(got, O.vit_forward(TINY_P14, blob_q, d["images"]))
    print(f"\n[patch14] tiny fp16 weight-only e4m3 vs its own fp32 model: {e:.3e}")
    assert np.isfinite(got).all() and np.array_equal(got, host_quantised)
    assert e <= MODEL_TOL[FP16], e


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_patch14_fixture_logits_match_the_golden_fp64_logits(path):
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    wseed, iseed, batch = [int(v) for v in g["meta"]]
    blob, images = S.make_blob(cfg, wseed), S.make_images(cfg, iseed, batch)
    for dt in DT:
        got, _ = _forward(cfg, blob, images, dt)
        e = rel(got, g["logits_f64"])
        print(f"\n[patch14] fixture {os.path.basename(path)} {NAME[dt]}: logits vs fp64 golden {e:.3e}")
        assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], e)


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_same_bits_across_batch_streams_and_graph_replay(dt):
    cfg = TINY_P14
    blob = _tiny()["blob"]
    images = S.make_images(cfg, 8, 7)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=7)
    ctx.load_weights(blob)
    one = ctx.forward(images[:1])
    seven = ctx.forward(images)
    assert np.isfinite(seven).all()
    assert np.array_equal(seven[:1], one)
    ctx.set_streams(2)
    assert np.array_equal(ctx.forward(images), seven)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert np.array_equal(ctx.forward(images), seven)
    ctx.set_graph(False)
    ctx.close()


# ---- real shapes ---------------------------------------------------------------------------------------------------------

def _per_image(cfg, n, dt=FP16):
    blob, images = O.make_blob(cfg, 0), S.make_images(cfg, 1, n)
    ref = O.vit_forward(cfg, blob, images)
    got, _ = _forward(cfg, blob, images, dt)
    assert np.isfinite(got).all()
    return got, ref, np.abs(got - ref).max(1) / np.abs(ref).max()


def test_vit_b14_224_fp16_on_8_images_inside_the_north_star_tolerance():
    _, _, per = _per_image(VIT_B14_224, 8)
    print(f"\n[patch14] ViT-B/14-224 fp16 b8: per-image {' '.join(f'{x:.2e}' for x in per)}")
    assert per.max() <= MODEL_TOL[FP16], per


def test_dinov2_s14_518_fp16_through_the_streaming_attention():
    _, _, per = _per_image(DINO_S14_518, 2)
    print(f"\n[patch14] DINOv2-S/14-518 shape fp16 b2 (1370 tokens): per-image {' '.join(f'{x:.2e}' for x in per)}")
    assert per.max() <= MODEL_TOL[FP16], per


def test_vit_l14_224_fp16():
    # what test_gpu_vit.test_vit_large_384_long_sequence_config asserts for ViT-L: finite, whole-batch metric inside 1e-3
    got, ref, per = _per_image(VIT_L14_224, 4)
    e = rel(got, ref)
    print(f"\n[patch14] ViT-L/14-224 fp16 b4: logits {e:.3e}, per-image {' '.join(f'{x:.2e}' for x in per)}")
    assert e <= MODEL_TOL[FP16], e
