"""Any patch size on the host: models whose patch vector patch^2 * channels is not a multiple of 64 (or whose patch row
patch * channels is not a multiple of 4) are valid shapes -- the patch GEMM runs on the patch vector zero-padded to a multiple
of 64, and the blob keeps its size.  No GPU needed: vh_weight_blob_bytes and vh_blob_file_config run check_config only.  The
patch-14 configurations are defined here, not in vh_synth.CONFIGS (whose every entry other tests run on the GPU); the oracle
is pinned on a patch-14 model by tests/golden/patch14/ (tests/golden/make_golden_patch14.py)."""
import glob
import os

import numpy as np
import pytest

import oracle_lib as O
import vh_synth as S
from vh_testlib import lib_blob_bytes, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "patch14", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")


def _cfg(image, patch, dim, heads, mlp, layers, classes=1000, channels=3):
    return dict(image_size=image, patch_size=patch, channels=channels, dim=dim, heads=heads, mlp_dim=mlp,
                layers=layers, classes=classes)


VIT_L14_224 = _cfg(224, 14, 1024, 16, 4096, 24)   # 257 tokens, patch vector 588
VIT_B14_224 = _cfg(224, 14, 768, 12, 3072, 12)    # 257
DINO_S14_518 = _cfg(518, 14, 384, 6, 1536, 12)    # 1370 tokens
DINO_B14_518 = _cfg(518, 14, 768, 12, 3072, 12)   # 1370
GRAY_P14 = _cfg(112, 14, 128, 2, 256, 2, classes=40, channels=1)   # patch vector 196, patch row 14
TINY_P7 = _cfg(56, 7, 128, 2, 256, 2, classes=40)                   # patch vector 147, patch row 21
PATCH14_MICRO = _cfg(56, 14, 128, 2, 256, 2, classes=40)            # the fixture's model (make_golden_patch14.py)


@pytest.mark.parametrize("name,cfg,tokens", [("vit_l14_224", VIT_L14_224, 257), ("vit_b14_224", VIT_B14_224, 257),
                                             ("dinov2_s14_518", DINO_S14_518, 1370), ("dinov2_b14_518", DINO_B14_518, 1370),
                                             ("gray_p14", GRAY_P14, 65), ("tiny_p7", TINY_P7, 65)])
def test_any_patch_models_are_valid(name, cfg, tokens):
    assert S.tokens(cfg) == tokens
    kp = cfg["patch_size"] ** 2 * cfg["channels"]
    assert kp % 64 or (cfg["patch_size"] * cfg["channels"]) % 4   # shapes the patch-alignment rules rejected
    for dt in (vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8):
        assert lib_blob_bytes(cfg, dtype=dt) == 64 + 4 * S.param_count(cfg), (name, dt)


def test_patch14_blob_file_header_is_accepted_on_the_host(tmp_path):
    blob = S.make_blob(PATCH14_MICRO, 5)
    assert blob.nbytes == 64 + 4 * S.param_count(PATCH14_MICRO)
    path = tmp_path / "patch14_micro.vhblob"
    blob.tofile(path)
    got, eps = vithip.blob_file_config(path)
    assert got == PATCH14_MICRO and abs(eps - 1e-6) < 1e-12


def test_image_not_a_multiple_of_the_patch_is_still_rejected():
    assert lib_blob_bytes(_cfg(225, 14, 768, 12, 3072, 12)) == 0
    assert lib_blob_bytes(_cfg(224, 15, 768, 12, 3072, 12)) == 0


def test_more_than_4097_tokens_is_still_rejected_at_patch_14():
    cfg = _cfg(924, 14, 384, 6, 1536, 12)   # 66 x 66 patches: 4357 tokens
    assert S.tokens(cfg) == 4357
    assert lib_blob_bytes(cfg) == 0
    assert lib_blob_bytes(_cfg(896, 14, 384, 6, 1536, 12)) == 64 + 4 * S.param_count(_cfg(896, 14, 384, 6, 1536, 12))   # 64 x 64


def test_patch14_fixture_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["patch14_micro"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_oracle_matches_patch14_golden(path):
    # test_oracle_golden.test_oracle_matches_golden on the patch-14 fixture; its configuration is stored in the file
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    assert cfg == PATCH14_MICRO
    wseed, iseed, batch = [int(v) for v in g["meta"]]
    tensors = S.make_tensors(cfg, wseed)
    cs = np.array([float(v.astype(np.float64).sum()) for v in tensors.values()][:8])
    assert np.allclose(cs, g["weights_checksum"], rtol=0, atol=1e-9)
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(g["images_checksum"][0])) < 1e-9
    blob = S.pack_blob(cfg, tensors)
    assert np.array_equal(blob, O.make_blob(cfg, wseed))
    logits, hidden = O.vit_forward(cfg, blob, images, want_hidden=True)
    assert rel(logits, g["logits_f64"]) <= 5e-6
    assert rel(hidden[:64], g["hidden_last_f64"]) <= 5e-6
    assert rel(g["logits_f32"], g["logits_f64"]) <= 5e-6
    _, emb = O.vit_forward(cfg, blob, images, n_layers=0, want_hidden=True)
    assert rel(emb[:64], g["embed_f64"]) <= 5e-6
    _, h1 = O.vit_forward(cfg, blob, images, n_layers=1, want_hidden=True)
    assert rel(h1[:64], g["hidden_l1_f64"]) <= 5e-6


def test_im2col_padded_tap_checks_its_arguments_on_the_host():
    # kpad below the patch vector, kpad not a multiple of 8, an image that is not a multiple of the patch, an 8-bit dtype:
    # rejected before anything reaches a device (the pointers are never dereferenced)
    bf16 = vithip.DTYPE_BF16
    for args in ((1, 2, 56, 14, 3, 584, 1, bf16), (1, 2, 56, 14, 3, 596, 1, bf16), (1, 2, 57, 14, 3, 640, 1, bf16),
                 (1, 2, 56, 14, 3, 640, 1, vithip.DTYPE_FP8), (1, 0, 56, 14, 3, 640, 1, bf16), (None, 2, 56, 14, 3, 640, 1, bf16)):
        with pytest.raises(vithip.VhError):
            vithip.op_im2col_padded(*args)
