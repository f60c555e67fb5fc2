"""Head dims other than 64 on the host: models whose head dim dim/heads is 32, 48, 80, 96, 112 or 128 (ViT-H/14 among them)
are valid shapes -- the forward runs them through the K/V-streaming attention kernel of kernels_attn_hd.hip -- and every other
head dim is still rejected.  No GPU needed: vh_weight_blob_bytes and vh_blob_file_config run check_config only, and the
vh_op_attention_hd tap checks its arguments before it touches a device.  The configurations are defined here, not in
vh_synth.CONFIGS (whose every entry other tests run on the GPU); the oracle is pinned on head dims 80 and 128 by
tests/golden/headdim/ (tests/golden/make_golden_headdim.py)."""
import glob
import os

import numpy as np
import pytest

import oracle_lib as O
import vh_synth as S
from vh_testlib import lib_blob_bytes, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "headdim", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8


def _cfg(image, patch, dim, heads, mlp, layers, classes=1000, channels=3):
    return dict(image_size=image, patch_size=patch, channels=channels, dim=dim, heads=heads, mlp_dim=mlp,
                layers=layers, classes=classes)


VIT_H14_224 = _cfg(224, 14, 1280, 16, 5120, 32)   # head dim 80, 257 tokens
# (name, config, head dim): one model per supported head dim other than 64
VALID = [("vit_h14_224", VIT_H14_224, 80),
         ("hd32_d256", _cfg(224, 16, 256, 8, 1024, 4), 32),
         ("hd32_d384", _cfg(224, 16, 384, 12, 1536, 4), 32),
         ("hd48_d384", _cfg(224, 16, 384, 8, 1536, 4), 48),
         ("hd80_d320", _cfg(64, 16, 320, 4, 640, 2, classes=40), 80),
         ("hd96_d768", _cfg(224, 16, 768, 8, 3072, 4), 96),
         ("hd112_d448", _cfg(224, 16, 448, 4, 1792, 4), 112),
         ("hd128_d256", _cfg(64, 16, 256, 2, 512, 2, classes=40), 128),
         ("hd128_d1024_512px", _cfg(512, 16, 1024, 8, 4096, 4), 128)]
HD80_MICRO = _cfg(64, 16, 320, 4, 640, 2, classes=40)      # the fixtures' models (make_golden_headdim.py)
HD128_MICRO = _cfg(64, 16, 256, 2, 512, 2, classes=40)


@pytest.mark.parametrize("name,cfg,hd", VALID, ids=[v[0] for v in VALID])
def test_models_with_other_head_dims_are_valid(name, cfg, hd):
    assert cfg["dim"] // cfg["heads"] == hd and cfg["dim"] % cfg["heads"] == 0 and hd != 64
    for dt in (BF16, FP16, FP8):
        if dt == FP8 and (cfg["dim"] % 128 or cfg["mlp_dim"] % 128):
            assert lib_blob_bytes(cfg, dtype=dt) == 0, (name, "fp8 keeps its multiples of 128")
            continue
        assert lib_blob_bytes(cfg, dtype=dt) == 64 + 4 * S.param_count(cfg), (name, dt)


def test_vit_h14_is_valid_in_every_dtype_and_its_blob_size():
    assert S.tokens(VIT_H14_224) == 257
    for dt in (BF16, FP16, FP8):
        assert lib_blob_bytes(VIT_H14_224, max_batch=128, dtype=dt) == 64 + 4 * S.param_count(VIT_H14_224)


@pytest.mark.parametrize("dim,heads", [(576, 8), (1408, 16), (256, 16), (576, 4), (768, 5), (640, 6), (1024, 3), (2048, 128)],
                         ids=["hd72", "hd88", "hd16", "hd144", "d768_h5", "d640_h6", "d1024_h3", "hd16_h128"])
def test_other_head_dims_are_rejected(dim, heads):
    cfg = _cfg(224, 16, dim, heads, 4 * dim, 2)
    for dt in (BF16, FP16):
        assert lib_blob_bytes(cfg, dtype=dt) == 0, (dim, heads)


def test_the_other_rules_still_hold_at_head_dim_80():
    assert lib_blob_bytes(_cfg(224, 16, 1280, 16, 5120, 2)) > 0
    assert lib_blob_bytes(_cfg(224, 16, 1360, 17, 5120, 2)) == 0                     # dim not a multiple of 64
    assert lib_blob_bytes(_cfg(224, 16, 320, 4, 640, 2), dtype=FP8) == 0              # fp8: dim a multiple of 128
    assert lib_blob_bytes(_cfg(224, 16, 2560, 32, 5120, 2)) == 0                     # dim > 2048
    assert lib_blob_bytes(_cfg(1040, 16, 1280, 16, 5120, 2)) == 0                    # 65 x 65 patches: > 4097 tokens


def test_vit_h14_blob_file_header_is_accepted_on_the_host(tmp_path):
    # a micro model's 64-byte header (magic, then the eight shape words as int32, then ln_eps) rewritten to ViT-H/14's
    # shape, in a sparse file of ViT-H/14's blob size (vh_blob_file_config reads the header and checks the size)
    hdr = S.make_blob(HD80_MICRO, 5)[:64].copy()
    words = hdr.view(np.int32)
    assert words[2:10].tolist() == [HD80_MICRO[k] for k in CFG_KEYS]
    words[2:10] = [VIT_H14_224[k] for k in CFG_KEYS]
    path = tmp_path / "vit_h14.vhblob"
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.truncate(64 + 4 * S.param_count(VIT_H14_224))
    got, eps = vithip.blob_file_config(path)
    assert got == VIT_H14_224 and abs(eps - 1e-6) < 1e-12


def test_head_dim_80_blob_file_is_accepted_on_the_host(tmp_path):
    blob = S.make_blob(HD80_MICRO, 5)
    assert blob.nbytes == 64 + 4 * S.param_count(HD80_MICRO)
    path = tmp_path / "hd80_micro.vhblob"
    blob.tofile(path)
    got, eps = vithip.blob_file_config(path)
    assert got == HD80_MICRO and abs(eps - 1e-6) < 1e-12


def test_attention_hd_tap_checks_its_arguments_on_the_host():
    # unsupported head dims, heads <= 0 or too wide, tokens outside 1..4097, null pointers, an unknown dtype: rejected before
    # anything reaches a device (the pointers are never dereferenced)
    op = vithip.op_attention_hd
    bad = [(1, 1, 197, 4, 72, 1, BF16), (1, 1, 197, 4, 88, 1, BF16), (1, 1, 197, 4, 16, 1, BF16), (1, 1, 197, 4, 144, 1, BF16),
           (1, 1, 197, 4, 0, 1, BF16), (1, 1, 197, 4, -80, 1, BF16),
           (1, 1, 197, 0, 80, 1, BF16), (1, 1, 197, -2, 80, 1, BF16), (1, 1, 197, 17, 128, 1, BF16),
           (1, 1, 0, 4, 80, 1, BF16), (1, 1, 4098, 4, 80, 1, BF16), (1, 1, -5, 4, 80, 1, BF16),
           (1, 0, 197, 4, 80, 1, BF16),
           (None, 1, 197, 4, 80, 1, BF16), (1, 1, 197, 4, 80, None, BF16),
           (1, 1, 197, 4, 80, 1, 3), (1, 1, 197, 4, 80, 1, -1), (1, 1, 197, 4, 80, 1, 100)]
    for args in bad:
        with pytest.raises(vithip.VhError):
            op(*args)


def test_headdim_fixtures_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["hd128_micro", "hd80_micro"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_oracle_matches_headdim_golden(path):
    # test_any_patch.test_oracle_matches_patch14_golden on the head-dim fixtures; the configuration is stored in the file
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    assert cfg in (HD80_MICRO, HD128_MICRO)
    wseed, iseed, batch = [int(v) for v in g["meta"]]
    tensors = S.make_tensors(cfg, wseed)
    cs = np.array([float(v.astype(np.float64).sum()) for v in tensors.values()][:8])
    assert np.allclose(cs, g["weights_checksum"], rtol=0, atol=1e-9)
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(g["images_checksum"][0])) < 1e-9
    blob = S.pack_blob(cfg, tensors)
    assert np.array_equal(blob, O.make_blob(cfg, wseed))
    n = len(g["hidden_last_f64"])
    logits, hidden = O.vit_forward(cfg, blob, images, want_hidden=True)
    assert rel(logits, g["logits_f64"]) <= 5e-6
    assert rel(hidden[:n], g["hidden_last_f64"]) <= 5e-6
    assert rel(g["logits_f32"], g["logits_f64"]) <= 5e-6
    _, emb = O.vit_forward(cfg, blob, images, n_layers=0, want_hidden=True)
    assert rel(emb[:n], g["embed_f64"]) <= 5e-6
    _, h1 = O.vit_forward(cfg, blob, images, n_layers=1, want_hidden=True)
    assert rel(h1[:n], g["hidden_l1_f64"]) <= 5e-6
