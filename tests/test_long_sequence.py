"""Long sequences on the host: token counts beyond the LDS-resident attention's 640 are valid model shapes up to 4097
(64 x 64 patches + the class token), with max_batch x tokens bounded by 640 x 2^20.  No GPU needed: vh_weight_blob_bytes
and vh_blob_file_config run check_config only.  The long-sequence configurations are defined here, not in vh_synth.CONFIGS
(whose every entry other tests run on the GPU)."""

import pytest

import vh_synth as S
from vh_testlib import lib_blob_bytes

vithip = pytest.importorskip("vithip")


def _cfg(image, patch, dim, heads, mlp, layers, classes=1000, channels=3):
    return dict(image_size=image, patch_size=patch, channels=channels, dim=dim, heads=heads, mlp_dim=mlp,
                layers=layers, classes=classes)


VIT_B16_448 = _cfg(448, 16, 768, 12, 3072, 12)     # 785 tokens
VIT_B16_512 = _cfg(512, 16, 768, 12, 3072, 12)     # 1025
VIT_B16_1024 = _cfg(1024, 16, 768, 12, 3072, 12)   # 4097
VIT_B8_224 = _cfg(224, 8, 768, 12, 3072, 12)       # 785
TINY_P8_256 = _cfg(256, 8, 128, 2, 256, 2, classes=40)   # 1025


@pytest.mark.parametrize("name,cfg,tokens", [("vit_b16_448", VIT_B16_448, 785), ("vit_b16_512", VIT_B16_512, 1025),
                                             ("vit_b16_1024", VIT_B16_1024, 4097), ("vit_b8_224", VIT_B8_224, 785),
                                             ("tiny_p8_256", TINY_P8_256, 1025)])
def test_long_sequence_models_are_valid(name, cfg, tokens):
    assert S.tokens(cfg) == tokens
    for dt in (vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8):
        assert lib_blob_bytes(cfg, dtype=dt) == 64 + 4 * S.param_count(cfg), (name, dt)


def test_more_than_4097_tokens_is_rejected():
    cfg = _cfg(1040, 16, 768, 12, 3072, 12)   # 65 x 65 patches: 4226 tokens
    assert S.tokens(cfg) == 4226
    assert lib_blob_bytes(cfg) == 0


def test_max_batch_times_tokens_is_bounded_by_640_x_2_20():
    vit_b16_384 = _cfg(384, 16, 768, 12, 3072, 12)   # 577 tokens: every max_batch up to 2^20 stays valid
    assert lib_blob_bytes(vit_b16_384, max_batch=1 << 20) == 64 + 4 * S.param_count(vit_b16_384)
    assert lib_blob_bytes(VIT_B16_512, max_batch=1 << 20) == 0   # 1025 x 2^20 > 640 x 2^20
    assert lib_blob_bytes(VIT_B16_512, max_batch=1 << 19) == 64 + 4 * S.param_count(VIT_B16_512)
    assert lib_blob_bytes(VIT_B16_1024, max_batch=(640 << 20) // 4097) > 0
    assert lib_blob_bytes(VIT_B16_1024, max_batch=(640 << 20) // 4097 + 1) == 0


def test_long_sequence_blob_file_header_is_accepted_on_the_host(tmp_path):
    blob = S.make_blob(TINY_P8_256, 5)
    path = tmp_path / "tiny_p8_256.vhblob"
    blob.tofile(path)
    got, eps = vithip.blob_file_config(path)
    assert got == TINY_P8_256 and abs(eps - 1e-6) < 1e-12
