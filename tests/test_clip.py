"""The two CLIP switches on the host: VH_FLAG_PRE_LN and VH_FLAG_QUICK_GELU are valid flags (alone, together, with every other
flag and dtype), the blob grows by pre_ln.weight / pre_ln.bias exactly when the first is set, the blob header carries both as
model bits, and the new taps and epilogue codes check their arguments before they touch a device.  The reference the GPU tests
use, tests/vit_ref.py, is pinned here: against three fixtures computed by Hugging Face `transformers` models
(tests/golden/make_golden_clip.py), and, with neither switch, against the C oracle.  No GPU needed."""
import functools
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as H
import oracle_lib as O
import vh_synth as S
import vit_ref as R
from vh_testlib import lib_blob_bytes, rel, vit_cfg

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "clip", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU
VH_ERR_INVALID, VH_ERR_UNSUPPORTED = 1, 4


# the vision towers of OpenAI CLIP and LAION / OpenCLIP; classes = the width of the image embedding
CLIP = [("vit_b32_224", vit_cfg(224, 32, 768, 12, 3072, 12, 512), 50),
        ("vit_b16_224", vit_cfg(224, 16, 768, 12, 3072, 12, 512), 197),
        ("vit_l14_224", vit_cfg(224, 14, 1024, 16, 4096, 24, 768), 257),
        ("vit_l14_336", vit_cfg(336, 14, 1024, 16, 4096, 24, 768), 577),
        ("vit_h14_224", vit_cfg(224, 14, 1280, 16, 5120, 32, 1024), 257)]
MICRO = S.CONFIGS["vit_micro"]


_blob_bytes = functools.partial(lib_blob_bytes, ln_eps=1e-5)      # CLIP's layer_norm_eps


def test_the_flag_and_epilogue_constants():
    assert (PRE, QUICK) == (16, 32) == (R.FLAG_PRE_LN, R.FLAG_QUICK_GELU)
    assert (vithip.EPI_BIAS_QGELU, vithip.EPI_LNFOLD_QGELU) == (10, 11)
    assert vithip.STAGES[-1] == "pre_layernorm" and vithip.STAGES.index("ln_stats") == 11
    assert vithip.lib().vh_stage_name(12) == b"pre_layernorm" and vithip.lib().vh_abi_version() == 1


@pytest.mark.parametrize("name,cfg,tokens", CLIP, ids=[c[0] for c in CLIP])
def test_clip_tower_blob_sizes_with_and_without_the_pre_layernorm(name, cfg, tokens):
    assert S.tokens(cfg) == tokens
    base = 64 + 4 * S.param_count(cfg)
    for dt in (BF16, FP16, FP8):
        assert _blob_bytes(cfg, 0, dt) == base
        assert _blob_bytes(cfg, QUICK, dt) == base                          # QuickGELU adds no tensor
        assert _blob_bytes(cfg, PRE, dt) == base + 8 * cfg["dim"]
        assert _blob_bytes(cfg, PRE | QUICK, dt, max_batch=256) == base + 8 * cfg["dim"] == R.blob_bytes(cfg, PRE | QUICK)


def test_the_flags_are_independent_and_combine_with_every_other_flag():
    cfg = CLIP[0][1]
    others = [0, vithip.FLAG_LN_FOLD_OFF, vithip.FLAG_LN_FOLD_ON, vithip.FLAG_W8_E4M3, vithip.FLAG_CLS_TAIL,
              vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL | vithip.FLAG_W8_E4M3]
    for mine in (PRE, QUICK, PRE | QUICK):
        for o in others:
            for dt in (BF16, FP16, FP8):
                want = 0 if (dt == FP8 and o & vithip.FLAG_W8_E4M3) else R.blob_bytes(cfg, mine)   # W8 stays a 16-bit flag
                assert _blob_bytes(cfg, mine | o, dt) == want, (mine, o, dt)


def test_unknown_flag_bits_and_the_other_rules_still_hold():
    cfg = CLIP[0][1]
    for bad in (64, 128, 1 << 20, PRE | 64, QUICK | 256, -1):
        assert _blob_bytes(cfg, bad) == 0, bad
    assert _blob_bytes(cfg, PRE | vithip.FLAG_LN_FOLD_OFF | vithip.FLAG_LN_FOLD_ON) == 0      # still exclude each other
    assert _blob_bytes(vit_cfg(224, 32, 576, 8, 2304, 2, 512), PRE | QUICK) == 0                   # head dim 72
    assert _blob_bytes(vit_cfg(224, 32, 320, 4, 640, 2, 512), PRE | QUICK, FP8) == 0               # fp8: multiples of 128


def test_layout_of_the_blob_with_the_pre_layernorm():
    names = [n for n, *_ in R.tensor_table(MICRO, PRE)]
    assert names[:6] == ["patch.weight", "patch.bias", "cls", "pos", "pre_ln.weight", "pre_ln.bias"] and names[6] == "l0.ln1.weight"
    assert [n for n, *_ in R.tensor_table(MICRO, QUICK)] == [n for n, *_ in S.tensor_table(MICRO)]
    t = R.make_tensors(MICRO, 9, PRE)
    # tensor ids 5 and 6, sigma and offset of the other LayerNorms
    assert np.array_equal(t["pre_ln.weight"], S.fill(MICRO["dim"], 9, 5, 1, 0.05, 1.0))
    assert np.array_equal(t["pre_ln.bias"], S.fill(MICRO["dim"], 9, 6, 1, 0.02, 0.0))
    # a model with neither flag: byte for byte today's blob
    assert np.array_equal(R.make_blob(MICRO, 9, 0), S.make_blob(MICRO, 9))
    b = R.make_blob(MICRO, 9, PRE | QUICK)
    assert b.nbytes == S.make_blob(MICRO, 9).nbytes + 8 * MICRO["dim"]
    assert b[52:56].view(np.uint32)[0] == 6 and R.make_blob(MICRO, 9, QUICK)[52:56].view(np.uint32)[0] == 4


def test_header_bits_round_trip_through_the_blob_file_entry_points(tmp_path):
    for flags in (0, PRE, QUICK, PRE | QUICK):
        blob = R.make_blob(MICRO, 5, flags, 1e-5)
        path = tmp_path / f"micro_{flags}.vhblob"
        blob.tofile(path)
        got, eps = vithip.blob_file_config(path)                # (cfg, eps): the return value existing callers unpack
        assert got == MICRO and abs(eps - 1e-5) < 1e-12
        assert vithip.blob_file_flags(path) == flags
        back = np.zeros(blob.nbytes, np.uint8)
        rc = vithip.lib().vh_blob_file_read(os.fsencode(path), back.ctypes.data, back.nbytes)
        assert rc == 0 and np.array_equal(back, blob)            # the memory form keeps the model bits
        # the file form: checksum present (bit 0) beside the model bits
        filed = blob.copy()
        h = 0xCBF29CE484222325
        for byte in filed[64:64 + 4096].tobytes():               # (short prefix only to build a WRONG sum cheaply below)
            h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        filed[52:56] = np.array([1 | (filed[52:56].view(np.uint32)[0])], np.uint32).view(np.uint8)
        filed[44:52] = np.array([h], np.uint64).view(np.uint8)
        filed.tofile(path)
        assert vithip.blob_file_flags(path) == flags            # header only
        rc = vithip.lib().vh_blob_file_read(os.fsencode(path), back.ctypes.data, back.nbytes)
        assert rc == VH_ERR_INVALID and b"checksum" in vithip.lib().vh_last_error(None)


def test_a_file_whose_bits_do_not_match_its_size_or_are_unknown_is_refused(tmp_path):
    path = tmp_path / "bad.vhblob"
    blob = R.make_blob(MICRO, 5, 0)
    blob[52:56] = np.array([2], np.uint32).view(np.uint8)        # claims a pre-LayerNorm, holds no such tensors
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    blob = R.make_blob(MICRO, 5, PRE)
    blob[52:56] = np.array([0], np.uint32).view(np.uint8)        # the tensors without the bit
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    blob = R.make_blob(MICRO, 5, QUICK)
    blob[52:56] = np.array([4 | 8], np.uint32).view(np.uint8)
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="unknown bits"):
        vithip.blob_file_flags(path)


# ---- the reference against independent implementations ----------------------------------------------------------------------------

def test_the_three_fixtures_are_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["clip_both", "clip_preln", "vit_quick"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_clip_ref_matches_the_hugging_face_fixtures(path):
    g = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in g["config"])))
    wseed, iseed, batch, flags = [int(v) for v in g["meta"]]
    eps = float(g["ln_eps"])
    assert abs(eps - 1e-5) < 1e-12 and os.path.getsize(path) < 200 * 1024
    tensors = H.make_clip_tensors(cfg, wseed, flags) if int(g["zero_bias"]) else R.make_tensors(cfg, wseed, flags)
    cs = np.array([float(v.astype(np.float64).sum()) for v in tensors.values()][:8])
    assert np.allclose(cs, g["weights_checksum"], rtol=0, atol=1e-9)
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(g["images_checksum"][0])) < 1e-9
    blob = R.pack_blob(cfg, tensors, flags, eps)
    n = len(g["hidden_last_f64"])
    # two float64 implementations: 1e-7 is below one fp32 rounding (6e-8 per operation), which is what a reference for an fp32 /
    # 16-bit forward has to resolve (measured: 1e-15 after the pre-LayerNorm, 1e-9 after two layers)
    F64 = 1e-7
    logits, hidden = R.forward(cfg, blob, images, flags, eps, want_hidden=True)
    assert rel(logits, g["logits_f64"]) <= F64 and rel(hidden[:n], g["hidden_last_f64"]) <= F64
    _, emb = R.forward(cfg, blob, images, flags, eps, n_layers=0, want_hidden=True)     # the rows AFTER the pre-LayerNorm
    assert rel(emb[:n], g["embed_f64"]) <= F64
    _, h1 = R.forward(cfg, blob, images, flags, eps, n_layers=1, want_hidden=True)
    assert rel(h1[:n], g["hidden_l1_f64"]) <= F64
    assert rel(R.forward(cfg, blob, images, flags, eps, dtype=np.float32), g["logits_f64"]) <= 5e-6
    assert rel(g["logits_f32"], g["logits_f64"]) <= 5e-6
    # each switch matters: without it the result is far from the fixture
    if flags & QUICK:   # ten times the fp32 agreement bound above: erf GELU in its place is a different model
        assert rel(R.forward(cfg, blob, images, flags & ~QUICK, eps), g["logits_f64"]) > 5e-5


def test_clip_ref_with_no_flag_is_the_oracle():
    blob, images = S.make_blob(MICRO, 11), S.make_images(MICRO, 12, 3)
    want, want_h = O.vit_forward(MICRO, blob, images, want_hidden=True)
    got, got_h = R.forward(MICRO, blob, images, 0, 1e-6, want_hidden=True)
    assert rel(got, want) <= 5e-6 and rel(got_h, want_h) <= 5e-6
    # and its emulation of the fp8 data flow is the oracle's, in both forms (vit_q8: dims multiples of 128)
    cfg = S.CONFIGS["vit_q8"]
    blob, images = S.make_blob(cfg, 11), S.make_images(cfg, 12, 2)
    ref32 = O.vit_forward(cfg, blob, images)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    for mine, theirs in (("plain", True), ("folded", "folded")):
        a, b = R.forward(cfg, blob, images, 0, 1e-6, fp8=mine), O.vit_forward(cfg, blob, images, fp8=theirs)
        # the same rounding points; a value on an e4m3 boundary falls either way (numpy and the oracle sum in different orders), so
        # the two emulations agree as two realisations of one quantisation noise: closer to each other than either is to fp32
        print(f"\n[clip] fp8 emulation {mine}: vit_ref vs oracle {rms(a, b):.3e}, oracle vs fp32 {rms(b, ref32):.3e}")
        assert rms(a, b) <= rms(b, ref32), (mine, rms(a, b), rms(b, ref32))
        assert abs(rms(a, ref32) - rms(b, ref32)) <= 0.25 * rms(b, ref32), mine


def test_quick_gelu_reference_over_the_whole_range():
    v = np.array([-1e30, -800.0, -30.0, -1.0, -0.0, 0.0, 1.0, 30.0, 800.0, 1e30])
    got = R.quick_gelu(v)
    assert np.isfinite(got).all() and got[0] == 0 and got[1] == 0 and got[-1] == 1e30
    assert abs(got[6] - 1.0 / (1.0 + np.exp(-1.702))) < 1e-15 and abs(got[3] + 1.0 / (1.0 + np.exp(1.702))) < 1e-15


# ---- the converter --------------------------------------------------------------------------------------------------------------

def _hf_clip(cfg, act):
    transformers = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    hc = transformers.CLIPVisionConfig(hidden_size=cfg["dim"], intermediate_size=cfg["mlp_dim"], projection_dim=cfg["classes"],
                                       num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], num_channels=3,
                                       image_size=cfg["image_size"], patch_size=cfg["patch_size"], hidden_act=act,
                                       layer_norm_eps=1e-5, attention_dropout=0.0)
    hc._attn_implementation = "eager"
    torch.manual_seed(7)
    m = transformers.CLIPVisionModelWithProjection(hc).eval()
    with torch.no_grad():   # the default initialisation leaves LayerNorms at (1, 0) and biases at 0: make every tensor count
        for p_ in m.parameters():
            p_.add_(0.02 * torch.randn_like(p_))
    return m, torch


@pytest.mark.parametrize("act,flags", [("quick_gelu", PRE | QUICK), ("gelu", PRE)], ids=["openai", "laion"])
def test_blob_from_clip_state_dict_reproduces_the_models_image_embeds(act, flags):
    cfg = vit_cfg(64, 16, 128, 2, 256, 2, 48)
    m, torch = _hf_clip(cfg, act)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    blob = vithip.blob_from_clip_state_dict(sd, dict(cfg, flags=flags))
    assert blob.nbytes == _blob_bytes(cfg, flags) and blob[52:56].view(np.uint32)[0] == (6 if flags & QUICK else 2)
    t = R.unpack_blob(cfg, blob, flags)
    assert not t["patch.bias"].any() and not t["head.bias"].any()
    images = S.make_images(cfg, 3, 2)
    with torch.no_grad():
        want = m(pixel_values=torch.from_numpy(images.transpose(0, 3, 1, 2).copy())).image_embeds.numpy()
    got = R.forward(cfg, blob, images, flags, 1e-5, dtype=np.float32)
    assert rel(got, want) <= 5e-6, rel(got, want)


def test_blob_from_clip_state_dict_refuses_by_name():
    cfg = vit_cfg(64, 16, 128, 2, 256, 1, 48)
    D, M = 128, 256
    sd = {"vision_model.embeddings.patch_embedding.weight": np.zeros((D, 3, 16, 16), np.float32),
          "vision_model.embeddings.class_embedding": np.zeros(D, np.float32),
          "vision_model.embeddings.position_embedding.weight": np.zeros((17, D), np.float32),
          "vision_model.pre_layrnorm.weight": np.ones(D, np.float32), "vision_model.pre_layrnorm.bias": np.zeros(D, np.float32),
          "vision_model.post_layernorm.weight": np.ones(D, np.float32), "vision_model.post_layernorm.bias": np.zeros(D, np.float32),
          "visual_projection.weight": np.zeros((48, D), np.float32)}
    b = "vision_model.encoder.layers.0."
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        sd[f"{b}self_attn.{n}.weight"], sd[f"{b}self_attn.{n}.bias"] = np.zeros((D, D), np.float32), np.zeros(D, np.float32)
    for n in ("layer_norm1", "layer_norm2"):
        sd[f"{b}{n}.weight"], sd[f"{b}{n}.bias"] = np.ones(D, np.float32), np.zeros(D, np.float32)
    sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = np.zeros((M, D), np.float32), np.zeros(M, np.float32)
    sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = np.zeros((D, M), np.float32), np.zeros(D, np.float32)
    full = dict(cfg, flags=PRE | QUICK)
    assert vithip.blob_from_clip_state_dict(sd, full).nbytes == _blob_bytes(cfg, PRE)
    missing = dict(sd)
    del missing["vision_model.pre_layrnorm.bias"]
    with pytest.raises(KeyError, match="vision_model.pre_layrnorm.bias"):
        vithip.blob_from_clip_state_dict(missing, full)
    wrong = dict(sd)
    wrong[b + "mlp.fc1.weight"] = np.zeros((D, M), np.float32)
    with pytest.raises(ValueError, match="mlp.fc1.weight"):
        vithip.blob_from_clip_state_dict(wrong, full)
    with pytest.raises(ValueError, match="FLAG_PRE_LN"):
        vithip.blob_from_clip_state_dict(sd, dict(cfg, flags=QUICK))


# ---- taps and epilogue codes check their arguments before they touch a device ---------------------------------------------------

def _code(fn, *args):
    with pytest.raises(vithip.VhError) as e:
        fn(*args)
    return e.value.code


def test_pre_layernorm_tap_checks_its_arguments_on_the_host():
    op = vithip.op_pre_layernorm     # (x, rows, dim, gamma, beta, eps, y32, hi, lo, stats, dtype); pointers are never dereferenced
    bad = [(None, 4, 128, 1, 1, 1e-5, 1, 1, 1, 1, BF16), (1, 4, 128, None, 1, 1e-5, 1, 1, 1, 1, BF16),
           (1, 4, 128, 1, None, 1e-5, 1, 1, 1, 1, BF16),
           (1, 4, 128, 1, 1, 1e-5, None, None, None, 1, BF16),       # no output at all
           (1, 4, 128, 1, 1, 1e-5, 1, None, 1, 1, BF16),             # a lo plane without its hi plane
           (1, 0, 128, 1, 1, 1e-5, 1, 1, 1, 1, BF16), (1, -3, 128, 1, 1, 1e-5, 1, 1, 1, 1, BF16),
           (1, 4, 0, 1, 1, 1e-5, 1, 1, 1, 1, BF16), (1, 4, 130, 1, 1, 1e-5, 1, 1, 1, 1, BF16), (1, 4, 2052, 1, 1, 1e-5, 1, 1, 1, 1, BF16),
           (1, 4, 128, 1, 1, 0.0, 1, 1, 1, 1, BF16), (1, 4, 128, 1, 1, -1.0, 1, 1, 1, 1, BF16),
           (1, 4, 128, 1, 1, 1e-5, 1, 1, 1, 1, 3), (1, 4, 128, 1, 1, 1e-5, 1, 1, 1, 1, -1), (1, 4, 128, 1, 1, 1e-5, 1, 1, 1, 1, 100)]
    for args in bad:
        assert _code(op, *args) == VH_ERR_INVALID, args


def test_the_new_epilogue_codes_check_their_arguments_on_the_host():
    for epi in (vithip.EPI_BIAS_QGELU, vithip.EPI_LNFOLD_QGELU):
        # (a, w, bias, out, M, N, K, epilogue, dtype): K % 64, N % 4, empty shapes, null pointers, unknown dtype
        for args in ((1, 1, 1, 1, 256, 256, 100, epi, BF16), (1, 1, 1, 1, 256, 258, 128, epi, BF16), (1, 1, 1, 1, 0, 256, 128, epi, BF16),
                     (None, 1, 1, 1, 256, 256, 128, epi, BF16), (1, 1, 1, None, 256, 256, 128, epi, BF16), (1, 1, 1, 1, 256, 256, 128, epi, 7)):
            assert _code(vithip.op_gemm, *args) == VH_ERR_INVALID, args
    # LNFOLD_QGELU needs the statistics and c, like LNFOLD_GELU
    assert _code(vithip.op_gemm, 1, 1, 1, 1, 256, 256, 128, vithip.EPI_LNFOLD_QGELU, BF16) == VH_ERR_INVALID
    assert _code(vithip.op_gemm, 1, 1, 1, 1, 256, 256, 128, 12, BF16) == VH_ERR_INVALID          # the next code is unknown
    # fp8 taps: the plain tap takes BIAS_QGELU and refuses the fold form as it refuses LNFOLD_GELU; the _ex tap the other way round
    f8, f8x = vithip.op_gemm_fp8, vithip.op_gemm_fp8_ex
    assert _code(f8, 1, 1, 1, 1, 1, 256, 256, 100, vithip.EPI_BIAS_QGELU) == VH_ERR_INVALID      # K % 128
    assert _code(f8, None, 1, 1, 1, 1, 256, 256, 128, vithip.EPI_BIAS_QGELU) == VH_ERR_INVALID
    assert _code(f8, 1, 1, 1, 1, 1, 256, 256, 128, vithip.EPI_LNFOLD_QGELU) == VH_ERR_UNSUPPORTED
    assert _code(f8x, 1, 1, 1, 1, 1, 256, 256, 128, vithip.EPI_BIAS_QGELU) == VH_ERR_UNSUPPORTED
    assert _code(f8x, 1, 1, 1, 1, 1, 256, 256, 128, vithip.EPI_LNFOLD_QGELU) == VH_ERR_INVALID   # no c / stats
    assert _code(f8x, 1, 1, 1, 1, 1, 256, 260, 128, vithip.EPI_LNFOLD_QGELU, 1, 1) == VH_ERR_INVALID   # N % 256


def test_the_e4m3_row_limit_is_checked_where_the_forward_launches():
    """gemm_check is what launch_gemm asks first, so the limits the e4m3 taps state hold for every caller: M above 0x7fffffff / 2 is
    refused through the layout tap with the reason, the limit itself passes the check (and is refused for its tile range only)."""
    f8l = vithip.op_gemm_fp8_layout      # (a8, w8, scale, bias, out, M, N, K, epilogue, ...); pointers are never dereferenced
    limit = 0x7FFFFFFF // 2
    with pytest.raises(vithip.VhError) as e:
        f8l(1, 1, 1, 1, 1, limit + 1, 256, 256, vithip.EPI_BIAS, variant=5, tile_count=1)
    assert e.value.code == VH_ERR_INVALID and "gemm_fp8_layout: M too large" in str(e.value)
    with pytest.raises(vithip.VhError) as e:
        f8l(1, 1, 1, 1, 1, limit, 256, 256, vithip.EPI_BIAS, variant=5, tile_begin=limit, tile_count=5)
    assert e.value.code == VH_ERR_INVALID and "tile range beyond the 4194304 tiles" in str(e.value)
