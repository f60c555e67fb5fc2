"""SigLIP's two switches on the host: VH_FLAG_TANH_GELU and VH_FLAG_MAP_HEAD are valid settings in the combinations the contract names,
the blob gains the eleven map.* tensors behind head.bias, the header carries both bits, every refusal has its message, and the
converter gives the reference's bytes.  The reference the GPU tests use, tests/vit_ref.py, is pinned here on these two flags: against three fixtures
computed by Hugging Face `transformers` (SiglipVisionModel twice, SiglipForImageClassification; tests/golden/make_golden_siglip.py);
its folded head against the literal multihead attention with K and V of every token; its blob sizes against the library.  The bound
of the GPU kernel test (tests/test_gpu_siglip.py MAP_BOUND) is measured here from a float32 statement of the function.  No GPU needed."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import features_ref as FR
import hf_state_dicts as HF
import vh_synth as S
import vit_ref as R
from vh_testlib import blob_digest, lib_blob_bytes, recorded_blob_digest

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "siglip", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK, REG, NO_CLS, POOL = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU, vithip.FLAG_REGISTERS, vithip.FLAG_NO_CLS, vithip.FLAG_POOL
MAP, TANH = vithip.FLAG_MAP_HEAD, vithip.FLAG_TANH_GELU
VH_ERR_INVALID = 1
MICRO = S.CONFIGS["vit_micro"]
MID = dict(image_size=64, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=3, classes=40)   # folds; eligible for fp8
# every legal combination of the two flags with the model bits they meet
LEGAL = [TANH, TANH | PRE, TANH | REG(4), TANH | POOL(vithip.POOL_CLS_AVG), TANH | NO_CLS | POOL(vithip.POOL_AVG_NORM),
         TANH | NO_CLS | POOL(vithip.POOL_AVG_FCNORM) | REG(2), MAP | NO_CLS, MAP | NO_CLS | TANH, MAP | NO_CLS | QUICK, MAP | NO_CLS | PRE,
         MAP | NO_CLS | TANH | PRE]
# The GPU kernel test's bound per class of inputs (tests/hf_state_dicts.py map_pool_inputs): 4 x the largest error of the float32
# statement map_z32 against float64 over the kernel test's own inputs, as max |z32 - z64| / max |z64| of a case.  The factor covers
# the summation order and the 1-ulp exp2 / rcp.  Measured by test_the_gpu_bound_is_four_times_the_float32_statements_error:
#   random 3.63e-6, ascending 9.87e-7, descending 1.04e-6, gap 2.10e-4 (scores near 1000: their fp32 rounding, 6e-5 apiece, is the
#   relative error of the softmax's numerators)
MAP_BOUND = {"random": 1.5e-5, "ascending": 4.0e-6, "descending": 4.2e-6, "gap": 8.5e-4}


def _create_error(cfg, flags=0, dtype=BF16, max_batch=1):
    c = vithip.make_config(cfg, dtype, max_batch, 1e-6, flags)
    h = C.c_void_p()
    rc = vithip.lib().vh_create(C.byref(c), 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, vithip.lib().vh_last_error(None).decode()


def test_the_macro_values():
    assert MAP == 1 << 19 == R.FLAG_MAP_HEAD and TANH == 1 << 21 == R.FLAG_TANH_GELU
    assert (vithip.EPILOGUE_BIAS_TGELU, vithip.EPILOGUE_LNFOLD_TGELU) == (13, 14) and vithip.MAP_MAX_HEADS == 16 == R.MAX_HEADS
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("#define VH_FLAG_MAP_HEAD (1 << 19)", "#define VH_FLAG_TANH_GELU (1 << 21)", "#define VH_EPI_BIAS_TGELU 13",
                 "#define VH_EPI_LNFOLD_TGELU 14", "#define VH_MAP_MAX_HEADS 16", "#define VH_ABI_VERSION 1", "int vh_op_map_pool("):
        assert text in hdr, text
    assert "vh_op_map_pool" in vithip.SYMBOLS
    assert vithip.lib().vh_abi_version() == 1


def test_blob_bytes_of_every_legal_combination():
    for cfg in (MICRO, MID, dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=768)):
        D, M, H = cfg["dim"], cfg["mlp_dim"], cfg["heads"]
        extra = 4 * (H * D + 2 * (D * D + D) + 2 * D + (M * D + M) + (D * M + D))
        for flags in LEGAL:
            for more in (0, vithip.FLAG_W8_E4M3, vithip.FLAG_LN_FOLD_ON, vithip.FLAG_LN_FOLD_OFF):
                assert R.legal(cfg, flags), flags
                want = R.blob_bytes(cfg, flags & ~(MAP | TANH)) + (extra if flags & MAP else 0)
                assert lib_blob_bytes(cfg, flags | more) == want == R.blob_bytes(cfg, flags), (flags, more)
    # neither flag: the blob is byte for byte what it was (the digest recorded before the flags' module was merged into vit_ref)
    assert blob_digest(R.make_blob(MICRO, 5, 0)) == recorded_blob_digest("vit_micro", 5, 0) and R.blob_bytes(MICRO, 0) == 64 + 4 * S.param_count(MICRO)
    # fp8 contexts take both
    assert lib_blob_bytes(MID, MAP | NO_CLS | TANH, dtype=FP8) == R.blob_bytes(MID, MAP | NO_CLS | TANH)


def test_layout_of_the_blob():
    flags = MAP | NO_CLS | TANH
    names = [n for n, *_ in R.tensor_table(MICRO, flags)]
    assert names[-13:] == ["head.weight", "head.bias", "map.qk", "map.v.weight", "map.v.bias", "map.o.weight", "map.o.bias", "map.ln.weight",
                           "map.ln.bias", "map.fc1.weight", "map.fc1.bias", "map.fc2.weight", "map.fc2.bias"]
    # no existing offset moves: the MAP blob starts with the bytes of the same model without the head
    base = NO_CLS | POOL(vithip.POOL_AVG_NORM)
    with_map, without = R.make_blob(MICRO, 9, flags), R.make_blob(MICRO, 9, base)
    assert np.array_equal(with_map[64:without.nbytes], without[64:])
    t = R.make_tensors(MICRO, 9, flags)
    assert t["map.qk"].shape == (MICRO["heads"], MICRO["dim"]) and t["map.fc1.weight"].shape == (MICRO["mlp_dim"], MICRO["dim"])
    assert abs(float(t["map.ln.weight"].mean()) - 1.0) < 0.05
    assert with_map[52:56].view(np.uint32)[0] == (1 << 15) | (1 << 19) | (1 << 21)
    assert R.make_blob(MICRO, 9, TANH | PRE)[52:56].view(np.uint32)[0] == 2 | (1 << 21)


def test_refusals_each_with_its_message():
    avg = POOL(vithip.POOL_AVG_NORM)
    heads32 = dict(MID, dim=1024, heads=32, mlp_dim=1024)
    for cfg, f, text in ((MICRO, TANH | QUICK, "VH_FLAG_TANH_GELU and VH_FLAG_QUICK_GELU exclude each other"),
                         (MICRO, MAP, "VH_FLAG_MAP_HEAD needs VH_FLAG_NO_CLS"),
                         (MICRO, MAP | avg, "VH_FLAG_MAP_HEAD needs VH_FLAG_NO_CLS"),
                         (MICRO, MAP | NO_CLS | avg, "VH_FLAG_MAP_HEAD excludes VH_FLAG_POOL"),
                         (MICRO, MAP | NO_CLS | POOL(vithip.POOL_CLS_AVG), "VH_FLAG_MAP_HEAD excludes VH_FLAG_POOL"),
                         (MICRO, MAP | NO_CLS | REG(4), "VH_FLAG_MAP_HEAD excludes VH_FLAG_REGISTERS"),
                         (MICRO, MAP | NO_CLS | vithip.FLAG_CLS_TAIL, "VH_FLAG_MAP_HEAD excludes VH_FLAG_CLS_TAIL"),
                         (heads32, MAP | NO_CLS, "VH_FLAG_MAP_HEAD takes at most 16 heads"),
                         (MICRO, NO_CLS, "VH_POOL_CLS reads the class token"),                       # as before, without MAP_HEAD
                         (MICRO, NO_CLS | TANH, "VH_POOL_CLS reads the class token")):
        assert not R.legal(cfg, f), f
        assert lib_blob_bytes(cfg, f) == 0, f
        rc, msg = _create_error(cfg, f)
        assert rc == VH_ERR_INVALID and text in msg, (f, msg)
    assert lib_blob_bytes(heads32, NO_CLS | avg | TANH) > 0          # 32 heads are fine without the MAP head
    # the pinned unknown bits stay unknown, alone and beside the new flags
    for bad in (64, 128, 256, 1 << 14, 1 << 18, 1 << 20, 1 << 22, TANH | (1 << 20), MAP | NO_CLS | (1 << 18)):
        assert lib_blob_bytes(MICRO, bad) == 0, bad
        assert "unknown bits in flags" in _create_error(MICRO, bad)[1]


def test_header_bits_round_trip_through_the_blob_file_entry_points(tmp_path):
    for flags in LEGAL:
        blob = R.make_blob(MICRO, 5, flags, 1e-5)
        path = tmp_path / f"micro_{flags}.vhblob"
        blob.tofile(path)
        got, eps = vithip.blob_file_config(path)
        assert got == MICRO and abs(eps - 1e-5) < 1e-12
        assert vithip.blob_file_flags(path) == flags == vithip.blob_flags_of(blob)
        back = np.zeros(blob.nbytes, np.uint8)
        assert vithip.lib().vh_blob_file_read(os.fsencode(path), back.ctypes.data, back.nbytes) == 0 and np.array_equal(back, blob)


def test_forged_header_bits_are_refused(tmp_path):
    path = tmp_path / "bad.vhblob"

    def with_bits(blob, bits):
        out = blob.copy()
        out[52:56] = np.array([bits], np.uint32).view(np.uint8)
        out.tofile(path)
        return out

    plain = R.make_blob(MICRO, 5, NO_CLS | POOL(vithip.POOL_AVG_NORM))
    with_bits(plain, NO_CLS | MAP)                         # the MAP bit over a blob without the eleven tensors: the length gives it away
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    with_bits(plain, MAP)                                  # an illegal combination in a header
    with pytest.raises(vithip.VhError, match="VH_FLAG_MAP_HEAD needs VH_FLAG_NO_CLS"):
        vithip.blob_file_config(path)
    with_bits(plain, NO_CLS | POOL(vithip.POOL_AVG_NORM) | TANH | 4)
    with pytest.raises(vithip.VhError, match="exclude each other"):
        vithip.blob_file_config(path)
    for unknown in (8, 1 << 18, 1 << 20, 1 << 22):         # header bit 3 and the neighbours of the new bits are still unknown
        with_bits(plain, NO_CLS | POOL(vithip.POOL_AVG_NORM) | unknown)
        with pytest.raises(vithip.VhError, match="unknown bits in the header"):
            vithip.blob_file_config(path)
    # a tanh blob and an erf blob have the same size: only the header tells them apart, and the file entry points report the bit
    erf, tanh = R.make_blob(MICRO, 5, 0), R.make_blob(MICRO, 5, TANH)
    assert erf.nbytes == tanh.nbytes and np.array_equal(erf[64:], tanh[64:]) and not np.array_equal(erf[:64], tanh[:64])
    with_bits(erf, 1 << 21)
    assert vithip.blob_file_flags(path) == TANH


def load_fixture(path):
    z = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in z["config"])))
    wseed, iseed, batch, flags, classifier = (int(v) for v in z["meta"])
    return z, cfg, wseed, iseed, batch, flags, bool(classifier), float(z["ln_eps"])


def fixture_blob(cfg, wseed, classifier, eps, prefix=""):
    t, raw, flags = HF.siglip_tensors(cfg, wseed, classifier)
    return vithip.blob_from_siglip_state_dict(HF.siglip_state_dict(cfg, t, raw, classifier, prefix), cfg, eps), flags


def test_fixtures_are_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["cls_a", "vision_a", "vision_b"], GOLDEN
    assert all(os.path.getsize(p) < 200 * 1024 for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p).split("_s")[0] for p in GOLDEN])
def test_siglip_ref_reproduces_the_transformers_fixture(path):
    """pooler_output / the logits and last_hidden_state of the transformers model (float64) against vit_ref in float64, the blob
    made by the converter (its fold included).  The bound 1e-5 is tests/test_pool.py's for the same comparison: the fp32 rounding of
    the weights -- and here of the folded map.qk."""
    z, cfg, wseed, iseed, batch, flags, classifier, eps = load_fixture(path)
    blob, made = fixture_blob(cfg, wseed, classifier, eps)
    assert made == flags == vithip.blob_flags_of(blob) and blob.nbytes == R.blob_bytes(cfg, flags) == lib_blob_bytes(cfg, flags)
    assert bool(flags & MAP) != classifier and flags & TANH and flags & NO_CLS
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(z["images_checksum"][0])) < 1e-9
    out, x = R.forward(cfg, blob, images, flags, eps, np.float64, want_hidden=True)
    t = R.unpack_blob(cfg, blob, flags)
    last = R.layernorm(x, t["lnf.weight"].astype(np.float64), t["lnf.bias"].astype(np.float64), eps)
    for name, got, want in (("last_hidden_state", last.reshape(z["last_hidden_state"].shape), z["last_hidden_state"]), ("output", out, z["output"])):
        e = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"\n[siglip] {os.path.basename(path)} {name}: {e:.3e}")
        assert got.shape == want.shape and e <= 1e-5, (name, e)
    # the erf activation misses that bound: the fixture pins tanh GELU
    if classifier:
        erf_blob = blob.copy()
        erf_blob[52:56] = np.array([flags & ~TANH], np.uint32).view(np.uint8)
        wrong = R.forward(cfg, erf_blob, images, flags & ~TANH, eps, np.float64)
        assert float(np.abs(wrong - z["output"]).max() / np.abs(z["output"]).max()) > 2e-5


def test_the_folded_head_is_the_literal_multihead_attention():
    """The fold itself, float64 at 1e-10 relative: scores through qk instead of K of every token (the key bias drops out of the softmax),
    V of the weighted row instead of the weighted V of every token (the weights sum to 1)."""
    rng = np.random.default_rng(3)
    for D, H, NP, batch in ((128, 2, 16, 3), (256, 4, 25, 2), (192, 12, 7, 2), (64, 1, 1, 1)):
        y = rng.standard_normal((batch, NP, D)) * 1.3 + 0.2
        probe = rng.standard_normal(D) * 0.5
        in_w, in_b = rng.standard_normal((3 * D, D)) * 0.06, rng.standard_normal(3 * D) * 0.8      # large biases: the key bias must cancel
        out_w, out_b = rng.standard_normal((D, D)) * 0.06, rng.standard_normal(D) * 0.1
        want = R.literal_map(y, probe, in_w, in_b, out_w, out_b, H)
        qk = R.fold_qk(probe, in_w[:D], in_b[:D], in_w[D:2 * D], H)
        z = R.map_z(y, qk)
        a = np.einsum("bhk,hjk->bhj", z, in_w[2 * D:].reshape(H, D // H, D)).reshape(batch, D) + in_b[2 * D:]
        got = a @ out_w.T + out_b
        e = float(np.abs(got - want).max() / np.abs(want).max())
        assert e <= 1e-10, (D, H, NP, e)
        # and it is the key bias that is dropped: with it in the fold's place the scores of a head shift by one constant
        s_lit = np.einsum("hj,bthj->bht", (in_w[:D] @ probe + in_b[:D]).reshape(H, D // H),
                          (y @ in_w[D:2 * D].T + in_b[D:2 * D]).reshape(batch, NP, H, D // H)) / np.sqrt(D // H)
        shift = s_lit - np.einsum("btk,hk->bht", y, qk)
        assert np.abs(shift - shift[:, :, :1]).max() <= 1e-10 * np.abs(s_lit).max()


def test_converter_gives_pack_blobs_bytes_and_refuses():
    A = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=256)
    for classifier, cfg in ((False, A), (True, dict(A, classes=8))):
        t, raw, flags = HF.siglip_tensors(cfg, 7, classifier)
        want = R.pack_blob(cfg, HF.fixture_blob_tensors(cfg, t, raw, flags), flags, 1e-6)
        for prefix in ("", "vision_model."):
            sd = HF.siglip_state_dict(cfg, t, raw, classifier, prefix)
            assert np.array_equal(vithip.blob_from_siglip_state_dict(sd, cfg, 1e-6), want), (classifier, prefix)
    sd = HF.siglip_state_dict(A, *HF.siglip_tensors(A, 7, False)[:2], False)
    conv = vithip.blob_from_siglip_state_dict
    assert vithip.blob_flags_of(conv(sd, A, hidden_act="gelu")) == NO_CLS | MAP
    assert vithip.blob_flags_of(conv(sd, A, hidden_act="quick_gelu")) == NO_CLS | MAP | QUICK
    with pytest.raises(ValueError, match="hidden_act"):
        conv(sd, A, hidden_act="relu")
    with pytest.raises(ValueError, match="must equal cfg\\['dim'\\]"):
        conv(sd, dict(A, classes=8))
    with pytest.raises(KeyError, match="head.probe"):
        conv({k: v for k, v in sd.items() if k != "head.probe"}, A)
    with pytest.raises(ValueError, match="in_proj_weight has shape"):
        conv(dict(sd, **{"head.attention.in_proj_weight": np.zeros((2 * 256, 256), np.float32)}), A)
    with pytest.raises(ValueError, match="25"):
        conv(dict(sd, **{"embeddings.position_embedding.weight": np.zeros((36, 256), np.float32)}), A)
    with pytest.raises(ValueError, match="at most 16 heads"):
        conv(sd, dict(A, heads=32))


def test_op_map_pool_refusals():
    ok = dict(hi_ptr=4096, lo_ptr=8192, form=BF16, batch=2, tokens=9, lead=1, dim=64, gamma_ptr=4096, beta_ptr=4096, eps=1e-6,
              qk_ptr=4096, heads=4, z_ptr=4096)
    cases = [(dict(hi_ptr=None), "null input"), (dict(form=7), "form must be"), (dict(form=-1), "fp32 rows take no lo plane"),
             (dict(lo_ptr=None), "split planes need the lo plane"), (dict(batch=0), "batch outside"), (dict(batch=(1 << 20) + 1), "batch outside"),
             (dict(tokens=0, lead=0), "tokens below 1"), (dict(tokens=4098), "tokens above 4097"), (dict(lead=-1), "lead rows outside 0 .. tokens - 1"),
             (dict(lead=9), "lead rows outside 0 .. tokens - 1"), (dict(dim=56), "dim below 64"), (dict(dim=2056), "dim above 2048"),
             (dict(dim=68), "multiple of 8"), (dict(z_ptr=None), "null output"), (dict(gamma_ptr=None), "needs gamma and beta"),
             (dict(beta_ptr=None), "needs gamma and beta"), (dict(eps=0.0), "eps must be positive"), (dict(hi_ptr=4100), "not 16-byte aligned"),
             (dict(z_ptr=4104), "not 16-byte aligned"), (dict(qk_ptr=None), "null qk"), (dict(qk_ptr=4100), "not 16-byte aligned"),
             (dict(heads=0), "heads outside 1..16"), (dict(heads=17), "heads outside 1..16")]
    for change, text in cases:
        with pytest.raises(vithip.VhError) as e:
            vithip.op_map_pool(**dict(ok, **change))
        assert e.value.code == VH_ERR_INVALID and "map_pool:" in str(e.value) and text in str(e.value), (change, str(e.value))


def test_the_gpu_bound_is_four_times_the_float32_statements_error():
    """MAP_BOUND, which tests/test_gpu_siglip.py holds the kernel to: over the kernel test's own inputs, in all four input forms, the
    float32 statement of the function against float64.  Also checks the inputs themselves: finite float64 results, and the arranged
    cases arranged as their names say."""
    forms = (vithip.FEAT_FORM_F32, BF16, FP16, FP8)
    worst = {}
    for dim in HF.MAP_DIMS:
        for heads, NP, lead, batch, order in HF.map_pool_cases(dim):
            x, gamma, beta, qk = HF.map_pool_inputs(dim, heads, NP, lead, batch, order)
            assert np.abs(x).max() == 300.0
            for fm in forms:
                xr = FR.split_planes(x.reshape(-1, dim), fm)[2].reshape(x.shape)
                z64, s = HF.map_z64(xr, gamma, beta, qk, lead)
                assert np.isfinite(z64).all()
                e = float(np.abs(HF.map_z32(xr, gamma, beta, qk, lead) - z64).max() / np.abs(z64).max())
                worst[order] = max(worst.get(order, 0.0), e)
                g = HF.map_pool_group(dim, heads)
                if order == "ascending":
                    assert (np.diff(s, axis=-1) >= 0).all()
                elif order == "descending":
                    assert (np.diff(s, axis=-1) <= 0).all()
                elif order == "gap":
                    for k in range(2):
                        assert (s[:, :, (k + 1) * g:(k + 2) * g].min(-1) - s[:, :, k * g:(k + 1) * g].max(-1)).min() >= 200.0
    print("\n[siglip] float32 statement vs float64, max |d| / max |z64|: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        assert 4.0 * v <= MAP_BOUND[k] <= 4.0 * v * 1.25, (k, v, MAP_BOUND[k])
