"""Pooled heads and models without a class token on the host: VH_FLAG_NO_CLS and VH_FLAG_POOL(m) are valid settings in the
combinations the contract names, the blob loses `cls` and pos[0] / widens the head accordingly, the header carries the bits, every
refusal has its message, and the converters give the reference's bytes.  The reference the GPU tests use, tests/vit_ref.py, is
pinned here: against four fixtures computed by Hugging Face `transformers` (IJepaForImageClassification,
Dinov2[WithRegisters]ForImageClassification, BeitForImageClassification; tests/golden/make_golden_pool.py); its blob sizes and header
bits, over every legal flag word, against the library.  No GPU needed."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as H
import vh_synth as S
import vit_ref as R
from vh_testlib import lib_blob_bytes, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "pool", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK, REG, NO_CLS, POOL = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU, vithip.FLAG_REGISTERS, vithip.FLAG_NO_CLS, vithip.FLAG_POOL
CLS, AVG_NORM, AVG_FCNORM, CLS_AVG = vithip.POOL_CLS, vithip.POOL_AVG_NORM, vithip.POOL_AVG_FCNORM, vithip.POOL_CLS_AVG
VH_ERR_INVALID = 1
MICRO = S.CONFIGS["vit_micro"]
LEGAL = [POOL(m) for m in (CLS, AVG_NORM, AVG_FCNORM, CLS_AVG)] + [NO_CLS | POOL(AVG_NORM), NO_CLS | POOL(AVG_FCNORM)]


def _create_error(cfg, flags=0, dtype=BF16, max_batch=1):
    c = vithip.make_config(cfg, dtype, max_batch, 1e-6, flags)
    h = C.c_void_p()
    rc = vithip.lib().vh_create(C.byref(c), 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, vithip.lib().vh_last_error(None).decode()


def test_the_macro_values():
    assert NO_CLS == 1 << 15 == R.FLAG_NO_CLS
    assert [POOL(m) for m in range(4)] == [0, 1 << 16, 2 << 16, 3 << 16] == [R.FLAG_POOL(m) for m in range(4)]
    assert (CLS, AVG_NORM, AVG_FCNORM, CLS_AVG) == (0, 1, 2, 3)
    assert [vithip.pool_of(POOL(m) | NO_CLS | REG(4) | PRE | 15) for m in range(4)] == [0, 1, 2, 3]
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("#define VH_FLAG_NO_CLS (1 << 15)", "#define VH_FLAG_POOL(m) (((m) & 3) << 16)", "#define VH_POOL_CLS 0",
                 "#define VH_POOL_AVG_NORM 1", "#define VH_POOL_AVG_FCNORM 2", "#define VH_POOL_CLS_AVG 3", "int vh_op_pool_rows("):
        assert text in hdr, text
    assert "vh_op_pool_rows" in vithip.SYMBOLS


def test_blob_bytes_of_every_legal_combination():
    for cfg in (MICRO, dict(image_size=224, patch_size=14, channels=3, dim=384, heads=6, mlp_dim=1536, layers=12, classes=1000)):
        base, D, Cn = 64 + 4 * S.param_count(cfg), cfg["dim"], cfg["classes"]
        for f in LEGAL:
            for n in (0, 4):
                for pre in (0, PRE):
                    flags = f | REG(n) | pre
                    want = base + 4 * (n * D + (2 * D if pre else 0) - (2 * D if f & NO_CLS else 0) + (Cn * D if vithip.pool_of(f) == CLS_AVG else 0))
                    assert lib_blob_bytes(cfg, flags) == want == R.blob_bytes(cfg, flags), (f, n, pre)


def test_layout_of_the_blob():
    names = [n for n, *_ in R.tensor_table(MICRO, NO_CLS | POOL(AVG_NORM) | REG(4))]
    assert names[:4] == ["patch.weight", "patch.bias", "pos", "reg"] and "cls" not in names
    t = R.make_tensors(MICRO, 9, NO_CLS | POOL(AVG_NORM) | REG(4))
    full = R.make_tensors(MICRO, 9, REG(4))
    assert t["pos"].shape == (S.tokens(MICRO) - 1, MICRO["dim"])
    assert np.array_equal(t["reg"], full["reg"]) and np.array_equal(t["lnf.weight"], full["lnf.weight"])   # the tensor ids are kept
    t = R.make_tensors(MICRO, 9, POOL(CLS_AVG))
    assert t["head.weight"].shape == (MICRO["classes"], 2 * MICRO["dim"])
    assert R.make_blob(MICRO, 9, NO_CLS | POOL(AVG_FCNORM) | REG(4) | PRE)[52:56].view(np.uint32)[0] == 2 | (4 << 9) | (1 << 15) | (2 << 16)


def test_refusals_each_with_its_message():
    for f, text in ((NO_CLS, "VH_POOL_CLS reads the class token"), (NO_CLS | POOL(CLS_AVG), "VH_FLAG_NO_CLS excludes VH_POOL_CLS_AVG"),
                    (vithip.FLAG_CLS_TAIL | NO_CLS | POOL(AVG_NORM), "VH_FLAG_CLS_TAIL excludes VH_FLAG_NO_CLS"),
                    (vithip.FLAG_CLS_TAIL | POOL(AVG_NORM), "VH_FLAG_CLS_TAIL excludes VH_FLAG_POOL"),
                    (vithip.FLAG_CLS_TAIL | POOL(CLS_AVG), "VH_FLAG_CLS_TAIL excludes VH_FLAG_POOL")):
        assert lib_blob_bytes(MICRO, f) == 0, f
        rc, msg = _create_error(MICRO, f)
        assert rc == VH_ERR_INVALID and text in msg, (f, msg)
    # the token bounds apply to the new T: a 64 x 64 grid without a class token has room for one register token
    grid64 = dict(image_size=1024, patch_size=16, channels=3, dim=128, heads=2, mlp_dim=256, layers=1, classes=4)
    nc = NO_CLS | POOL(AVG_NORM)
    assert lib_blob_bytes(grid64, nc) == R.blob_bytes(grid64, nc) and lib_blob_bytes(grid64, nc | REG(1)) == R.blob_bytes(grid64, nc | REG(1))
    assert lib_blob_bytes(grid64, nc | REG(2)) == 0 and lib_blob_bytes(grid64, POOL(AVG_NORM) | REG(1)) == 0
    rc, msg = _create_error(grid64, nc | REG(2))
    assert rc == VH_ERR_INVALID and "4097" in msg and "without a class token" in msg, msg
    grid26 = dict(grid64, image_size=416)     # 676 tokens without the class token, 677 with it
    big = (640 << 20) // 676
    assert big < 1 << 20 and lib_blob_bytes(grid26, nc, max_batch=big) > 0 and lib_blob_bytes(grid26, POOL(AVG_NORM), max_batch=big) == 0
    assert "max_batch x tokens" in _create_error(grid26, nc, max_batch=big + 1)[1]
    one = dict(grid64, image_size=16)         # T = 1: one patch, no class token, no register
    assert lib_blob_bytes(one, nc) == R.blob_bytes(one, nc) and R.tokens(one, nc) == 1


def test_the_pinned_unknown_bits_are_still_unknown():
    for bad in (64, 128, 256, 1 << 14, 1 << 20, -1, POOL(AVG_NORM) | (1 << 14), NO_CLS | POOL(AVG_NORM) | (1 << 18), 1 << 18):
        assert lib_blob_bytes(MICRO, bad) == 0, bad
        assert "unknown bits in flags" in _create_error(MICRO, bad)[1]


def test_header_bits_round_trip_through_the_blob_file_entry_points(tmp_path):
    for flags in LEGAL[1:] + [NO_CLS | POOL(AVG_FCNORM) | REG(4) | PRE | QUICK]:
        blob = R.make_blob(MICRO, 5, flags, 1e-5)
        path = tmp_path / f"micro_{flags}.vhblob"
        blob.tofile(path)
        got, eps = vithip.blob_file_config(path)
        assert got == MICRO and abs(eps - 1e-5) < 1e-12
        assert vithip.blob_file_flags(path) == flags
        back = np.zeros(blob.nbytes, np.uint8)
        assert vithip.lib().vh_blob_file_read(os.fsencode(path), back.ctypes.data, back.nbytes) == 0 and np.array_equal(back, blob)
    path = tmp_path / "bad.vhblob"
    blob = R.make_blob(MICRO, 5, POOL(CLS_AVG))
    blob[52:56] = np.array([POOL(AVG_NORM)], np.uint32).view(np.uint8)             # a [C][2 D] head under a header that says [C][D]
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    blob[52:56] = np.array([NO_CLS], np.uint32).view(np.uint8)                     # an illegal combination in a header
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="VH_POOL_CLS reads the class token"):
        vithip.blob_file_config(path)
    blob[52:56] = np.array([8], np.uint32).view(np.uint8)                          # header bit 3 is still unknown
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="unknown bits in the header"):
        vithip.blob_file_config(path)


# ---- the reference against the fixtures -------------------------------------------------------------------------------------
def load_fixture(path):
    z = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in z["config"])))
    wseed, iseed, batch, flags = (int(v) for v in z["meta"])
    return z, str(z["kind"]), cfg, wseed, iseed, batch, flags, float(z["ln_eps"])


def fixture_blob(kind, cfg, wseed, flags, eps):
    """The blob of a fixture's model through the converter that takes its state dict (BEiT has none: vit_ref.pack_blob)."""
    t = H.fixture_tensors(kind, cfg, flags, wseed)
    if kind == "ijepa":
        return vithip.blob_from_ijepa_state_dict(H.ijepa_state_dict(cfg, t), cfg, eps)
    if kind == "dinov2":
        return vithip.blob_from_dinov2_state_dict(H.dinov2_classifier_state_dict(cfg, t, wseed), dict(cfg, registers=R.registers_of(flags)), eps,
                                                  pool=CLS_AVG)
    return R.pack_blob(cfg, t, flags, eps)


def test_fixtures_are_present():
    assert len(GOLDEN) == 4, GOLDEN
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "golden", "reg", "*.npz")))
    assert all(os.path.getsize(p) <= biggest for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p).split("_s")[0] for p in GOLDEN])
def test_pool_ref_reproduces_the_transformers_fixture(path):
    """Logits, the head's input and the final rows of the transformers model (float64) against vit_ref in float64.  The bound 1e-5
    is tests/test_registers.py's: the fp32 rounding of the weights and of the folded LayerScale."""
    z, kind, cfg, wseed, iseed, batch, flags, eps = load_fixture(path)
    blob = fixture_blob(kind, cfg, wseed, flags, eps)
    assert blob.nbytes == R.blob_bytes(cfg, flags) and int(blob[52:56].view(np.uint32)[0]) == flags
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(z["images_checksum"][0])) < 1e-9
    logits, x, hin = R.forward(cfg, blob, images, flags, eps, np.float64, want_hidden=True, want_head=True)
    T, D = R.tokens(cfg, flags), cfg["dim"]
    # BEiT's encoder ends without a norm when it mean-pools (pooler.layernorm is lnf); the others return LN(x)
    last = x if kind == "beit" else R.layernorm(x, *(R.unpack_blob(cfg, blob, flags)[k].astype(np.float64) for k in ("lnf.weight", "lnf.bias")), eps)
    for name, got, want in (("last_hidden_state", last.reshape(batch, T, D), z["last_hidden_state"]), ("head_input", hin, z["head_input"]),
                            ("logits", logits, z["logits"])):
        e = rel(got, want)
        print(f"{os.path.basename(path)}: {name}: max|d|/max|ref| = {e:.3e}")
        assert got.shape == want.shape and e <= 1e-5, (name, e)


def test_every_legal_flag_word_has_the_librarys_blob_bytes_and_a_header_that_round_trips(tmp_path):
    """The flag words profiles/ref_model_equivalence.txt lists: the CLIP switches, register counts, and NO_CLS x POOL x REG."""
    grid = [0, PRE, QUICK, PRE | QUICK, REG(1), REG(4), PRE | QUICK | REG(1)]
    grid += [nc | POOL(m) | REG(n) for nc in (0, NO_CLS) for m in range(4) for n in (0, 4) if R.legal(MICRO, nc | POOL(m))]
    assert len(set(grid)) == 17 and not any(R.legal(MICRO, NO_CLS | POOL(m)) for m in (CLS, CLS_AVG))
    for flags in grid:
        assert R.blob_bytes(MICRO, flags) == lib_blob_bytes(MICRO, flags) > 0, flags
        blob = R.make_blob(MICRO, 5, flags, 1e-5)
        assert blob.nbytes == R.blob_bytes(MICRO, flags)
        path = tmp_path / f"micro_{flags}.vhblob"
        blob.tofile(path)
        assert vithip.blob_file_config(path)[0] == MICRO and vithip.blob_file_flags(path) == flags, flags


def test_assembly_without_row_0_and_the_pool_modes():
    rng = np.random.default_rng(3)
    emb, cls, pos, reg = rng.normal(size=(2, 4, 8)), rng.normal(size=8), rng.normal(size=(5, 8)), rng.normal(size=(3, 8))
    full = R.assemble(emb, cls, pos, reg)
    x = R.assemble(emb, None, pos[1:], reg)
    assert x.shape == (2, 7, 8) and np.array_equal(x, full[:, 1:])                # the class-token model's rows without row 0
    assert np.array_equal(R.assemble(emb, None, pos[1:]), full[:, 4:])
    g, b = rng.normal(size=8), rng.normal(size=8)
    ln = lambda v: R.layernorm(v, g, b, 1e-6)
    assert np.array_equal(R.head_input(full, g, b, 1e-6, 4, CLS), ln(full[:, 0]))
    assert np.array_equal(R.head_input(full, g, b, 1e-6, 4, AVG_NORM), ln(full[:, 4:]).mean(1))      # never the class token or the registers
    assert np.array_equal(R.head_input(full, g, b, 1e-6, 4, AVG_FCNORM), ln(full[:, 4:].mean(1)))
    assert np.array_equal(R.head_input(full, g, b, 1e-6, 4, CLS_AVG), np.concatenate([ln(full[:, 0]), ln(full[:, 4:]).mean(1)], 1))
    assert np.array_equal(R.head_input(x, g, b, 1e-6, 3, AVG_NORM), R.head_input(full, g, b, 1e-6, 4, AVG_NORM))


# ---- the converters ---------------------------------------------------------------------------------------------------------
CONV = dict(image_size=28, patch_size=14, channels=3, dim=64, heads=2, mlp_dim=128, layers=2, classes=8)


def test_ijepa_converter_gives_pack_blobs_bytes_and_refuses():
    flags = NO_CLS | POOL(AVG_NORM)
    t = R.make_tensors(CONV, 71, flags)
    sd = H.ijepa_state_dict(CONV, t)
    assert np.array_equal(vithip.blob_from_ijepa_state_dict(sd, CONV), R.pack_blob(CONV, t, flags))
    body = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    zero = dict(t, **{"head.weight": np.zeros_like(t["head.weight"]), "head.bias": np.zeros_like(t["head.bias"])})
    assert np.array_equal(vithip.blob_from_ijepa_state_dict(body, CONV), R.pack_blob(CONV, zero, flags))
    bare = {k[len("ijepa."):]: v for k, v in body.items()}                          # an IJepaModel state dict
    assert np.array_equal(vithip.blob_from_ijepa_state_dict(bare, CONV, head=(t["head.weight"], t["head.bias"])), R.pack_blob(CONV, t, flags))
    with pytest.raises(ValueError, match="head has shapes"):
        vithip.blob_from_ijepa_state_dict(body, CONV, head=(np.zeros((8, 128)), np.zeros(8)))
    with pytest.raises(ValueError, match=r"position_embeddings has 4 rows, cfg needs NP = 16"):
        vithip.blob_from_ijepa_state_dict(sd, dict(CONV, image_size=56))
    with pytest.raises(ValueError, match="has a class token"):
        vithip.blob_from_ijepa_state_dict(dict(sd, **{"ijepa.embeddings.cls_token": np.zeros((1, 1, 64), np.float32)}), CONV)
    with pytest.raises(KeyError, match="layernorm_after"):
        vithip.blob_from_ijepa_state_dict({k: v for k, v in sd.items() if k != "ijepa.layers.1.layernorm_after.bias"}, CONV)


def test_dinov2_converter_with_the_linear_classifiers_head():
    for regs in (0, 2):
        flags = REG(regs) | POOL(CLS_AVG)
        t = R.make_tensors(CONV, 71, flags)
        cfg = dict(CONV, registers=regs)
        sd = H.dinov2_classifier_state_dict(CONV, t, 71, unit_scale=True)
        assert any(k.startswith("dinov2_with_registers." if regs else "dinov2.") for k in sd)
        assert np.array_equal(vithip.blob_from_dinov2_state_dict(sd, cfg, pool=CLS_AVG), R.pack_blob(CONV, t, flags))
        backbone = H.dinov2_state_dict(CONV, t, 71, unit_scale=True)               # the backbone's own names + an explicit head
        assert np.array_equal(vithip.blob_from_dinov2_state_dict(backbone, cfg, head=(t["head.weight"], t["head.bias"]), pool=CLS_AVG),
                              R.pack_blob(CONV, t, flags))
        with pytest.raises(ValueError, match="head has shapes"):                   # a [C][2 D] head needs the mode
            vithip.blob_from_dinov2_state_dict(sd, cfg)
        with pytest.raises(ValueError, match="head has shapes"):
            vithip.blob_from_dinov2_state_dict(backbone, cfg, head=(np.zeros((8, 64)), np.zeros(8)), pool=CLS_AVG)
    with pytest.raises(ValueError, match="pool = 7"):
        vithip.blob_from_dinov2_state_dict(H.dinov2_state_dict(CONV, R.make_tensors(CONV, 71, 0), 71), CONV, pool=7)


def timm_state_dict(cfg, t, seed, fc_norm, unit_scale=False, no_embed_class=False):
    """The seeded tensors under timm's VisionTransformer parameter names (built by hand: timm is not installed here)."""
    D = cfg["dim"]
    sd = {"patch_embed.proj.weight": t["patch.weight"], "patch_embed.proj.bias": t["patch.bias"]}
    if "cls" in t:
        sd["cls_token"] = t["cls"].reshape(1, 1, D)
    if "reg" in t:
        sd["reg_token"] = t["reg"].reshape(1, -1, D)
    pos = t["pos"][1:] if no_embed_class else t["pos"]
    sd["pos_embed"] = pos.reshape(1, -1, D)
    for l in range(cfg["layers"]):
        b = f"blocks.{l}."
        sd[b + "attn.qkv.weight"] = np.concatenate([t[f"l{l}.{n}.weight"] for n in "qkv"])
        sd[b + "attn.qkv.bias"] = np.concatenate([t[f"l{l}.{n}.bias"] for n in "qkv"])
        for ours, theirs in (("ln1", "norm1"), ("o", "attn.proj"), ("ln2", "norm2"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + theirs + ".weight"], sd[b + theirs + ".bias"] = t[f"l{l}.{ours}.weight"], t[f"l{l}.{ours}.bias"]
        if not unit_scale:
            sd[b + "ls1.gamma"], sd[b + "ls2.gamma"] = H.layer_scale(cfg, seed, l)
    ln = "fc_norm" if fc_norm else "norm"
    sd[ln + ".weight"], sd[ln + ".bias"] = t["lnf.weight"], t["lnf.bias"]
    sd["head.weight"], sd["head.bias"] = t["head.weight"], t["head.bias"]
    return sd


def test_timm_converter_gives_pack_blobs_bytes_and_refuses():
    conv = vithip.blob_from_timm_vit_state_dict
    for flags, pool, fcn in ((0, "token", False), (POOL(AVG_FCNORM), "avg", True), (POOL(AVG_NORM), "avg", False),
                             (NO_CLS | POOL(AVG_FCNORM) | REG(2), "avg", None), (REG(2) | POOL(AVG_NORM), "avg", False)):
        t = R.make_tensors(CONV, 73, flags)
        cfg = dict(CONV, registers=R.registers_of(flags))
        fc = pool == "avg" if fcn is None else fcn
        assert np.array_equal(conv(timm_state_dict(CONV, t, 73, fc, unit_scale=True), cfg, 1e-6, pool, fcn), R.pack_blob(CONV, t, flags)), flags
    # LayerScale folds as in the DINOv2 converter; the fused qkv splits into q, k, v
    t = R.make_tensors(CONV, 73, POOL(AVG_FCNORM))
    got = R.unpack_blob(CONV, conv(timm_state_dict(CONV, t, 73, True), CONV, 1e-6, "avg", True), POOL(AVG_FCNORM))
    l1, l2 = (a.astype(np.float64) for a in H.layer_scale(CONV, 73, 1))
    assert np.array_equal(got["l1.o.weight"], (t["l1.o.weight"].astype(np.float64) * l1[:, None]).astype(np.float32))
    assert np.array_equal(got["l1.fc2.bias"], (t["l1.fc2.bias"].astype(np.float64) * l2).astype(np.float32))
    assert all(np.array_equal(got[f"l1.{n}.weight"], t[f"l1.{n}.weight"]) for n in "qkv")
    # no_embed_class: NP rows with a class token, whose position row is zero
    got = R.unpack_blob(CONV, conv(timm_state_dict(CONV, t, 73, True, True, no_embed_class=True), CONV, 1e-6, "avg", True), POOL(AVG_FCNORM))
    assert not got["pos"][0].any() and np.array_equal(got["pos"][1:], t["pos"][1:])
    sd = timm_state_dict(CONV, t, 73, True, True)
    with pytest.raises(ValueError, match=r"pos_embed has 5 rows, cfg needs NP = 16 or NP \+ 1 = 17"):
        conv(sd, dict(CONV, image_size=56), 1e-6, "avg", True)
    with pytest.raises(ValueError, match=r"pos_embed has 5 rows, cfg needs NP = 4$"):
        conv({k: v for k, v in sd.items() if k != "cls_token"}, CONV, 1e-6, "avg", True)
    with pytest.raises(ValueError, match="needs a cls_token"):
        conv({k: v for k, v in sd.items() if k != "cls_token"}, CONV, 1e-6, "token")
    with pytest.raises(ValueError, match="is not 'token' or 'avg'"):
        conv(sd, CONV, 1e-6, "max")
    with pytest.raises(ValueError, match="head.weight has shape"):
        conv(dict(sd, **{"head.weight": np.zeros((8, 128), np.float32)}), CONV, 1e-6, "avg", True)
    with pytest.raises(KeyError, match="fc_norm.weight"):
        conv(timm_state_dict(CONV, t, 73, False, True), CONV, 1e-6, "avg", True)


# ---- the tap's refusals (every argument is checked before a device is touched) ----------------------------------------------
def test_op_pool_rows_refusals():
    ok = dict(hi_ptr=4096, lo_ptr=8192, form=BF16, batch=2, tokens=9, lead=1, dim=64, gamma_ptr=4096, beta_ptr=4096, eps=1e-6,
              norm=vithip.FEAT_NORM, mean_ptr=4096)
    cases = [(dict(hi_ptr=None), "null input"), (dict(form=7), "form must be"), (dict(form=-1), "fp32 rows take no lo plane"),
             (dict(lo_ptr=None), "split planes need the lo plane"), (dict(batch=0), "batch outside"), (dict(batch=(1 << 20) + 1), "batch outside"),
             (dict(tokens=0, lead=0), "tokens below 1"), (dict(tokens=4098), "tokens above 4097"), (dict(lead=-1), "lead rows outside 0 .. tokens - 1"),
             (dict(lead=9), "lead rows outside 0 .. tokens - 1"), (dict(dim=56), "dim below 64"), (dict(dim=2056), "dim above 2048"),
             (dict(dim=68), "multiple of 8"), (dict(mean_ptr=None), "null output"), (dict(norm=2), "norm must be"),
             (dict(gamma_ptr=None), "needs gamma and beta"), (dict(beta_ptr=None), "needs gamma and beta"), (dict(eps=0.0), "eps must be positive"),
             (dict(hi_ptr=4100), "not 16-byte aligned"), (dict(mean_ptr=4104), "not 16-byte aligned")]
    for change, text in cases:
        with pytest.raises(vithip.VhError) as e:
            vithip.op_pool_rows(**dict(ok, **change))
        assert e.value.code == VH_ERR_INVALID and "pool_rows:" in str(e.value) and text in str(e.value), (change, str(e.value))


def test_get_intermediate_layers_refuses_the_class_token_without_one():
    ctx = vithip.VitContext.__new__(vithip.VitContext)      # no device needed: the refusal comes before any library call
    ctx.h, ctx.cfg = None, dict(MICRO)
    ctx.c = vithip.make_config(MICRO, flags=NO_CLS | POOL(AVG_NORM))
    with pytest.raises(ValueError, match="without a class token"):
        ctx.get_intermediate_layers(1, return_class_token=True)
