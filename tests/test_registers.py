"""Register tokens on the host: VH_FLAG_REGISTERS(n) is a valid setting (0 .. 16, with every other flag and dtype), the blob grows
by reg [R][D] directly after `pos`, the header carries the count, and the DINOv2 converter folds LayerScale exactly and refuses
what the library does not run.  The reference the GPU tests use, tests/vit_ref.py, is pinned here: against two fixtures computed
by Hugging Face `transformers`' Dinov2WithRegistersModel (tests/golden/make_golden_reg.py), and, with no flag, against vh_synth's
blob and the C oracle.  No GPU needed."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as H
import oracle_lib as O
import vh_synth as S
import vit_ref as R
from vh_testlib import lib_blob_bytes, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "reg", "*.npz")))
CFG_KEYS = ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK, REG = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU, vithip.FLAG_REGISTERS
VH_ERR_INVALID = 1
MICRO = S.CONFIGS["vit_micro"]
S14 = dict(image_size=224, patch_size=14, channels=3, dim=384, heads=6, mlp_dim=1536, layers=12, classes=1000)


def _create_error(cfg, flags=0, dtype=BF16, max_batch=1):
    """The message vh_create refuses the configuration with (the configuration is checked before any device is looked for)."""
    c = vithip.make_config(cfg, dtype, max_batch, 1e-6, flags)
    h = C.c_void_p()
    rc = vithip.lib().vh_create(C.byref(c), 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, vithip.lib().vh_last_error(None).decode()


def load_fixture(path):
    z = np.load(path)
    cfg = dict(zip(CFG_KEYS, (int(v) for v in z["config"])))
    wseed, iseed, batch, regs = (int(v) for v in z["meta"])
    return z, cfg, wseed, iseed, batch, regs, float(z["ln_eps"])


def fixture_blob(cfg, wseed, regs, eps, unit_scale=False, head=None):
    """The converter's blob of the fixture's model (the seeded tensors under the Hugging Face names + the seeded LayerScale)."""
    sd = H.dinov2_state_dict(cfg, R.make_tensors(cfg, wseed, REG(regs)), wseed, unit_scale)
    return vithip.blob_from_dinov2_state_dict(sd, dict(cfg, registers=regs), eps, head)


def test_the_flag_macros():
    assert [REG(n) for n in (0, 1, 4, 16, 31)] == [0, 512, 2048, 8192, 31 << 9]
    assert vithip.FLAG_REGISTERS_MASK == 31 << 9 == R.FLAG_REGISTERS_MASK
    assert [vithip.registers_of(REG(n) | PRE | QUICK | 15) for n in (0, 3, 16)] == [0, 3, 16]
    assert vithip.lib().vh_abi_version() == 1 and C.sizeof(vithip.Config) == 48          # the count travels in flags


def test_blob_bytes_grow_by_the_register_rows():
    for cfg in (MICRO, S14):
        base = 64 + 4 * S.param_count(cfg)
        D = cfg["dim"]
        for n in (0, 1, 4, 16):
            for dt in (BF16, FP16) + ((FP8,) if D % 128 == 0 else ()):
                assert lib_blob_bytes(cfg, REG(n), dt) == base + 4 * n * D == R.blob_bytes(cfg, REG(n)), (n, dt)
        assert lib_blob_bytes(cfg, REG(4) | PRE) == base + 4 * 4 * D + 8 * D == R.blob_bytes(cfg, REG(4) | PRE)
        # the count from the model dict, as make_config / VitContext / VitGroup take it
        assert lib_blob_bytes(dict(cfg, registers=4)) == base + 4 * 4 * D
        assert vithip.make_config(dict(cfg, registers=4)).flags == REG(4) == vithip.make_config(cfg, flags=REG(4)).flags
    with pytest.raises(ValueError, match="registers"):
        vithip.make_config(dict(MICRO, registers=4), flags=REG(2))


def test_the_setting_is_independent_of_every_other_flag_and_dtype():
    cfg = dict(image_size=224, patch_size=32, channels=3, dim=768, heads=12, mlp_dim=3072, layers=2, classes=512)
    others = [0, vithip.FLAG_LN_FOLD_OFF, vithip.FLAG_LN_FOLD_ON, vithip.FLAG_W8_E4M3, vithip.FLAG_CLS_TAIL, PRE, QUICK,
              vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL | vithip.FLAG_W8_E4M3 | PRE | QUICK]
    for n in (1, 16):
        for o in others:
            for dt in (BF16, FP16, FP8):
                want = 0 if (dt == FP8 and o & vithip.FLAG_W8_E4M3) else R.blob_bytes(cfg, REG(n) | (o & (PRE | QUICK)))
                assert lib_blob_bytes(cfg, REG(n) | o, dt) == want, (n, o, dt)


def test_layout_of_the_blob_with_registers():
    names = [n for n, *_ in R.tensor_table(MICRO, REG(4))]
    assert names[:5] == ["patch.weight", "patch.bias", "cls", "pos", "reg"] and names[5] == "l0.ln1.weight"
    names = [n for n, *_ in R.tensor_table(MICRO, REG(4) | PRE)]
    assert names[:7] == ["patch.weight", "patch.bias", "cls", "pos", "reg", "pre_ln.weight", "pre_ln.bias"]
    t = R.make_tensors(MICRO, 9, REG(4))
    assert t["pos"].shape == (S.tokens(MICRO), MICRO["dim"])                       # registers carry no position row
    assert np.array_equal(t["reg"], S.fill(4 * MICRO["dim"], 9, 7, 1, 0.02, 0.0).reshape(4, -1))   # tensor id 7, sigma as cls
    assert np.array_equal(R.make_blob(MICRO, 9, 0), S.make_blob(MICRO, 9))         # R = 0: byte for byte today's blob
    assert R.make_blob(MICRO, 9, REG(4) | PRE | QUICK)[52:56].view(np.uint32)[0] == 6 | (4 << 9)


def test_counts_above_16_and_the_64_grid_are_refused_with_a_message():
    assert lib_blob_bytes(MICRO, REG(16)) > 0
    for n in (17, 24, 31):
        assert lib_blob_bytes(MICRO, REG(n)) == 0
        rc, msg = _create_error(MICRO, REG(n))
        assert rc == VH_ERR_INVALID and "0 .. 16 register tokens" in msg, msg
    grid64 = dict(image_size=1024, patch_size=16, channels=3, dim=128, heads=2, mlp_dim=256, layers=1, classes=4)
    assert lib_blob_bytes(grid64, 0) > 0                                              # 4097 tokens: still accepted
    for n in (1, 16):
        assert lib_blob_bytes(grid64, REG(n)) == 0
        rc, msg = _create_error(grid64, REG(n))
        assert rc == VH_ERR_INVALID and "4097" in msg and "register" in msg, msg
    grid63 = dict(grid64, image_size=1008)
    assert lib_blob_bytes(grid63, REG(16)) == R.blob_bytes(grid63, REG(16))           # 63^2 + 17 = 3986 tokens
    # max_batch x tokens <= 640 x 2^20 counts the register rows: a 25 x 25 grid has 626 tokens (every max_batch <= 2^20 fits) and
    # 642 with 16 registers
    grid25 = dict(grid64, image_size=400)
    big = (640 << 20) // 642
    assert big < 1 << 20 and lib_blob_bytes(grid25, REG(16), max_batch=big) > 0 and lib_blob_bytes(grid25, REG(16), max_batch=big + 1) == 0
    assert "max_batch x tokens" in _create_error(grid25, REG(16), max_batch=big + 1)[1]
    assert lib_blob_bytes(grid25, 0, max_batch=1 << 20) > 0
    # the bits around the count are still unknown (bit 8 among them: tests/test_clip.py lists QUICK | 256)
    for bad in (1 << 14, REG(4) | (1 << 14), 256, REG(4) | 256, 64, 128):
        assert lib_blob_bytes(MICRO, bad) == 0, bad


def test_header_count_round_trips_through_the_blob_file_entry_points(tmp_path):
    for flags in (REG(1), REG(16), REG(4) | PRE | QUICK):
        blob = R.make_blob(MICRO, 5, flags, 1e-5)
        path = tmp_path / f"micro_{flags}.vhblob"
        blob.tofile(path)
        got, eps = vithip.blob_file_config(path)
        assert got == MICRO and abs(eps - 1e-5) < 1e-12
        assert vithip.blob_file_flags(path) == flags and vithip.registers_of(vithip.blob_file_flags(path)) == flags >> 9 & 31
        back = np.zeros(blob.nbytes, np.uint8)
        assert vithip.lib().vh_blob_file_read(os.fsencode(path), back.ctypes.data, back.nbytes) == 0 and np.array_equal(back, blob)
    path = tmp_path / "bad.vhblob"
    blob = R.make_blob(MICRO, 5, REG(4))
    blob[52:56] = np.array([REG(3)], np.uint32).view(np.uint8)                     # one register row more than the header says
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    blob[52:56] = np.array([REG(17)], np.uint32).view(np.uint8)
    blob.tofile(path)
    with pytest.raises(vithip.VhError, match="register tokens"):
        vithip.blob_file_config(path)


def test_abi_symbol_for_the_register_count():
    assert "vh_get_register_tokens" in vithip.SYMBOLS
    fn = vithip.lib().vh_get_register_tokens
    assert fn.restype is C.c_int and fn(None) == -1                                # a null context: no count
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("int vh_get_register_tokens(const vh_ctx* ctx);", "#define VH_FLAG_REGISTERS(n) (((n) & 31) << 9)",
                 "#define VH_FLAG_REGISTERS_MASK (31 << 9)", "#define VH_FLAG_REGISTERS_OF(flags)"):
        assert text in hdr, text


# ---- the reference against the fixtures -------------------------------------------------------------------------------------
def test_fixtures_are_present():
    assert len(GOLDEN) == 2, GOLDEN


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:9] for p in GOLDEN])
def test_reg_ref_on_the_converters_blob_reproduces_the_transformers_fixture(path):
    """Final-LayerNorm rows and every hidden state of Dinov2WithRegistersModel (float64) against vit_ref in float64 on the
    converter's blob.  The bound 1e-5 is the fp32 rounding of the weights and of the folded LayerScale."""
    z, cfg, wseed, iseed, batch, regs, eps = load_fixture(path)
    flags = REG(regs)
    blob = fixture_blob(cfg, wseed, regs, eps)
    assert blob.nbytes == R.blob_bytes(cfg, flags) and int(blob[52:56].view(np.uint32)[0]) == flags
    images = S.make_images(cfg, iseed, batch)
    assert abs(float(images.astype(np.float64).sum()) - float(z["images_checksum"][0])) < 1e-9
    _, x, hidden = R.forward(cfg, blob, images, flags, eps, np.float64, all_hidden=True)
    T, D = R.tokens(cfg, flags), cfg["dim"]
    assert z["hidden_states"].shape == (cfg["layers"] + 1, batch, T, D) and len(hidden) == cfg["layers"] + 1
    for l, h in enumerate(hidden):
        e = rel(h.reshape(batch, T, D), z["hidden_states"][l])
        print(f"{os.path.basename(path)}: hidden state {l}: max|d|/max|ref| = {e:.3e}")
        assert e <= 1e-5, (l, e)
    e = rel(R.final_norm(cfg, blob, x, flags, eps).reshape(batch, T, D), z["last_hidden_state"])
    print(f"{os.path.basename(path)}: last_hidden_state: max|d|/max|ref| = {e:.3e}")
    assert e <= 1e-5, e
    # the register rows are where the row order says: rows 1 .. R of the embedded state are reg, the same for every image
    reg = R.unpack_blob(cfg, blob, flags)["reg"]
    assert np.array_equal(z["hidden_states"][0][:, 1:1 + regs].astype(np.float32), np.broadcast_to(reg, (batch, regs, D)))


def test_with_no_flag_vit_ref_is_vh_synths_blob_and_the_oracle():
    for cfg in (MICRO, S14, S.CONFIGS["vit_gray"]):
        assert R.tensor_table(cfg) == S.tensor_table(cfg)
    for cfg in (MICRO, S.CONFIGS["vit_gray"]):
        assert np.array_equal(R.make_blob(cfg, 11), S.make_blob(cfg, 11))
    assert np.array_equal(R.make_blob(MICRO, 11, 0, 1e-5), S.make_blob(MICRO, 11, 1e-5))
    blob, images = S.make_blob(MICRO, 11), S.make_images(MICRO, 12, 3)
    assert rel(R.forward(MICRO, blob, images, 0), O.vit_forward(MICRO, blob, images)) <= 1e-5


def test_token_assembly_row_order():
    rng = np.random.default_rng(3)
    emb, cls, pos, reg = rng.normal(size=(2, 4, 8)), rng.normal(size=8), rng.normal(size=(5, 8)), rng.normal(size=(3, 8))
    x = R.assemble(emb, cls, pos, reg)
    assert x.shape == (2, 8, 8)
    assert np.array_equal(x[:, 0], np.broadcast_to(cls + pos[0], (2, 8)))
    assert np.array_equal(x[:, 1:4], np.broadcast_to(reg, (2, 3, 8)))              # no position row
    assert np.array_equal(x[:, 4:], emb + pos[1:])
    assert np.array_equal(R.assemble(emb, cls, pos), np.concatenate([x[:, :1], x[:, 4:]], 1))


# ---- the converter ----------------------------------------------------------------------------------------------------------
CONV = dict(image_size=28, patch_size=14, channels=3, dim=64, heads=2, mlp_dim=128, layers=2, classes=8)


def _conv_sd(regs=2, unit_scale=False):
    return H.dinov2_state_dict(CONV, R.make_tensors(CONV, 71, REG(regs)), 71, unit_scale)


def test_converter_with_unit_layer_scale_gives_the_unfolded_tensors_bit_for_bit():
    t = R.make_tensors(CONV, 71, REG(2))
    blob = vithip.blob_from_dinov2_state_dict(_conv_sd(2, unit_scale=True), dict(CONV, registers=2))
    want = dict(t, **{"head.weight": np.zeros_like(t["head.weight"]), "head.bias": np.zeros_like(t["head.bias"])})
    assert np.array_equal(blob, R.pack_blob(CONV, want, REG(2)))                   # header included: eps 1e-6, count in bits 9 .. 13
    hw, hb = t["head.weight"], t["head.bias"]
    blob = vithip.blob_from_dinov2_state_dict(_conv_sd(2, unit_scale=True), dict(CONV, registers=2), head=(hw, hb))
    assert np.array_equal(blob, R.pack_blob(CONV, t, REG(2)))
    # no registers: a Dinov2Model state dict, today's blob layout
    blob0 = vithip.blob_from_dinov2_state_dict(_conv_sd(0, unit_scale=True), CONV, head=(hw, hb))
    assert np.array_equal(blob0, S.pack_blob(CONV, R.make_tensors(CONV, 71, 0)))


def test_converter_folds_layer_scale_in_float64_with_one_rounding():
    t = R.make_tensors(CONV, 71, REG(2))
    got = R.unpack_blob(CONV, vithip.blob_from_dinov2_state_dict(_conv_sd(2), dict(CONV, registers=2)), REG(2))
    for l in range(CONV["layers"]):
        l1, l2 = (a.astype(np.float64) for a in H.layer_scale(CONV, 71, l))
        assert 0.5 <= l1.min() and l1.max() <= 1.5 and l1.std() > 0.1              # non-trivial vectors
        for name, lam in (("o", l1), ("fc2", l2)):
            w = (t[f"l{l}.{name}.weight"].astype(np.float64) * lam[:, None]).astype(np.float32)
            b = (t[f"l{l}.{name}.bias"].astype(np.float64) * lam).astype(np.float32)
            assert np.array_equal(got[f"l{l}.{name}.weight"], w) and np.array_equal(got[f"l{l}.{name}.bias"], b)
            assert not np.array_equal(w, t[f"l{l}.{name}.weight"])
        for name in ("q", "k", "v", "fc1", "ln1", "ln2"):
            assert np.array_equal(got[f"l{l}.{name}.weight"], t[f"l{l}.{name}.weight"])
    assert np.array_equal(got["reg"], t["reg"]) and not got["head.weight"].any() and not got["head.bias"].any()


def test_converter_refusals():
    sd = _conv_sd(2)
    swiglu = dict(sd, **{"encoder.layer.0.mlp.weights_in.weight": np.zeros((256, 64), np.float32)})
    with pytest.raises(ValueError, match="SwiGLU"):
        vithip.blob_from_dinov2_state_dict(swiglu, dict(CONV, registers=2))
    with pytest.raises(ValueError, match=r"position_embeddings has 5 rows, cfg needs NP \+ 1 = 17"):
        vithip.blob_from_dinov2_state_dict(sd, dict(CONV, image_size=56, registers=2))
    with pytest.raises(ValueError, match=r"has 2 register tokens, cfg\['registers'\] is 4"):
        vithip.blob_from_dinov2_state_dict(sd, dict(CONV, registers=4))
    with pytest.raises(ValueError, match=r"has 2 register tokens, cfg\['registers'\] is 0"):
        vithip.blob_from_dinov2_state_dict(sd, CONV)
    with pytest.raises(ValueError, match=r"has 0 register tokens, cfg\['registers'\] is 2"):
        vithip.blob_from_dinov2_state_dict(_conv_sd(0), dict(CONV, registers=2))
    missing = {k: v for k, v in sd.items() if k != "encoder.layer.1.layer_scale2.lambda1"}
    with pytest.raises(KeyError, match="layer_scale2"):
        vithip.blob_from_dinov2_state_dict(missing, dict(CONV, registers=2))
    with pytest.raises(ValueError, match="head has shapes"):
        vithip.blob_from_dinov2_state_dict(sd, dict(CONV, registers=2), head=(np.zeros((8, 32)), np.zeros(8)))
    # mask_token is ignored: present or not, the same blob
    a = vithip.blob_from_dinov2_state_dict(sd, dict(CONV, registers=2))
    b = vithip.blob_from_dinov2_state_dict({k: v for k, v in sd.items() if "mask_token" not in k}, dict(CONV, registers=2))
    assert np.array_equal(a, b)
