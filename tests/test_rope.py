"""The rotary model switch on the host: VH_FLAG_ROPE is a valid setting beside every other model bit except VH_FLAG_CLS_TAIL, the blob
gains rope.cos / rope.sin at its very end, the header carries bit 23, the refusals have their messages, and the DINOv3 converter and
its tables are what the contract says.  The reference the GPU tests use, tests/vit_ref.py, is pinned here on this flag against three fixtures
computed by Hugging Face `transformers` (DINOv3ViTModel in float64; tests/golden/make_golden_dinov3.py), which it misses with the flag
cleared.  The fp16 model bound of the GPU tests rests on one rounding of q and k more than any other model has: its effect is
measured here on the CPU.  No GPU needed.  (The named refusal of a blob whose bit differs from a CONTEXT's needs a context: it is in
tests/test_gpu_rope.py.)"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as HF
import vh_synth as S
import vit_ref as R
from vh_testlib import blob_digest, lib_blob_bytes, recorded_blob_digest, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "dinov3", "*.npz")))
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK, REG, NO_CLS, POOL = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU, vithip.FLAG_REGISTERS, vithip.FLAG_NO_CLS, vithip.FLAG_POOL
MAP, TANH, ROPE = vithip.FLAG_MAP_HEAD, vithip.FLAG_TANH_GELU, vithip.FLAG_ROPE
VH_ERR_INVALID = 1
MICRO = S.CONFIGS["vit_micro"]
MID = dict(image_size=64, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=3, classes=40)
HD80 = dict(image_size=48, patch_size=16, channels=3, dim=320, heads=4, mlp_dim=384, layers=2, classes=8)
LEGAL = [ROPE, ROPE | REG(4), ROPE | PRE | QUICK, ROPE | TANH, ROPE | POOL(vithip.POOL_CLS_AVG), ROPE | NO_CLS | POOL(vithip.POOL_AVG_NORM),
         ROPE | NO_CLS | REG(2) | POOL(vithip.POOL_AVG_FCNORM), ROPE | MAP | NO_CLS | TANH]


def _create_error(cfg, flags=0, dtype=BF16, max_batch=1):
    c = vithip.make_config(cfg, dtype, max_batch, 1e-6, flags)
    h = C.c_void_p()
    rc = vithip.lib().vh_create(C.byref(c), 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, vithip.lib().vh_last_error(None).decode()


def load(name):
    path, = [p for p in GOLDEN if os.path.basename(p).startswith(name + "_s")]
    return np.load(path)


def test_the_macro_values():
    assert ROPE == 1 << 23 == R.FLAG_ROPE
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("#define VH_FLAG_ROPE (1 << 23)", "int vh_op_rope(", "tensor id 0x7030", "#define VH_ABI_VERSION 1"):
        assert text in hdr, text
    assert "vh_op_rope" in vithip.SYMBOLS and R.TID_ROPE == 0x7030
    assert vithip.lib().vh_abi_version() == 1


def test_blob_bytes_with_and_without_the_flag():
    big = dict(image_size=224, patch_size=16, channels=3, dim=768, heads=12, mlp_dim=3072, layers=12, classes=768)
    for cfg in (MICRO, MID, HD80, big):
        NP, half = R.rope_shape(cfg)
        for flags in LEGAL:
            for more in (0, vithip.FLAG_W8_E4M3, vithip.FLAG_LN_FOLD_ON, vithip.FLAG_LN_FOLD_OFF):
                assert R.legal(cfg, flags), flags
                want = R.blob_bytes(cfg, flags & ~ROPE) + 2 * 4 * NP * half
                assert lib_blob_bytes(cfg, flags | more) == want == R.blob_bytes(cfg, flags), (flags, more)
                assert lib_blob_bytes(cfg, flags & ~ROPE | more) == R.blob_bytes(cfg, flags & ~ROPE)
    # without the flag: byte for byte what it was (the digests recorded before the flag's module was merged into vit_ref)
    for flags in [0] + [f & ~ROPE for f in LEGAL]:
        assert blob_digest(R.make_blob(MICRO, 5, flags)) == recorded_blob_digest("vit_micro", 5, flags), flags
    assert lib_blob_bytes(MID, ROPE | REG(4), dtype=FP8) == R.blob_bytes(MID, ROPE | REG(4))


def test_layout_of_the_blob():
    # the two tensors are the LAST ones, behind head.bias and behind the map.* tensors; no existing offset moves
    for flags in (ROPE | REG(4), ROPE | MAP | NO_CLS | TANH):
        names = [n for n, *_ in R.tensor_table(MICRO, flags)]
        assert names[-2:] == ["rope.cos", "rope.sin"] and names[-3] == ("map.fc2.bias" if flags & MAP else "head.bias")
        with_rope, without = R.make_blob(MICRO, 9, flags), R.make_blob(MICRO, 9, flags & ~ROPE)
        assert np.array_equal(with_rope[64:without.nbytes], without[64:])
        assert int(with_rope[52:56].view(np.uint32)[0]) == int(without[52:56].view(np.uint32)[0]) | (1 << 23)
        back, f0 = R.without_rope(MICRO, with_rope, flags)
        assert np.array_equal(back, without) and f0 == flags & ~ROPE
    t = R.make_tensors(MID, 9, ROPE)
    c, s = t["rope.cos"].astype(np.float64), t["rope.sin"].astype(np.float64)
    assert c.shape == s.shape == (64, 32)
    assert np.abs(c * c + s * s - 1.0).max() < 2e-7 and c.std() > 0.5 and s.std() > 0.5     # a true rotation, over the whole circle


def test_refusals_each_with_its_message():
    for f in (ROPE | vithip.FLAG_CLS_TAIL, ROPE | REG(4) | vithip.FLAG_CLS_TAIL):
        assert not R.legal(MICRO, f)
        assert lib_blob_bytes(MICRO, f) == 0
        rc, msg = _create_error(MICRO, f)
        assert rc == VH_ERR_INVALID and "VH_FLAG_ROPE excludes VH_FLAG_CLS_TAIL" in msg, msg
    # what was refused is still refused beside the new bit, with its own message
    assert "VH_FLAG_MAP_HEAD needs VH_FLAG_NO_CLS" in _create_error(MICRO, ROPE | MAP)[1]
    assert "VH_POOL_CLS reads the class token" in _create_error(MICRO, ROPE | NO_CLS)[1]
    # the pinned unknown bits stay unknown, alone and beside the new flag; so do the bits above it
    for bad in (64, 128, 256, 1 << 14, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 30, ROPE | (1 << 22), ROPE | (1 << 24), ROPE | REG(4) | (1 << 18)):
        assert lib_blob_bytes(MICRO, bad) == 0, bad
        assert "unknown bits in flags" in _create_error(MICRO, bad)[1]


def test_header_bit_round_trips_through_the_blob_file_entry_points(tmp_path):
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

    plain, rope = R.make_blob(MICRO, 5, 0), R.make_blob(MICRO, 5, ROPE)
    with_bits(plain, ROPE)                                 # the bit over a blob without the two tensors: the length gives it away
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    with_bits(rope, 0)                                     # and the reverse
    with pytest.raises(vithip.VhError, match="bytes, the header implies"):
        vithip.blob_file_config(path)
    for unknown in (8, 1 << 18, 1 << 20, 1 << 22, 1 << 24):   # header bit 3 and the neighbours of the new bit are still unknown
        with_bits(rope, ROPE | unknown)
        with pytest.raises(vithip.VhError, match="unknown bits in the header"):
            vithip.blob_file_config(path)
    with_bits(rope, ROPE)                                  # the bit alone is fine
    assert vithip.blob_file_flags(path) == ROPE


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["a", "b", "c"], GOLDEN
    assert all(os.path.getsize(p) <= 300 * 1024 for p in GOLDEN)
    for name in "abc":
        z, cfg = load(name), HF.fixture_cfg(name)
        _, regs, key_bias, wseed, iseed, batch = HF.FIXTURES[name]
        assert [int(v) for v in z["meta"]] == [wseed, iseed, batch, regs, int(key_bias)]
        assert [int(v) for v in z["config"]] == [cfg[k] for k in ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")]
        assert np.array_equal(z["images"], HF.fixture_images(name))
        sd = HF.dinov3_state_dict(name)
        assert abs(sum(float(np.asarray(v, np.float64).sum()) for v in sd.values()) - float(z["state_checksum"][0])) < 1e-9
        lam = np.concatenate([v for k, v in sd.items() if "lambda1" in k])
        assert lam.std() > 0.2 and lam.min() > 0.0           # a spread of LayerScale values, not the constant initial value


def test_rope_tables_against_the_models_own():
    """Against the values the Hugging Face module produced (stored in every fixture; A first).  Its coordinates and frequencies are
    float32: two relative errors of 2^-24 on an angle of at most 2 pi, 7.5e-7 absolute, plus our own rounding to fp32 (6e-8): 1e-6.
    Measured: A 3.3e-7, B 5.6e-8, C 3.7e-7."""
    for name in "abc":
        z, cfg = load(name), HF.fixture_cfg(name)
        g, hd = cfg["image_size"] // cfg["patch_size"], cfg["dim"] // cfg["heads"]
        cos, sin = vithip.rope_tables_dinov3(g, hd)
        assert cos.dtype == sin.dtype == np.float32 and cos.shape == sin.shape == (g * g, hd // 2)
        hc, hs = z["rope_cos"], z["rope_sin"]
        assert hc.shape == (g * g, hd) and np.array_equal(hc[:, :hd // 2], hc[:, hd // 2:]) and np.array_equal(hs[:, :hd // 2], hs[:, hd // 2:])
        err = max(np.abs(cos - hc[:, :hd // 2]).max(), np.abs(sin - hs[:, :hd // 2]).max())
        print(f"rope tables {name}: max |d| = {err:.3e}")
        assert err <= 1e-6
    # the formula itself, at one entry: patch (y, x) = (1, 3) of a 5 x 5 grid, hd 64, columns 2 (a y column) and 16 + 2 (an x column)
    cos, sin = vithip.rope_tables_dinov3(5, 64)
    for col, coord in ((2, 2 * 1.5 / 5 - 1), (18, 2 * 3.5 / 5 - 1)):
        a = 2 * np.pi * coord * 100.0 ** (-4 * 2 / 64)
        assert cos[1 * 5 + 3, col] == np.float32(np.cos(a)) and sin[1 * 5 + 3, col] == np.float32(np.sin(a))
    c2, _ = vithip.rope_tables_dinov3(5, 64, theta=10000.0)
    assert not np.array_equal(c2, cos)


def test_converter_layout_and_fold():
    for name in "abc":
        cfg, flags = HF.fixture_cfg(name), HF.fixture_flags(name)
        sd = HF.dinov3_state_dict(name)
        blob = HF.fixture_blob(name)
        assert vithip.blob_flags_of(blob) == flags and blob.nbytes == R.blob_bytes(cfg, flags) == lib_blob_bytes(cfg, flags)
        assert abs(float(blob[40:44].view(np.float32)[0]) - 1e-5) < 1e-12
        t = R.unpack_blob(cfg, blob, flags)
        t0 = HF.fixture_model_tensors(name)
        assert not t["pos"].any() and np.array_equal(t["head.weight"], np.eye(cfg["dim"], dtype=np.float32))
        cos, sin = vithip.rope_tables_dinov3(cfg["image_size"] // cfg["patch_size"], cfg["dim"] // cfg["heads"])
        assert np.array_equal(t["rope.cos"], cos) and np.array_equal(t["rope.sin"], sin)
        for l in range(cfg["layers"]):
            assert np.array_equal(t[f"l{l}.q.weight"], t0[f"l{l}.q.weight"]) and np.array_equal(t[f"l{l}.fc1.bias"], t0[f"l{l}.fc1.bias"])
            kb = t[f"l{l}.k.bias"]
            assert np.array_equal(kb, t0[f"l{l}.k.bias"]) if HF.FIXTURES[name][2] else not kb.any()       # key_bias=False: zeros
            for ours, i in (("o", 1), ("fc2", 2)):       # LayerScale folded in float64, one rounding
                lam = sd[f"model.layer.{l}.layer_scale{i}.lambda1"].astype(np.float64)
                assert np.array_equal(t[f"l{l}.{ours}.weight"], (t0[f"l{l}.{ours}.weight"].astype(np.float64) * lam[:, None]).astype(np.float32))
                assert np.array_equal(t[f"l{l}.{ours}.bias"], (t0[f"l{l}.{ours}.bias"].astype(np.float64) * lam).astype(np.float32))
        # `layer.N.` names give the same blob; the head is zero unless given; mask_token is ignored
        short = {k.replace("model.layer.", "layer."): v for k, v in sd.items() if k != "embeddings.mask_token"}
        D = cfg["dim"]
        assert np.array_equal(vithip.blob_from_dinov3_state_dict(short, cfg, head=(np.eye(D, dtype=np.float32), np.zeros(D, np.float32))), blob)
        zero = R.unpack_blob(cfg, vithip.blob_from_dinov3_state_dict(sd, cfg), flags)
        assert not zero["head.weight"].any() and not zero["head.bias"].any()
    cfg = HF.fixture_cfg("b")
    avg = vithip.blob_from_dinov3_state_dict(HF.dinov3_state_dict("b"), cfg, pool=vithip.POOL_AVG_NORM)
    assert vithip.blob_flags_of(avg) == ROPE | REG(4) | POOL(vithip.POOL_AVG_NORM)


def test_converter_refusals_by_name():
    cfg, sd = HF.fixture_cfg("b"), HF.dinov3_state_dict("b")
    conv = vithip.blob_from_dinov3_state_dict
    with pytest.raises(ValueError, match=r"gated MLP \(mlp.gate_proj\)"):
        conv(dict(sd, **{"model.layer.0.mlp.gate_proj.weight": np.zeros((cfg["mlp_dim"], cfg["dim"]), np.float32)}), cfg)
    with pytest.raises(ValueError, match=r"has 4 register tokens, cfg\['registers'\] is 2"):
        conv(sd, dict(cfg, registers=2))
    with pytest.raises(ValueError, match=r"has 0 register tokens, cfg\['registers'\] is 4"):
        conv({k: v for k, v in sd.items() if k != "embeddings.register_tokens"}, cfg)
    with pytest.raises(ValueError, match=r"model.layer.0.mlp.up_proj.weight has shape \(256, 128\), expected \(128, 128\)"):
        conv(sd, dict(cfg, mlp_dim=128))
    with pytest.raises(ValueError, match=r"embeddings.cls_token has shape"):
        conv(dict(sd, **{"embeddings.cls_token": np.zeros((1, 2, cfg["dim"]), np.float32)}), cfg)
    with pytest.raises(KeyError, match="model.layer.1.layer_scale2.lambda1"):
        conv({k: v for k, v in sd.items() if k != "model.layer.1.layer_scale2.lambda1"}, cfg)
    with pytest.raises(KeyError, match="model.layer.0.attention.q_proj.bias"):       # only the KEY bias may be absent
        conv({k: v for k, v in sd.items() if k != "model.layer.0.attention.q_proj.bias"}, cfg)
    with pytest.raises(ValueError, match="head has shapes"):
        conv(sd, cfg, head=(np.zeros((8, 32)), np.zeros(8)))
    with pytest.raises(ValueError, match="pool = 7"):
        conv(sd, cfg, pool=7)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_reference_reproduces_the_fixture(name):
    """vit_ref.forward in float64 against Hugging Face's float64 model, 1e-9 relative, on the model's own numbers: its own tables and
    the LayerScale product unrounded (hf_state_dicts.fixture_tensors64).  Measured 1e-15.  The CONVERTED blob differs from that model by what
    the blob format rounds to fp32 -- the folded o / fc2 weights (2^-24 relative each) and the tables (test_rope_tables_against_the_
    models_own) -- and reproduces the fixture to 1e-6 (measured: A 4.4e-8, B 2.9e-8, C 7.0e-8)."""
    z, cfg, flags = load(name), HF.fixture_cfg(name), HF.fixture_flags(name)
    t = HF.fixture_tensors64(name, z["rope_cos"], z["rope_sin"])
    logits, x = R.forward(cfg, t, z["images"], flags, HF.DINOV3_EPS, np.float64, want_hidden=True)
    last = R.final_norm(cfg, t, x, flags, HF.DINOV3_EPS).reshape(z["last_hidden_state"].shape)
    e = (rel(logits, z["pooler_output"]), rel(last, z["last_hidden_state"]))
    print(f"fixture {name}: float64 reference {e[0]:.3e} / {e[1]:.3e}")
    assert max(e) <= 1e-9
    blob = HF.fixture_blob(name)
    logits, x = R.forward(cfg, blob, z["images"], flags, HF.DINOV3_EPS, np.float64, want_hidden=True)
    last = R.final_norm(cfg, blob, x, flags, HF.DINOV3_EPS).reshape(z["last_hidden_state"].shape)
    e = (rel(logits, z["pooler_output"]), rel(last, z["last_hidden_state"]))
    print(f"fixture {name}: converted blob {e[0]:.3e} / {e[1]:.3e}")
    assert max(e) <= 1e-6


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_without_the_flag_the_fixture_is_missed(name):
    """The same model with FLAG_ROPE cleared (the blob minus its two tensors) is another function: measured A 0.16, B 0.29, C 0.28 of
    the output's largest magnitude, against fp16 / bf16 model bounds of 1e-3 / 1e-2 (ten times which the GPU test asks for)."""
    z, cfg, flags = load(name), HF.fixture_cfg(name), HF.fixture_flags(name)
    blob, f0 = R.without_rope(cfg, HF.fixture_blob(name), flags)
    assert f0 == flags & ~ROPE and blob.nbytes == R.blob_bytes(cfg, f0)
    e = rel(R.forward(cfg, blob, z["images"], f0, HF.DINOV3_EPS), z["pooler_output"])
    print(f"fixture {name}: flag cleared {e:.3e}")
    assert e > 0.15
    # the forward without the flag is the forward WITH it and the identity rotation (cos 1, sin 0), to the bit: one function, two paths
    t = dict(R.unpack_blob(cfg, blob, f0))
    t["rope.cos"], t["rope.sin"] = np.ones(R.rope_shape(cfg), np.float32), np.zeros(R.rope_shape(cfg), np.float32)
    assert rel(R.forward(cfg, t, z["images"], flags, HF.DINOV3_EPS), z["pooler_output"]) == e


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_extra_rounding_of_q_and_k_stays_inside_the_fp16_bound(name):
    """The GPU tests hold fp16 forwards of these fixtures to 1e-3; a ROPE model's q and k are rounded to fp16 twice (behind the
    projection, behind the rotation).  vit_ref in float32 with exactly those two roundings and nothing else rounded to 16 bits:
    measured A 1.9e-4, B 2.3e-4, C 2.1e-4 of the fixture (bf16, for the record: 1.6e-3, 1.6e-3, 1.9e-3 against its bound of 1e-2).  The
    device, which rounds every GEMM operand, measures 6.7e-4 / 4.7e-4 / 6.5e-4 in fp16 (tests/test_gpu_rope.py)."""
    z, cfg, flags = load(name), HF.fixture_cfg(name), HF.fixture_flags(name)
    blob = HF.fixture_blob(name)
    e16 = rel(R.forward(cfg, blob, z["images"], flags, HF.DINOV3_EPS, np.float32, q16=R.fp16), z["pooler_output"])
    eb = rel(R.forward(cfg, blob, z["images"], flags, HF.DINOV3_EPS, np.float32, q16=R.bf16), z["pooler_output"])
    print(f"fixture {name}: q and k rounded twice: fp16 {e16:.3e}, bf16 {eb:.3e}")
    assert e16 <= 1e-3 and eb <= 1e-2


def test_rotation_of_the_reference_is_the_stated_function():
    rng = np.random.default_rng(3)
    batch, T, H, dh, lead = 2, 7, 3, 32, 2
    qkv = rng.standard_normal((batch * T, 3 * H * dh))
    a = rng.uniform(-np.pi, np.pi, (T - lead, dh // 2))
    out = R.rotate_qkv(qkv, np.cos(a), np.sin(a), batch, T, H, dh, lead).reshape(batch, T, 3, H, dh)
    x = qkv.reshape(batch, T, 3, H, dh)
    assert np.array_equal(out[:, :lead], x[:, :lead]) and np.array_equal(out[:, :, 2], x[:, :, 2])
    b, p, w, h, d = 1, 3, 1, 2, 5
    c, s = np.cos(a[p, d]), np.sin(a[p, d])
    lo, hi = x[b, lead + p, w, h, d], x[b, lead + p, w, h, d + dh // 2]
    assert out[b, lead + p, w, h, d] == lo * c - hi * s and out[b, lead + p, w, h, d + dh // 2] == hi * c + lo * s
    # a rotation: norms of every (row, head) survive, and q . k of two rows depends on the DIFFERENCE of their angles
    assert np.allclose((out[:, :, :2] ** 2).sum(-1), (x[:, :, :2] ** 2).sum(-1), rtol=1e-12)
