"""The SwiGLU model switch on the host: VH_FLAG_SWIGLU is a valid setting beside the register, pooling, pre-LN and rotary bits; the blob's
fc1 doubles; the header carries bit 25; every excluded combination has its message; both DINO converters place, pad and fold what the
contract says once swiglu=True is given, and refuse as before without it.  The reference the GPU tests use, tests/swiglu_ref.py, is pinned
here against three fixtures computed by Hugging Face `transformers` in float64 (tests/golden/make_golden_swiglu.py).  The model bounds of
the GPU tests rest on two roundings more than a GELU model has (z as fc1 stores it, h once): their effect is measured here on the CPU.
No GPU needed.  (The named refusal of a blob whose bit differs from a CONTEXT's needs a context: tests/test_gpu_swiglu.py.)"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import swiglu_ref as W
import vh_synth as S
import vit_ref as R
from vh_testlib import lib_blob_bytes, rel

vithip = pytest.importorskip("vithip")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "swiglu", "*.npz")))
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
PRE, QUICK, REG, NO_CLS, POOL = vithip.FLAG_PRE_LN, vithip.FLAG_QUICK_GELU, vithip.FLAG_REGISTERS, vithip.FLAG_NO_CLS, vithip.FLAG_POOL
MAP, TANH, ROPE = vithip.FLAG_MAP_HEAD, vithip.FLAG_TANH_GELU, vithip.FLAG_ROPE
SWIGLU = getattr(vithip, "FLAG_SWIGLU", None)
VH_ERR_INVALID = 1
MICRO = S.CONFIGS["vit_micro"]
MID = dict(image_size=64, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=3, classes=40)
GIANT = dict(image_size=224, patch_size=14, channels=3, dim=1536, heads=24, mlp_dim=4096, layers=40, classes=1536)   # DINOv2-g/14
MODEL_TOL = {"fp16": 1e-3, "bf16": 1e-2}


def legal_flags():
    return [SWIGLU, SWIGLU | REG(4), SWIGLU | ROPE | REG(4), SWIGLU | PRE, SWIGLU | POOL(vithip.POOL_CLS_AVG),
            SWIGLU | NO_CLS | POOL(vithip.POOL_AVG_NORM), SWIGLU | NO_CLS | REG(2) | POOL(vithip.POOL_AVG_FCNORM)]


def _create_error(cfg, flags=0, dtype=BF16, max_batch=1):
    c = vithip.make_config(cfg, dtype, max_batch, 1e-6, flags)
    h = C.c_void_p()
    rc = vithip.lib().vh_create(C.byref(c), 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, vithip.lib().vh_last_error(None).decode()


def load(name):
    path, = [p for p in GOLDEN if os.path.basename(p).startswith(name + "_s")]
    return np.load(path)


def tensors64(name, z):
    return W.fixture_tensors64(name, z["rope_cos"], z["rope_sin"]) if "rope_cos" in z.files else W.fixture_tensors64(name)


# ---- header, table and ABI ----------------------------------------------------------------------------------------------------------
def test_the_macro_values():
    assert SWIGLU == 1 << 25 == W.FLAG_SWIGLU
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("#define VH_FLAG_SWIGLU (1 << 25)", "int vh_op_swiglu(", "#define VH_ABI_VERSION 1"):
        assert text in hdr, text
    assert "vh_op_swiglu" in vithip.SYMBOLS and callable(vithip.op_swiglu)
    assert vithip.lib().vh_abi_version() == 1


def test_table_sizes_and_blob_bytes():
    for cfg in (MICRO, MID, GIANT):
        D, M, L = cfg["dim"], cfg["mlp_dim"], cfg["layers"]
        for flags in legal_flags():
            assert W.legal(cfg, flags), flags
            shapes = {n: s for n, s, *_ in W.tensor_table(cfg, flags)}
            assert shapes["l0.fc1.weight"] == (2 * M, D) and shapes["l0.fc1.bias"] == (2 * M,) and shapes["l0.fc2.weight"] == (D, M)
            assert [(n, s) for n, s, *_ in W.tensor_table(cfg, flags)] == [(n, tuple(s)) for n, s in vithip.blob_tensor_table(cfg, flags)]
            without = R.blob_bytes(cfg, flags & ~SWIGLU)
            for more in (0, vithip.FLAG_LN_FOLD_ON, vithip.FLAG_LN_FOLD_OFF):
                assert lib_blob_bytes(cfg, flags | more) == without + L * (M * D + M) * 4 == W.blob_bytes(cfg, flags), (flags, more)
                assert lib_blob_bytes(cfg, flags & ~SWIGLU | more) == without
    # without the flag the table is vit_ref's, name for name
    assert W.tensor_table(MID, ROPE | REG(4)) == R.tensor_table(MID, ROPE | REG(4))


def test_layout_and_header_bit_of_a_packed_blob(tmp_path):
    for flags in legal_flags():
        blob = W.make_blob(MICRO, 9, flags, 1e-5)
        plain = R.make_blob(MICRO, 9, flags & ~SWIGLU, 1e-5)
        assert int(blob[52:56].view(np.uint32)[0]) == int(plain[52:56].view(np.uint32)[0]) | (1 << 25)
        assert vithip.blob_flags_of(blob) == flags
        t, t0 = W.unpack_blob(MICRO, blob, flags), R.unpack_blob(MICRO, plain, flags & ~SWIGLU)
        M = MICRO["mlp_dim"]
        for name in t:
            if ".fc1." in name:    # the same tensor id: the gate rows are the unflagged model's fc1, the value rows the stream's next values
                assert np.array_equal(t[name][:M], t0[name]) and not np.array_equal(t[name][M:], t0[name])
            else:
                assert np.array_equal(t[name], t0[name]), name
        assert np.array_equal(W.pack_blob(MICRO, t, flags, 1e-5), blob)
        path = tmp_path / f"m_{flags}.vhblob"
        blob.tofile(path)
        got, eps = vithip.blob_file_config(path)
        assert got == MICRO and abs(eps - 1e-5) < 1e-12 and vithip.blob_file_flags(path) == flags
    # forged: the bit over a blob without the longer tensors and the reverse -- the length gives both away
    path = tmp_path / "bad.vhblob"
    for blob, on in ((R.make_blob(MICRO, 5, 0), True), (W.make_blob(MICRO, 5, SWIGLU), False)):
        W.with_bit(blob, on).tofile(path)
        with pytest.raises(vithip.VhError, match="bytes, the header implies"):
            vithip.blob_file_config(path)


def test_refused_combinations_each_with_its_message():
    cases = ((SWIGLU | QUICK | PRE, BF16, "VH_FLAG_SWIGLU excludes VH_FLAG_QUICK_GELU and VH_FLAG_TANH_GELU"),
             (SWIGLU | TANH, BF16, "VH_FLAG_SWIGLU excludes VH_FLAG_QUICK_GELU and VH_FLAG_TANH_GELU"),
             (SWIGLU | MAP | NO_CLS, BF16, "VH_FLAG_SWIGLU excludes VH_FLAG_MAP_HEAD"),
             (SWIGLU | vithip.FLAG_CLS_TAIL, BF16, "VH_FLAG_SWIGLU excludes VH_FLAG_CLS_TAIL"),
             (SWIGLU | vithip.FLAG_W8_E4M3, FP16, "VH_FLAG_SWIGLU excludes VH_FLAG_W8_E4M3"),
             (SWIGLU | REG(4), FP8, "VH_FLAG_SWIGLU excludes VH_DTYPE_FP8"))
    for flags, dt, text in cases:
        assert lib_blob_bytes(MID, flags, dtype=dt) == 0, text
        rc, msg = _create_error(MID, flags, dtype=dt)
        assert rc == VH_ERR_INVALID and text in msg, msg
    assert not W.legal(MID, SWIGLU | TANH) and not W.legal(MID, SWIGLU | MAP | NO_CLS) and not W.legal(MID, SWIGLU | R.CLS_TAIL)
    # the pinned unknown bits stay unknown, alone and beside the new flag
    for bad in (1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 30, SWIGLU | (1 << 24), SWIGLU | (1 << 26), SWIGLU | REG(4) | (1 << 18)):
        assert lib_blob_bytes(MICRO, bad) == 0, bad
        assert "unknown bits in flags" in _create_error(MICRO, bad)[1]
    # what was refused is still refused beside the new bit, with its own message
    assert "VH_POOL_CLS reads the class token" in _create_error(MICRO, SWIGLU | NO_CLS)[1]


# ---- the converters -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_converter_places_pads_and_folds(name):
    kind, _, Mc, regs, *_ = W.FIXTURES[name]
    cfg, flags = W.fixture_cfg(name), W.fixture_flags(name)
    D, M = cfg["dim"], cfg["mlp_dim"]
    sd = W.fixture_state_dict(name)
    blob = W.fixture_blob(name)
    assert vithip.blob_flags_of(blob) == flags and blob.size == W.blob_bytes(cfg, flags) == lib_blob_bytes(cfg, flags)
    t, src = W.unpack_blob(cfg, blob, flags), W.fixture_model_tensors(name)
    assert (M > Mc) == (kind == "dinov2")
    for l in range(cfg["layers"]):
        w1, b1, w2, b2 = (t[f"l{l}.{n}"] for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
        # exact placement: gate rows first, value rows from row M on; the padding is zeros in all four places
        assert np.array_equal(w1[:Mc], src[f"l{l}.fc1.weight"]) and np.array_equal(w1[M:M + Mc], src[f"l{l}.up.weight"])
        assert np.array_equal(b1[:Mc], src[f"l{l}.fc1.bias"]) and np.array_equal(b1[M:M + Mc], src[f"l{l}.up.bias"])
        assert not w1[Mc:M].any() and not w1[M + Mc:].any() and not b1[Mc:M].any() and not b1[M + Mc:].any() and not w2[:, Mc:].any()
        # LayerScale folded into fc2 in float64, one rounding
        lam = np.asarray(W.lambdas(name, l)[1], np.float64)
        assert np.array_equal(w2[:, :Mc], (src[f"l{l}.fc2.weight"].astype(np.float64) * lam[:, None]).astype(np.float32))
        assert np.array_equal(b2, (src[f"l{l}.fc2.bias"].astype(np.float64) * lam).astype(np.float32))
        assert lam.std() > 0.2
    if kind == "dinov2":   # HF's rule for the hidden width: int(4 D * 2 / 3) rounded up to 8
        assert Mc == (int(4 * D * 2 / 3) + 7) // 8 * 8 and sd["encoder.layer.0.mlp.weights_in.weight"].shape == (2 * Mc, D)


def test_converter_refusals():
    conv2, conv3 = vithip.blob_from_dinov2_state_dict, vithip.blob_from_dinov3_state_dict
    sd2, cfg2, sd3, cfg3 = W.fixture_state_dict("a"), W.fixture_cfg("a"), W.fixture_state_dict("c"), W.fixture_cfg("c")
    # without the opt-in: the old messages, word for word
    with pytest.raises(ValueError, match=r"the checkpoint has a SwiGLU MLP \(mlp.weights_in\), which this library does not run"):
        conv2(sd2, cfg2)
    with pytest.raises(ValueError, match=r"the checkpoint has a gated MLP \(mlp.gate_proj\), which this library does not run"):
        conv3(sd3, cfg3, ln_eps=1e-5)
    # any other width mismatch: a smaller mlp_dim, a width that is a multiple of 64 under another mlp_dim
    with pytest.raises(ValueError, match="hidden width of 344, cfg\\['mlp_dim'\\] is 320"):
        conv2(sd2, dict(cfg2, mlp_dim=320), swiglu=True)
    with pytest.raises(ValueError, match="hidden width of 512, cfg\\['mlp_dim'\\] is 576"):
        conv3(sd3, dict(cfg3, mlp_dim=576), ln_eps=1e-5, swiglu=True)
    assert conv2(sd2, dict(cfg2, mlp_dim=448), swiglu=True).size == W.blob_bytes(dict(cfg2, mlp_dim=448), W.fixture_flags("a"))
    # both kinds of MLP in one state dict; a missing half
    with pytest.raises(ValueError, match="has both mlp.fc1 and a gated MLP"):
        conv2(dict(sd2, **{"encoder.layer.0.mlp.fc1.weight": np.zeros((8, 8), np.float32)}), cfg2, swiglu=True)
    with pytest.raises(ValueError, match="has both mlp.fc1 and a gated MLP"):
        conv3(dict(sd3, **{"model.layer.0.mlp.fc1.weight": np.zeros((8, 8), np.float32)}), cfg3, ln_eps=1e-5, swiglu=True)
    with pytest.raises(ValueError, match="swiglu=True, but the checkpoint has no mlp.weights_out"):
        conv2({k: v for k, v in sd2.items() if "weights_out" not in k}, cfg2, swiglu=True)
    for half in ("gate_proj", "up_proj", "down_proj"):
        with pytest.raises(ValueError, match=f"swiglu=True, but the checkpoint has no mlp.{half}"):
            conv3({k: v for k, v in sd3.items() if half not in k}, cfg3, ln_eps=1e-5, swiglu=True)
    with pytest.raises(KeyError, match="missing tensor model.layer.1.mlp.up_proj.bias"):
        conv3({k: v for k, v in sd3.items() if k != "model.layer.1.mlp.up_proj.bias"}, cfg3, ln_eps=1e-5, swiglu=True)
    with pytest.raises(ValueError, match="swiglu=True, but the checkpoint has no mlp.weights_in"):   # a plain checkpoint under the opt-in
        conv2({k.replace("weights_out", "fc2"): v for k, v in sd2.items() if "weights_in" not in k}, cfg2, swiglu=True)


# ---- numerics ------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_present():
    assert [os.path.basename(p).split("_s")[0] for p in GOLDEN] == ["a", "b", "c"], GOLDEN
    assert all(os.path.getsize(p) <= 300 * 1024 for p in GOLDEN)
    for name in "abc":
        z, cfg = load(name), W.fixture_cfg(name)
        _, _, Mc, regs, wseed, iseed, batch = W.FIXTURES[name]
        assert [int(v) for v in z["meta"]] == [wseed, iseed, batch, regs, Mc]
        assert [int(v) for v in z["config"]] == [cfg[k] for k in ("image_size", "patch_size", "channels", "dim", "heads", "mlp_dim", "layers", "classes")]
        assert np.array_equal(z["images"], W.fixture_images(name))
        sd = W.fixture_state_dict(name)
        assert abs(sum(float(np.asarray(v, np.float64).sum()) for v in sd.values()) - float(z["state_checksum"][0])) < 1e-9


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_reference_reproduces_the_fixtures(name):
    """The float64 reference on unrounded tensors against the model's own numbers (measured: a 3.9e-16, b 1.2e-15, c 1.2e-15, held to
    1e-12), and on the converted fp32 blob, whose LayerScale products are rounded once (measured: 2.7e-8, 2.5e-8, 5.7e-8, held to 1e-6).
    last_hidden_state is the final LayerNorm of every row."""
    z, cfg, flags, eps = load(name), W.fixture_cfg(name), W.fixture_flags(name), W.fixture_eps(name)
    t = tensors64(name, z)
    got, x = W.forward(cfg, t, z["images"], flags, eps, want_hidden=True)
    last = R.layernorm(x, t["lnf.weight"], t["lnf.bias"], eps).reshape(z["last_hidden_state"].shape)
    e_model, e_last = rel(got, z["pooler_output"]), rel(last, z["last_hidden_state"])
    e_blob = rel(W.forward(cfg, W.fixture_blob(name), z["images"], flags, eps), z["pooler_output"])
    print(f"\n[swiglu] fixture {name}: reference vs model {e_model:.3e} (rows {e_last:.3e}), converted blob vs model {e_blob:.3e}")
    assert e_model <= 1e-12 and e_last <= 1e-12 and e_blob <= 1e-6
    # and the gate matters: the value half alone (a model without the gate) is another function
    ungated = W.forward(cfg, {k: (np.concatenate([np.full_like(v[:len(v) // 2], 0), v[len(v) // 2:]]) if ".fc1." in k else v) for k, v in t.items()},
                        z["images"], flags, eps)
    assert rel(ungated, z["pooler_output"]) > 10 * MODEL_TOL["bf16"]


def test_gate_and_its_rounding_emulation():
    rng = np.random.default_rng(7)
    z = rng.standard_normal((5, 2 * 64)) * 4.0
    g, u = z[:, :64], z[:, 64:]
    assert np.allclose(W.gate(64)(z), g / (1 + np.exp(-g)) * u, rtol=1e-14, atol=0)
    assert np.array_equal(W.silu(np.array([0.0, -800.0, 800.0])), np.array([0.0, -0.0, 800.0]))
    for q in (R.fp16, R.bf16):
        z32 = z.astype(np.float32)
        zq = q(z32).astype(np.float32)
        want = q(W.silu(zq[:, :64]) * zq[:, 64:]).astype(np.float32)
        got = W.gate(64, q)(z32)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(q(got).astype(np.float32), got)          # h is a value of the storage type: rounded once, not twice


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_two_roundings_move_a_fixture_by_less_than_a_third_of_its_bound(name):
    """z as fc1 stores it and h rounded once, everything else float32, against the model's float64 output, as fractions of the project's
    bounds (fp16 1e-3, bf16 1e-2).  Measured: a 0.055 / 0.070, b 0.154 / 0.154, c 0.198 / 0.197.  More than a third: reseed the fixture."""
    z, cfg, flags, eps = load(name), W.fixture_cfg(name), W.fixture_flags(name), W.fixture_eps(name)
    blob = W.fixture_blob(name)
    base = rel(W.forward(cfg, blob, z["images"], flags, eps, dtype=np.float32), z["pooler_output"])
    for nm, q in (("fp16", R.fp16), ("bf16", R.bf16)):
        e = rel(W.forward(cfg, blob, z["images"], flags, eps, dtype=np.float32, q16=q), z["pooler_output"])
        print(f"\n[swiglu] fixture {name} {nm}: z and h rounded moves the output by {e:.3e} = {e / MODEL_TOL[nm]:.3f} of the bound (float32 alone: {base:.1e})")
        assert e <= MODEL_TOL[nm] / 3, (nm, e)
