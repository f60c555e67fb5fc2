"""VH_FLAG_SUB_LN on the host: the macro, the symbol and the header bit; the blob's three last tensors; every refusal by its message; the
EVA-02 converter's permutation, padding and width word; the reference against the three fixtures of tests/golden/eva02 (an independent
float64 restatement of the EVA-02 block with interleaved rotary pairs); the device's roundings emulated on the CPU.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import vithip

import subln_ref as U
import vit_ref as R
from subln_ref import fixture
from vh_testlib import lib_blob_bytes, rel

SUB_LN, SWIGLU, ROPE = getattr(vithip, "FLAG_SUB_LN", 0), vithip.FLAG_SWIGLU, vithip.FLAG_ROPE
MID = dict(image_size=64, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=3, classes=40)
MODEL_TOL = {"fp16": 1e-3, "bf16": 1e-2}
EPS = 1e-6


def create_error(cfg, flags):
    c, h = vithip.make_config(cfg, vithip.DTYPE_BF16, 1, EPS, flags), C.c_void_p()
    assert vithip.lib().vh_create(C.byref(c), 0, C.byref(h)) == 1 and not h.value
    return vithip.lib().vh_last_error(None).decode()


def test_macro_symbol_header_bit_and_blob_bytes():
    hdr = open(os.path.join(vithip.REPO_ROOT, "include", "vithip.h")).read()
    for text in ("#define VH_FLAG_SUB_LN (1 << 29)", "int vh_op_swiglu_ln(", "#define VH_ABI_VERSION 1"):
        assert text in hdr, text
    assert SUB_LN == 1 << 29 == U.FLAG_SUB_LN and "vh_op_swiglu_ln" in vithip.SYMBOLS and callable(vithip.op_swiglu_ln)
    for flags in (SWIGLU | SUB_LN, SWIGLU | SUB_LN | ROPE | vithip.FLAG_REGISTERS(4)):
        L, M = MID["layers"], MID["mlp_dim"]
        assert lib_blob_bytes(MID, flags) == lib_blob_bytes(MID, flags & ~SUB_LN) + (1 + 2 * L * M) * 4 == U.blob_bytes(MID, flags)
        assert [(n, tuple(s)) for n, s in vithip.blob_tensor_table(MID, flags)][-3:] == U.tensor_table(MID, flags)[-3:]
    blob = fixture("a")[3]
    assert int(blob[52:56].view(np.uint32)[0]) >> 29 & 1 and vithip.blob_flags_of(blob) & SUB_LN


@pytest.mark.parametrize("cfg,flags,text", [
    (MID, SUB_LN, "VH_FLAG_SUB_LN needs VH_FLAG_SWIGLU"), (MID, SUB_LN | ROPE, "VH_FLAG_SUB_LN needs VH_FLAG_SWIGLU"),
    (MID, SUB_LN | SWIGLU | vithip.FLAG_ATTN_BIAS, "VH_FLAG_SUB_LN excludes VH_FLAG_ATTN_BIAS"),
    (dict(MID, mlp_dim=4160), SUB_LN | SWIGLU, "VH_FLAG_SUB_LN needs mlp_dim <= 4096"),
    (MID, SUB_LN | SWIGLU | vithip.FLAG_TANH_GELU, "VH_FLAG_SWIGLU excludes VH_FLAG_QUICK_GELU and VH_FLAG_TANH_GELU")])
def test_refused_flag_combinations(cfg, flags, text):
    assert lib_blob_bytes(cfg, flags) == 0 and text in create_error(cfg, flags)


@pytest.mark.parametrize("word", [0.0, 385.0, 2.5])
def test_a_forged_width_word_is_refused(tmp_path, word):
    _, cfg, flags, blob, t = fixture("a")
    at = U.width_at(cfg, blob)
    assert blob[at:at + 4].view(np.float32)[0] == 344.0
    path = tmp_path / "m.vhblob"
    blob.tofile(path)
    assert vithip.blob_file_flags(path) == flags
    forged = blob.copy()
    forged[at:at + 4] = np.array([word], np.float32).view(np.uint8)
    forged.tofile(path)
    with pytest.raises(vithip.VhError, match=r"subln.width is [0-9.]+, not an integer in 1 .. mlp_dim = 384"):
        vithip.blob_file_config(path)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_converter_permutes_pads_and_writes_the_width(name):
    z, cfg, flags, blob, t = fixture(name)
    n, mean = U.FIXTURES[name][1:3]
    sd, D, M, hd = U.fixture_state_dict(name), cfg["dim"], cfg["mlp_dim"], cfg["dim"] // cfg["heads"]
    assert flags == ROPE | SWIGLU | SUB_LN | vithip.FLAG_POOL(vithip.POOL_AVG_FCNORM if mean else vithip.POOL_CLS)
    assert t["subln.width"][0] == n and M % (256 if name == "b" else 128) == 0 and M > n
    for l in range(cfg["layers"]):
        b = f"blocks.{l}."
        for x in "qk":    # row i of a head <- row 2 i, row hd / 2 + i <- row 2 i + 1; v stays
            w = t[f"l{l}.{x}.weight"].reshape(cfg["heads"], hd, D)
            src = sd[b + f"attn.{x}_proj.weight"].reshape(cfg["heads"], hd, D)
            assert np.array_equal(w[:, :hd // 2], src[:, 0::2]) and np.array_equal(w[:, hd // 2:], src[:, 1::2])
        assert np.array_equal(t[f"l{l}.q.bias"].reshape(-1, hd)[:, :hd // 2], sd[b + "attn.q_bias"].reshape(-1, hd)[:, 0::2])
        assert not t[f"l{l}.k.bias"].any() and np.array_equal(t[f"l{l}.v.weight"], sd[b + "attn.v_proj.weight"])
        w1, w2 = t[f"l{l}.fc1.weight"], t[f"l{l}.fc2.weight"]
        assert np.array_equal(w1[:n], sd[b + "mlp.fc1_g.weight"]) and np.array_equal(w1[M:M + n], sd[b + "mlp.fc1_x.weight"])
        assert np.array_equal(t["subln.weight"][l, :n], sd[b + "mlp.norm.weight"]) and np.array_equal(t["subln.bias"][l, :n], sd[b + "mlp.norm.bias"])
        pads = (w1[n:M], w1[M + n:], t[f"l{l}.fc1.bias"][n:M], t[f"l{l}.fc1.bias"][M + n:], w2[:, n:], t["subln.weight"][l, n:], t["subln.bias"][l, n:])
        assert not any(p.any() for p in pads)
    cos, sin = vithip.rope_tables_eva02(cfg["image_size"] // cfg["patch_size"], hd)
    assert np.array_equal(cos, z["rope_cos"].astype(np.float32)) and np.array_equal(t["rope.sin"], sin)
    fused = {k: v for k, v in sd.items() if "_proj.weight" not in k or "attn.proj" in k}     # the fused qkv form gives the same blob
    fused.update({f"blocks.{l}.attn.qkv.weight": np.concatenate([sd[f"blocks.{l}.attn.{x}_proj.weight"] for x in "qkv"]) for l in range(cfg["layers"])})
    assert np.array_equal(vithip.blob_from_eva02_state_dict(fused, cfg, EPS), blob)
    plain = vithip.blob_from_eva02_state_dict({k: v for k, v in sd.items() if "mlp.norm" not in k}, cfg, EPS)   # scale_mlp=False
    assert vithip.blob_flags_of(plain) == flags & ~SUB_LN and plain.size == lib_blob_bytes(cfg, flags & ~SUB_LN)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_reference_reproduces_the_fixture_and_the_roundings_stay_under_a_third_of_the_bounds(name):
    """The half-split rotation on the permuted rows against the interleaved-pair model: float64 on the fp32 blob within 1e-6 (the tables
    are rounded to fp32), on float64 tables within 1e-14 (measured: a 1.3e-15, b 1.2e-15).  Then z as fc1 stores it and h rounded once, everything else float32."""
    z, cfg, flags, blob, t = fixture(name)
    e32 = rel(U.forward(cfg, t, z["images"], flags, EPS), z["logits"])
    e64 = rel(U.forward(cfg, dict(t, **{"rope.cos": z["rope_cos"], "rope.sin": z["rope_sin"]}), z["images"], flags, EPS), z["logits"])
    print(f"\n[subln] fixture {name}: reference vs model {e64:.3e} (fp32 tables {e32:.3e})")
    assert e64 <= 1e-14 and e32 <= 1e-6
    assert rel(U.forward(cfg, dict(t, **{"subln.weight": np.ones_like(t["subln.weight"])}), z["images"], flags, EPS), z["logits"]) > 0.03
    for nm, q in (("fp16", R.fp16), ("bf16", R.bf16)):
        e = rel(U.forward(cfg, t, z["images"], flags, EPS, dtype=np.float32, q16=q), z["logits"])
        print(f"[subln] fixture {name} {nm}: z and h rounded moves the logits by {e:.3e} = {e / MODEL_TOL[nm]:.3f} of the bound")
        assert e <= MODEL_TOL[nm] / 3
