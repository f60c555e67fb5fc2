"""CPU suite of the attention rollout (include/vithip.h, "Attention rollout"): the symbols and the descriptor, every refusal that is
reachable without a device, and the float64 reference on attn_exact's designs."""
import ctypes as C

import numpy as np
import pytest

import attn_exact as AX
import rollout_ref as RO
import vithip

VH_ERR_INVALID, VH_ERR_UNSUPPORTED = 1, 4
BF16 = vithip.DTYPE_BF16
QKV, R0, R1 = 0x10000, 0x4000000, 0x8000000   # never dereferenced: every call below is refused first


def test_symbols_and_descriptor_layout():
    for name in ("vh_set_rollout", "vh_get_rollout", "vh_rollout_dims", "vh_read_rollout", "vh_read_rollout_device", "vh_read_rollout_device_async",
                 "vh_op_rollout"):
        assert name in vithip.SYMBOLS and hasattr(vithip.lib(), name)
    F = vithip.Rollout
    assert C.sizeof(F) == 24 and [getattr(F, n).offset for n in ("out", "elem", "rows", "keys", "reserved")] == [0, 8, 12, 16, 20]
    assert (vithip.ROLLOUT_MEAN, vithip.ROLLOUT_MAX, vithip.ROLLOUT_MAX_TOKENS) == (0, 1, 640)


def tap(qkv=QKV, batch=2, tokens=65, heads=3, hd=64, dtype=BF16, fusion=RO.MEAN, r_prev=R0, r_new=R1, hm=0):
    vithip.op_rollout(qkv, batch, tokens, heads, hd, dtype, fusion, r_prev, r_new, hm)


REFUSALS = [   # (name, arguments, code, the refusal's own text): one list in the library, rollout_check's, with the arguments behind it
    ("null_qkv", dict(qkv=None), VH_ERR_INVALID, "null q|k|v or r_new"), ("null_r_new", dict(r_new=None), VH_ERR_INVALID, "null q|k|v or r_new"),
    ("batch_0", dict(batch=0), VH_ERR_INVALID, "batch must be positive"), ("tokens_0", dict(tokens=0), VH_ERR_INVALID, "tokens outside 1..640"),
    ("tokens_641", dict(tokens=641), VH_ERR_UNSUPPORTED, "at most 640"), ("hd_40", dict(hd=40), VH_ERR_INVALID, "head_dim must be 32, 48"),
    ("heads_0", dict(heads=0), VH_ERR_INVALID, "heads * head_dim outside"), ("heads_33", dict(heads=33), VH_ERR_INVALID, "heads * head_dim outside"),
    ("dtype_fp8", dict(dtype=vithip.DTYPE_FP8), VH_ERR_INVALID, "VH_DTYPE_BF16 or VH_DTYPE_FP16"), ("fusion_2", dict(fusion=2), VH_ERR_INVALID, "fusion is not"),
    ("head_major_at_80", dict(hd=80, hm=256), VH_ERR_INVALID, "head_dim 64 only"), ("hm_short", dict(hm=129), VH_ERR_INVALID, "fewer than batch * tokens"),
    ("misaligned_qkv", dict(qkv=QKV + 8), VH_ERR_INVALID, "qkv16 is not 16-byte aligned"), ("misaligned_r_prev", dict(r_prev=R0 + 2), VH_ERR_INVALID, "not 4-byte aligned"),
    ("misaligned_r_new", dict(r_new=R1 + 1), VH_ERR_INVALID, "not 4-byte aligned"), ("in_place", dict(r_prev=R1), VH_ERR_INVALID, "overlap"),
    ("overlap", dict(r_prev=R1 + 4), VH_ERR_INVALID, "overlap"),
]


@pytest.mark.parametrize("name,kw,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_tap_refuses_before_touching_a_device(name, kw, code, text):
    with pytest.raises(vithip.VhError) as e:
        tap(**kw)
    assert e.value.code == code and "rollout:" in str(e.value) and text in str(e.value), str(e.value)


def test_context_calls_fail_loudly_without_a_context():
    L = vithip.lib()
    desc = vithip.Rollout(None, vithip.ELEM_F32, 1, vithip.ATTN_KEYS_ALL, 0)
    for rc in (L.vh_set_rollout(None, 1, -1, 0), L.vh_get_rollout(None, None, None, None), L.vh_rollout_dims(None, None, None, None, None, None),
               L.vh_read_rollout(None, C.byref(desc)), L.vh_read_rollout_device(None, C.byref(desc)), L.vh_read_rollout_device_async(None, C.byref(desc))):
        assert rc == VH_ERR_INVALID and b"null context" in L.vh_last_error(None)


@pytest.mark.parametrize("fusion", [RO.MEAN, RO.MAX], ids=["mean", "max"])
def test_reference_on_the_uniform_design(fusion):
    """Every p is 1 / T, so every entry of A^ is (1 / T + delta) / 2."""
    B, T, H, hd = 2, 37, 3, 32
    a = RO.fused64(AX.make_case("uniform", B, T, H, hd, seed=3).qkv, B, T, H, hd, fusion)
    assert np.allclose(a, (1.0 / T + np.eye(T)) / 2, rtol=1e-14, atol=0)


def test_reference_on_the_permutation_design():
    """One head: A^ = (P_pi + I) / 2 up to 2^-32, and the chain is the product of those matrices: the permutations composed."""
    B, T, hd = 2, 21, 64
    cases = [AX.make_case("permutation", B, T, 1, hd, seed=s) for s in (4, 5, 6)]
    got = RO.chain64([c.qkv for c in cases], B, T, 1, hd, RO.MAX)
    for b in range(B):
        want = np.eye(T)
        for c in cases:
            want = ((np.eye(T)[c.pi[b, 0]] + np.eye(T)) / 2) @ want
        assert np.abs(got[b] - want).max() < 3 * 2.0 ** -30
        assert got[b][0, cases[0].pi[b, 0][cases[1].pi[b, 0][cases[2].pi[b, 0][0]]]] >= 0.125 - 2.0 ** -30   # pi_1(pi_2(pi_3(0))) carries 1/8
