"""GPU suite of the attention maps (include/vithip.h, "Attention maps").

OPERATOR TAPS, EXACT.  On attn_exact's designs every score is an exact integer, every e = 2^(s - m) an exact power of two and the row
sum exact in fp32 whatever its order (tokens <= 1024: 14 + 10 bits; `uniform`: l = tokens), so the capture kernel must write
np.float32(e) / np.float32(l) BIT FOR BIT (attn_maps_ref.exact32); the read-out kernel equals its numpy emulation bit for bit.

OPERATOR TAP, RANDOM DATA (test_probs_tap_random_data).  Per element |p - p_ref| <= REL * p_ref against the float64 softmax, with
    REL = 2 ln2 * (head_dim * 2^-24 * max_t sum_k |q_k k_tk|)  +  (tokens + 8) * 2^-24  +  2 * EXP2_MAX
-- the two dot-product errors that meet in s - m, the sum and the division, and the hardware exp2.  EXP2_MAX = 1.319e-07: no ISA
document at hand states v_exp_f32's accuracy, so it was measured once through this tap against float64 on a sweep of 4 033 arguments
in [-126, 0] (tools/attn_maps_bench.py, recorded in profiles/attn_maps.txt: 1.319e-07 = 2^-22.85, the two roundings of the measuring
quotient included); twice that maximum is used.  It is the instruction's property, not this code's.

CONTEXT LEVEL.  Logits keep their bits; an image's map has the same bits whatever the batch, the streams, eager or graph replay
and the q|k|v layout; against the float64 numpy model (attn_maps_ref.layer_probs64) max|p - p_ref| <= TOL[dtype], where TOL is four
times the largest value measured on the listed models (profiles/attn_maps_gpu_tests.txt) and must stay below 1 / (4 tokens), or a
uniform map could pass.  VH_DTYPE_FP8 needs dim % 128 == 0, which vit_mini (dim 192) is not: the fp8 cases are vit_micro's."""
import ctypes as C

import numpy as np
import pytest

import attn_exact as AX
import attn_maps_ref as AM
import vh_synth as S
import vit_ref as RR
import vithip
from layer_features_ref import Guarded
from vh_testlib import dev, _release_buffers  # noqa: F401  (autouse fixture: frees the buffers of a test)

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_UNSUPPORTED = 1, 3, 4
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
F32, F16, B16 = vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16
ALL, PATCH = vithip.ATTN_KEYS_ALL, vithip.ATTN_KEYS_PATCH
Q_CLS, Q_LEAD = vithip.ATTN_Q_CLS, vithip.ATTN_Q_LEAD
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
EXP2_MAX = 1.319e-07
BATCH = 3


# ---- operator taps -------------------------------------------------------------------------------------------------------------
def run_probs(qkv, batch, tokens, heads, hd, Q, dt, hm_rows=0):
    """The capture tap on fp32 values that are exact in `dt` -> fp32 [batch][heads][Q][tokens]; the output is a poisoned buffer with
    canaries on both sides, which the read checks."""
    b16 = vithip.to16(qkv, dt).reshape(qkv.shape)
    if hm_rows:
        b16 = vithip.pack_head_major(b16, heads, hm_rows, fill=0xFFFF)   # the padding rows are NaN in both 16-bit types
    out = Guarded(batch * heads * Q * tokens * 4)
    vithip.op_attention_probs(dev(b16).ptr, batch, tokens, heads, hd, Q, dt, out.ptr, hm_rows)
    got = out.read(np.float32, (batch, heads, Q, tokens))
    out.free()
    return got


def assert_bits(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = AM.bits(got) != AM.bits(want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} / {bad.size} elements differ in bits; first at [image, head, query, key] = {i}: "
                             f"got {got[i]!r}, want {want[i]!r}")


# (heads, head_dim, Q, tokens, dtype): every value of the issue's lists somewhere; tokens walk round the rows-per-instruction (4, 8, 16),
# the 4-deep load unroll and the 64- and 256-wide steps of the row passes
EXACT = [(1, 32, 1, 1, BF16), (3, 64, 1, 2, FP16), (3, 80, 5, 63, BF16), (1, 128, 17, 64, FP16), (3, 32, 17, 65, FP16), (3, 64, 5, 197, BF16),
         (1, 80, 17, 261, FP16), (3, 128, 5, 1024, BF16), (1, 64, 17, 1024, FP16), (3, 32, 5, 261, BF16), (3, 128, 1, 197, FP16),
         (1, 80, 1, 65, BF16), (3, 64, 17, 65, BF16)]
EXACT_IDS = [f"h{h}_hd{hd}_q{q}_t{t}_{NAME[dt]}" for h, hd, q, t, dt in EXACT]


@pytest.mark.parametrize("heads,hd,Q,tokens,dt", EXACT, ids=EXACT_IDS)
def test_probs_tap_exact(heads, hd, Q, tokens, dt):
    for design in AX.DESIGNS:
        if design == "permutation" and tokens > 197:   # beyond, the tail of the row sum no longer rounds away
            continue
        case = AX.make_case(design, BATCH, tokens, heads, hd, seed=7)
        want = AM.exact32(case.qkv, BATCH, tokens, heads, hd, Q)
        got = run_probs(case.qkv, BATCH, tokens, heads, hd, Q, dt)
        assert_bits(got, want, f"{design} row-major")
        if design == "uniform":
            assert (got == np.float32(1) / np.float32(tokens)).all()
        if design == "permutation":
            at = np.zeros(got.shape, dtype=bool)
            np.put_along_axis(at, case.pi[:, :, :Q, None], True, axis=-1)
            assert (got[at] == 1.0).all() and (got[~at] < 2.0 ** -31).all()
        if hd == 64:   # the head-major layout: more rows than the batch fills, the rest poisoned
            assert_bits(run_probs(case.qkv, BATCH, tokens, heads, hd, Q, dt, hm_rows=BATCH * tokens + 37), want, f"{design} head-major")


def test_probs_tap_at_4097_tokens():
    tokens, heads, hd, Q = 4097, 1, 64, 17
    case = AX.make_case("uniform", BATCH, tokens, heads, hd, seed=7)
    got = run_probs(case.qkv, BATCH, tokens, heads, hd, Q, BF16)
    assert (got == np.float32(1) / np.float32(4097)).all()


@pytest.mark.parametrize("heads,hd,Q,tokens,dt", [(3, 64, 5, 197, FP16), (3, 80, 17, 261, BF16), (1, 128, 1, 65, FP16), (3, 32, 5, 1024, BF16)],
                         ids=["hd64", "hd80", "hd128", "hd32"])
def test_probs_tap_random_data(heads, hd, Q, tokens, dt):
    """The bound of the module docstring, per element, against the float64 softmax."""
    rng = np.random.default_rng([3, heads, hd, tokens])
    D = heads * hd
    qkv = rng.standard_normal((BATCH * tokens, 3 * D)).astype(np.float32)
    qkv[:, :D] *= np.float32(9.0 / np.sqrt(hd))   # scores of standard deviation 9: magnitudes up to about 30
    qkv = vithip.from16(vithip.to16(qkv, dt), dt).reshape(qkv.shape)
    got = run_probs(qkv, BATCH, tokens, heads, hd, Q, dt).astype(np.float64)
    ref = AM.probs64(qkv, BATCH, tokens, heads, hd, Q)
    x = qkv.astype(np.float64).reshape(BATCH, tokens, 3, heads, hd)
    mag = np.einsum("bqhd,bthd->bhqt", np.abs(x[:, :Q, 0]), np.abs(x[:, :, 1])).max(-1, keepdims=True)
    rel = 2 * np.log(2) * hd * 2.0 ** -24 * mag + (tokens + 8) * 2.0 ** -24 + 2 * EXP2_MAX
    s = AM.scores(qkv, BATCH, tokens, heads, hd, Q)
    worst = float((np.abs(got - ref) / (rel * ref)).max())
    print(f"hd {hd} T {tokens} Q {Q} {NAME[dt]}: max|score| {np.abs(s).max():.1f}, worst |p - ref| / bound = {worst:.3f}, "
          f"max rel err {float((np.abs(got - ref) / ref).max()):.3e}, bound {float(rel.min()):.3e} .. {float(rel.max()):.3e}")
    assert np.isfinite(got).all() and worst <= 1.0


@pytest.mark.parametrize("elem", [F32, F16, B16], ids=["f32", "f16", "bf16"])
def test_readout_tap_equals_its_emulation(elem):
    B, H, Q, T, lead = 3, 3, 5, 41, 5
    rng = np.random.default_rng(9)
    e = np.exp2(rng.uniform(-20, 0, size=(B, H, Q, T)))
    store = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    sp = dev(store).ptr
    dt = AM.NP_DTYPE[elem]
    es = np.dtype(dt).itemsize
    got = {}
    for keys, K in ((ALL, T), (PATCH, T - lead)):
        po, mo = Guarded(B * H * Q * K * es), Guarded(B * Q * K * es)
        vithip.op_attention_readout(sp, B, H, Q, T, lead, elem, keys, po.ptr, mo.ptr)
        p, m = po.read(dt, (B, H, Q, K)), mo.read(dt, (B, Q, K))
        wp, wm = AM.readout(store, lead, elem, keys)
        assert AM.same_bits(p, wp) and AM.same_bits(m, wm), keys
        # either output alone
        vithip.op_attention_readout(sp, B, H, Q, T, lead, elem, keys, None, mo.ptr)
        assert AM.same_bits(mo.read(dt, (B, Q, K)), wm)
        got[keys] = (p, m)
        po.free(); mo.free()
    assert AM.same_bits(got[PATCH][0], np.ascontiguousarray(got[ALL][0][..., lead:])) and AM.same_bits(got[PATCH][1], np.ascontiguousarray(got[ALL][1][..., lead:]))
    if elem != F32:   # the RNE of exactly the fp32 output
        assert np.array_equal(got[ALL][0], vithip.to16(store, AM.ELEM_DTYPE[elem]))
        assert np.array_equal(got[ALL][1], vithip.to16(AM.readout(store, lead, F32, ALL)[1], AM.ELEM_DTYPE[elem]))


# ---- context level -------------------------------------------------------------------------------------------------------------
SEED, EPS = 11, 1e-6
MICRO, MINI = S.CONFIGS["vit_micro"], S.CONFIGS["vit_mini"]
HD80_MICRO = dict(image_size=64, patch_size=16, channels=3, dim=320, heads=4, mlp_dim=640, layers=2, classes=40)
REG4 = vithip.FLAG_REGISTERS(4)
NOCLS2 = vithip.FLAG_NO_CLS | vithip.FLAG_REGISTERS(2) | vithip.FLAG_POOL(vithip.POOL_AVG_NORM)
# name: (config, dtype, flags)
CASES = {
    "micro_bf16": (MICRO, BF16, 0), "micro_fp16": (MICRO, FP16, 0), "micro_fp8": (MICRO, FP8, 0),
    "micro_reg4_fp8": (MICRO, FP8, REG4),
    "mini_bf16": (MINI, BF16, 0), "mini_fp16": (MINI, FP16, 0),
    "mini_reg4_bf16": (MINI, BF16, REG4), "mini_reg4_fp16": (MINI, FP16, REG4),
    "mini_nocls_reg2_bf16": (MINI, BF16, NOCLS2), "mini_nocls_reg2_fp16": (MINI, FP16, NOCLS2),
    "hd80_bf16": (HD80_MICRO, BF16, 0), "hd80_fp16": (HD80_MICRO, FP16, 0),
}
ALL_CASES = list(CASES)
# max|p - p_ref| against the float64 model: four times the largest value seen per dtype over the cases below
# (profiles/attn_maps_gpu_tests.txt: fp16 1.739e-05 and bf16 1.334e-04 on hd80 layer 2, fp8 7.564e-04 on micro layer 2)
TOL = {FP16: 4 * 1.739e-05, BF16: 4 * 1.334e-04, FP8: 4 * 7.564e-04}
_models = {}


def model(case):
    """(config, model flags, blob) of a case; made once."""
    if case not in _models:
        cfg, _, flags = CASES[case]
        _models[case] = (cfg, flags, RR.make_blob(cfg, SEED, flags, EPS))
    return _models[case]


def make_ctx(case, max_batch=5, layers=None, queries=None, flags=0):
    cfg, dtype, mflags = CASES[case]
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=max_batch, flags=mflags | flags, ln_eps=EPS)
    ctx.load_weights(model(case)[2])
    if layers is not None:
        q = queries if queries is not None else Q_LEAD
        ctx.set_attention_layers(layers, q)
        assert ctx.attention_layers() == (list(layers), q)
    return ctx, cfg


def images_of(case, n, seed=1):
    return S.make_images(model(case)[0], seed, n)


def lead_of(case):
    cfg, flags, _ = model(case)
    return RR.tokens(cfg, flags) - (S.tokens(cfg) - 1)


@pytest.mark.parametrize("case", ["micro_bf16", "mini_reg4_fp16", "micro_fp8", "hd80_bf16", "mini_nocls_reg2_bf16"])
def test_logits_keep_their_bits(case):
    ctx, cfg = make_ctx(case)
    L = cfg["layers"]
    images = images_of(case, 3)
    want = ctx.forward(images)
    for lst in ([L], [1, L], list(range(1, L + 1))):
        ctx.set_attention_layers(lst, Q_LEAD)
        assert np.array_equal(ctx.forward(images), want), lst
        assert np.isfinite(ctx.read_attention(L)["probs"]).all()
    ctx.set_attention_layers([])
    assert ctx.attention_layers()[0] == [] and np.array_equal(ctx.forward(images), want)
    ctx.close()


@pytest.mark.parametrize("case", ALL_CASES)
def test_maps_do_not_depend_on_batch_streams_or_graph(case):
    ctx, cfg = make_ctx(case, layers=[1, cfg_layers(case)])
    L = cfg["layers"]
    images = images_of(case, 5)
    ctx.forward(images)
    want = {k: ctx.read_attention(k, head_mean=True) for k in (1, L)}
    b, h, q, t, n = ctx.attention_dims()
    assert (b, h, q, t) == (5, cfg["heads"], lead_of(case), RR.tokens(cfg, model(case)[1])) and want[L]["probs"].shape == (5, h, q, t)
    for i in (0, 3):   # batch 1 against the same image inside batch 5
        ctx.forward(images[i:i + 1])
        for k in (1, L):
            assert AM.same_bits(ctx.read_attention(k)["probs"], want[k]["probs"][i:i + 1]), (k, i)
    ctx.set_streams(3)   # parts of 2, 2 and 1 images
    ctx.forward(images)
    for k in (1, L):
        got = ctx.read_attention(k, head_mean=True)
        assert AM.same_bits(got["probs"], want[k]["probs"]) and AM.same_bits(got["head_mean"], want[k]["head_mean"]), k
    ctx.set_streams(1)
    other = images_of(case, 5, seed=2)
    ctx.forward(other)
    want_other = {k: ctx.read_attention(k)["probs"] for k in (1, L)}
    assert not AM.same_bits(want_other[L], want[L]["probs"])
    ctx.set_graph(True)   # the first forward at a batch is eager, the second is captured, the third replays; other images in between
    for rep in range(3):
        ctx.forward(other if rep == 1 else images)
        for k in (1, L):
            assert AM.same_bits(ctx.read_attention(k)["probs"], (want_other[k] if rep == 1 else want[k]["probs"])), (k, rep)
    assert ctx.get_graph() == (True, 1)
    ctx.close()


def cfg_layers(case):
    return CASES[case][0]["layers"]


def test_maps_do_not_depend_on_the_qkv_layout(monkeypatch):
    """ViT-B/16 bf16 at batch 224 keeps q|k|v head-major (173 row tiles x 3 >= 512); a context created under VH_QKV_HM=0 keeps it
    row-major.  The same maps, bit for bit; debug tap 4 says which layout each forward took."""
    cfg = S.CONFIGS["vit_base"]
    batch = 224
    px = cfg["image_size"] ** 2 * cfg["channels"]
    din, dout = vithip.DeviceBuffer(batch * px * 4), vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    maps, used, logits = [], [], []
    for hm in ("1", "0"):
        monkeypatch.setenv("VH_QKV_HM", hm)
        ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=batch)
        ctx.init_weights_seeded(0)
        ctx.set_attention_layers([1, cfg["layers"]], Q_CLS)
        ctx.fill_input_seeded(1, batch, din.ptr)
        ctx.forward_device(din.ptr, batch, dout.ptr)
        used.append(int(ctx.debug_read(4, 1)[0]))
        maps.append([ctx.read_attention(k)["probs"] for k in (1, cfg["layers"])])
        logits.append(dout.to_numpy(np.float32, (batch, cfg["classes"])))
        ctx.close()
    din.free(); dout.free()
    assert used == [1, 0], used
    assert np.array_equal(logits[0], logits[1])
    for a, b in zip(*maps):
        assert a.shape == (batch, 12, 1, 197) and np.isfinite(a).all() and AM.same_bits(a, b)
        assert np.abs(a.astype(np.float64).sum(-1) - 1).max() <= (197 + 8) * 2.0 ** -24


@pytest.mark.parametrize("case", ALL_CASES)
def test_maps_against_the_numpy_model(case):
    cfg, dtype, _ = CASES[case]
    _, flags, blob = model(case)
    L, T = cfg["layers"], RR.tokens(cfg, flags)
    ctx, _ = make_ctx(case, layers=list(range(1, L + 1)))
    images = images_of(case, 3)
    ctx.forward(images)
    Q = ctx.attention_dims()[2]
    _, _, hidden = RR.forward(cfg, blob, images, flags, ln_eps=EPS, all_hidden=True)
    worst = 0.0
    for k in range(1, L + 1):
        got = ctx.read_attention(k)["probs"]
        ref = AM.layer_probs64(cfg, blob, hidden, k, 3, Q, flags, EPS)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err)
        print(f"{case} layer {k}: max|p - p_ref| = {err:.3e} (max p_ref {ref.max():.3f}, tol {TOL[dtype]:.3e}, 1 / (4 tokens) = {1 / (4 * T):.3e})")
        # rows: they sum to 1 within the sum's and the division's roundings
        assert np.abs(got.astype(np.float64).sum(-1) - 1).max() <= (T + 8) * 2.0 ** -24, k
    ctx.close()
    assert TOL[dtype] < 1 / (4 * T)
    assert worst <= TOL[dtype], (worst, TOL[dtype])


@pytest.mark.parametrize("case", ["mini_reg4_bf16", "micro_reg4_fp8", "hd80_fp16"])
def test_rows_and_layer_aliases(case):
    ctx, cfg = make_ctx(case, layers=[cfg_layers(case)], queries=Q_LEAD)
    L = cfg["layers"]
    images = images_of(case, 2)
    ctx.forward(images)
    lead = ctx.read_attention(L)["probs"]
    assert AM.same_bits(ctx.read_attention(-1)["probs"], lead)
    ctx.set_attention_layers([L], Q_CLS)
    ctx.forward(images)
    cls = ctx.read_attention(-1)["probs"]
    assert cls.shape[2] == 1 and AM.same_bits(cls[:, :, 0], np.ascontiguousarray(lead[:, :, 0]))
    # the read-out forms: host against device, 16-bit = RNE of fp32, the patch columns, the head mean
    full = ctx.read_attention(L, head_mean=True)
    for elem in (F32, F16, B16):
        for keys in (ALL, PATCH):
            wp, wm = AM.readout(full["probs"], lead_of(case), elem, keys)
            got = ctx.read_attention(L, head_mean=True, elem=elem, keys=keys)
            assert AM.same_bits(got["probs"], wp) and AM.same_bits(got["head_mean"], wm), (elem, keys)
    b, h, q, t, n = ctx.attention_dims()
    po, mo = Guarded(b * h * q * n * 2), Guarded(b * q * n * 2)
    for call in (ctx.read_attention_device, ctx.read_attention_device_async):
        call(vithip.AttentionMaps(po.ptr, mo.ptr, F16, L, PATCH, 0))
        ctx.synchronize()
        wp, wm = AM.readout(full["probs"], lead_of(case), F16, PATCH)
        assert AM.same_bits(po.read(np.uint16, wp.shape), wp) and AM.same_bits(mo.read(np.uint16, wm.shape), wm)
    po.free(); mo.free()
    # cls_attention: DINO's attentions[:, :, 0, 1:] reshaped
    g = cfg["image_size"] // cfg["patch_size"]
    ca = ctx.cls_attention(reshape=True)
    assert ca.shape == (2, h, g, g) and AM.same_bits(ca.reshape(2, h, g * g), np.ascontiguousarray(ctx.read_attention(L, keys=PATCH)["probs"][:, :, 0]))
    assert AM.same_bits(ctx.cls_attention(reshape=False), np.ascontiguousarray(cls[:, :, 0]))
    ctx.close()


def test_cls_attention_sets_the_list_itself():
    ctx, cfg = make_ctx("micro_fp16")
    images = images_of("micro_fp16", 2)
    ctx.forward(images)
    with pytest.raises(vithip.VhError) as e:   # the list is set here; no forward has run since
        ctx.cls_attention()
    assert e.value.code == VH_ERR_STATE and ctx.attention_layers() == ([cfg["layers"]], Q_CLS)
    ctx.forward(images)
    assert ctx.cls_attention().shape == (2, cfg["heads"], 4, 4)
    ctx.close()


@pytest.mark.parametrize("case", ["mini_fp16", "mini_reg4_bf16"])
def test_truncated_forwards(case):
    ctx, cfg = make_ctx(case, layers=[1, 2, cfg_layers(case)])
    L = cfg["layers"]
    images = images_of(case, 3)
    ctx.forward(images)
    want = {k: ctx.read_attention(k)["probs"] for k in (1, 2)}
    ctx.debug_set_layers(2)
    ctx.forward(images)
    for k in (1, 2):
        assert AM.same_bits(ctx.read_attention(k)["probs"], want[k]), k
    for layer in (L, -1):
        with pytest.raises(vithip.VhError) as e:
            ctx.read_attention(layer)
        assert e.value.code == VH_ERR_STATE and "did not reach" in str(e.value)
    ctx.close()


def test_refusals():
    case = "mini_reg4_fp16"
    ctx, cfg = make_ctx(case, layers=[1, 3])
    L, lib = cfg["layers"], vithip.lib()
    T = RR.tokens(cfg, model(case)[1])
    host = np.full((2, cfg["heads"], 5, T), np.float32(-7.0))
    mean = np.full((2, 5, T), np.float32(-7.0))
    dbuf = Guarded(host.nbytes)

    def read(code, text, probs=True, head_mean=True, elem=F32, layer=-1, keys=ALL, reserved=0, device=None):
        if device is None:
            desc = vithip.AttentionMaps(host.ctypes.data if probs else None, mean.ctypes.data if head_mean else None, elem, layer, keys, reserved)
            calls = (lib.vh_read_attention,)
        else:
            desc = vithip.AttentionMaps(device, None, elem, layer, keys, reserved)
            calls = (lib.vh_read_attention_device, lib.vh_read_attention_device_async)
        for call in calls:
            assert call(ctx.h, C.byref(desc)) == code, text
            assert text in lib.vh_last_error(ctx.h).decode(), lib.vh_last_error(ctx.h).decode()
        assert (host == -7.0).all() and (mean == -7.0).all() and dbuf.untouched()

    read(VH_ERR_STATE, "no forward has run")
    ctx.forward(images_of(case, 2))
    assert lib.vh_read_attention(ctx.h, None) == VH_ERR_INVALID and "null descriptor" in lib.vh_last_error(ctx.h).decode()
    read(VH_ERR_INVALID, "no output requested", probs=False, head_mean=False)
    read(VH_ERR_INVALID, "elem", elem=vithip.ELEM_U8)
    read(VH_ERR_INVALID, "keys", keys=2)
    read(VH_ERR_INVALID, "layer 0", layer=0)
    read(VH_ERR_INVALID, f"layer {L + 1}", layer=L + 1)
    read(VH_ERR_INVALID, "reserved", reserved=1)
    read(VH_ERR_INVALID, "16-byte aligned", device=dbuf.ptr + 8)
    read(VH_ERR_STATE, "was not in the list", layer=2)
    read(VH_ERR_STATE, "was not in the list", layer=2, device=dbuf.ptr)
    # a refused set call leaves the list in force
    for bad, q, code in (([3, 1], Q_LEAD, VH_ERR_INVALID), ([0], Q_LEAD, VH_ERR_INVALID), ([L + 1], Q_LEAD, VH_ERR_INVALID), ([1], 2, VH_ERR_INVALID),
                         (list(range(1, 66)), Q_LEAD, VH_ERR_INVALID)):
        with pytest.raises(vithip.VhError) as e:
            ctx.set_attention_layers(bad, q)
        assert e.value.code == code and "set_attention_layers" in str(e.value)
    assert ctx.attention_layers() == ([1, 3], Q_LEAD)
    assert np.isfinite(ctx.read_attention(3)["probs"]).all()   # and the last forward's maps are still there
    # a new list clears what the last forward captured
    ctx.set_attention_layers([2], Q_CLS)
    read(VH_ERR_STATE, "was not in the list", layer=2)
    # a ring
    ctx.ring_create(2, 1)
    read(VH_ERR_STATE, "a ring exists")
    with pytest.raises(vithip.VhError) as e:
        ctx.set_attention_layers([1])
    assert e.value.code == VH_ERR_STATE
    dbuf.free()
    ctx.close()


def test_refusals_by_kind_of_context():
    # the class-token tail's last layer runs another kernel
    ctx, cfg = make_ctx("micro_bf16", flags=vithip.FLAG_CLS_TAIL)
    with pytest.raises(vithip.VhError) as e:
        ctx.set_attention_layers([1])
    assert e.value.code == VH_ERR_UNSUPPORTED and "VH_FLAG_CLS_TAIL" in str(e.value)
    ctx.forward(images_of("micro_bf16", 1))
    with pytest.raises(vithip.VhError) as e:
        ctx.read_attention()
    assert e.value.code == VH_ERR_UNSUPPORTED
    ctx.close()
    # no class token: Q_CLS has no row
    ctx, cfg = make_ctx("mini_nocls_reg2_bf16")
    with pytest.raises(vithip.VhError) as e:
        ctx.set_attention_layers([1], Q_CLS)
    assert e.value.code == VH_ERR_INVALID and "VH_FLAG_NO_CLS" in str(e.value)
    ctx.set_attention_layers([1], Q_LEAD)
    ctx.forward(images_of("mini_nocls_reg2_bf16", 1))
    assert ctx.read_attention(1)["probs"].shape[2] == 2
    ctx.close()
    # no class token and no registers: no leading rows at all
    flags = vithip.FLAG_NO_CLS | vithip.FLAG_POOL(vithip.POOL_AVG_NORM)
    ctx = vithip.VitContext(MICRO, dtype=BF16, max_batch=1, flags=flags, ln_eps=EPS)
    ctx.load_weights(RR.make_blob(MICRO, SEED, flags, EPS))
    for q in (Q_CLS, Q_LEAD):
        with pytest.raises(vithip.VhError) as e:
            ctx.set_attention_layers([1], q)
        assert e.value.code == VH_ERR_INVALID
    assert "leading rows" in str(e.value)
    ctx.close()
