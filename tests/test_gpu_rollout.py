"""GPU suite of the attention rollout (include/vithip.h, "Attention rollout"): vh_op_rollout against the float64 reference
(rollout_ref), then the context against the tap and against the float64 model."""
import ctypes as C

import numpy as np
import pytest

import attn_exact as AX
import attn_maps_ref as AM
import rollout_ref as RO
import vh_synth as S
import vit_ref as RR
import vithip
from layer_features_ref import Guarded
from vh_testlib import dev, _release_buffers  # noqa: F401  (autouse fixture: frees the buffers of a test)

pytestmark = pytest.mark.gpu

VH_ERR_INVALID, VH_ERR_STATE, VH_ERR_UNSUPPORTED = 1, 3, 4
BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
F32, F16, B16 = vithip.ELEM_F32, vithip.ELEM_F16, vithip.ELEM_BF16
ALL, PATCH = vithip.ATTN_KEYS_ALL, vithip.ATTN_KEYS_PATCH
NAME = {BF16: "bf16", FP16: "fp16"}
# max|d| / max|ref| per image against float64 on real values.  The hardware exp2 and the MFMA summation order are not specified for
# bits, so the bound is 4 x the worst ratio measured on the MI355X over REAL below, 5.264e-06 (T 640, one head of 128, fp16;
# profiles/rollout_gpu_tests.txt).  A leaked padded key or a dropped key shifts a row by about 1 / T: it must stay below 1 / (8 * 640).
BOUND = 4 * 5.264e-06
# the context against the float64 MODEL adds the 16-bit forward's own distance: 4 x the worst ratio measured on the models of test_context
MODEL_BOUND = {BF16: BOUND + 4 * 1.013e-04, FP16: BOUND + 4 * 1.043e-05}


def run_step(qkv, batch, tokens, heads, hd, dt, fusion, r_prev=None, hm_rows=0):
    """The tap on fp32 values that are exact in `dt` -> fp32 [batch][tokens][tokens], written into a poisoned buffer with canaries."""
    b16 = vithip.to16(qkv, dt).reshape(qkv.shape)
    if hm_rows:
        b16 = vithip.pack_head_major(b16, heads, hm_rows, fill=0xFFFF)   # the padding rows are NaN in both 16-bit types
    out = Guarded(batch * tokens * tokens * 4)
    prev = None if r_prev is None else dev(np.ascontiguousarray(r_prev, dtype=np.float32)).ptr
    vithip.op_rollout(dev(b16).ptr, batch, tokens, heads, hd, dt, fusion, prev, out.ptr, hm_rows)
    got = out.read(np.float32, (batch, tokens, tokens))
    out.free()
    return got


def ratio(got, want):
    return max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want))


@pytest.mark.parametrize("tokens,heads,hd,dt", [(64, 2, 32, BF16), (128, 4, 80, FP16), (128, 2, 64, BF16)], ids=["t64", "t128_hd80", "t128_hd64"])
@pytest.mark.parametrize("fusion", [RO.MEAN, RO.MAX], ids=["mean", "max"])
def test_exact(tokens, heads, hd, dt, fusion):
    """`uniform` at a power-of-two T: p = 1 / T, A^ = (1 / T + delta) / 2; with R_prev = k / 256 every product and partial sum is a dyadic
    number of at most 17 bits, so R_new equals the float64 reference BIT FOR BIT whatever the summation order."""
    B = 2
    case = AX.make_case("uniform", B, tokens, heads, hd, seed=5)
    i, j, b = np.ogrid[:tokens, :tokens, :B]
    r_prev = np.ascontiguousarray((((7 * i + 13 * j + 5 * b + i * j) % 256) / 256.0).transpose(2, 0, 1))
    for prev in (None, r_prev):
        want = RO.step64(case.qkv, B, tokens, heads, hd, fusion, prev)
        for hm in ((0, B * tokens + 37) if hd == 64 else (0,)):
            got = run_step(case.qkv, B, tokens, heads, hd, dt, fusion, prev, hm)
            bad = np.argwhere(got.astype(np.float64) != want)
            assert not len(bad), f"{len(bad)} elements differ, first at [image, row, column] = {bad[0]}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("tokens", [5, 63, 65, 197])
def test_permutation_chain(tokens):
    """Three chained steps of `permutation` with a permutation per head, max fusion: A = (the union of the heads' permutation matrices)
    + I.  BOUND, derived: every off-target probability is below 2^-32 here and in the reference alike.  Per step and entry the kernel
    adds the rounding of p and of 1 / l (a few 2^-24, relative to values <= 1), T additions into a row sum <= heads + 1 and T
    multiply-adds into a partial sum <= 1 (R is row-stochastic and A^ too), each 2^-24, and one division: below (T + 8) * 2^-23.  A^
    is row-stochastic, so a step does not amplify the error it inherits: steps * (T + 8) * 2^-23 per entry."""
    B, H, hd, steps = 2, 3, 64, 3
    cases = [AX.make_case("permutation", B, tokens, H, hd, seed=20 + s) for s in range(steps)]
    got = None
    for c in cases:
        got = run_step(c.qkv, B, tokens, H, hd, BF16, RO.MAX, got)
    err = float(np.abs(got - RO.chain64([c.qkv for c in cases], B, tokens, H, hd, RO.MAX)).max())
    print(f"T {tokens}: max|d| = {err:.3e}, bound {steps * (tokens + 8) * 2.0 ** -23:.3e}")
    assert np.isfinite(got).all() and err <= steps * (tokens + 8) * 2.0 ** -23


# (tokens, heads, head_dim, batch, dtype, head-major): every size at which the kernel takes another path -- one query block and
# several, key tails, the four accumulator widths (<= 64, 256, 448, 640 tokens), padded and whole k-steps
REAL = [(1, 1, 32, 1, BF16, 0), (5, 3, 64, 3, FP16, 1), (63, 3, 80, 2, BF16, 0), (64, 12, 64, 1, FP16, 0), (65, 3, 128, 2, BF16, 0),
        (197, 12, 64, 2, BF16, 1), (261, 3, 32, 1, FP16, 0), (640, 3, 64, 1, BF16, 0), (640, 1, 128, 1, FP16, 0)]


@pytest.mark.parametrize("tokens,heads,hd,batch,dt,hm", REAL, ids=[f"t{t}_h{h}_hd{d}_b{b}_{NAME[dt]}{'_hm' if hm else ''}" for t, h, d, b, dt, hm in REAL])
def test_real_values(tokens, heads, hd, batch, dt, hm):
    """One step from a random row-stochastic R_prev, and a chain of four, both fusions."""
    rng = np.random.default_rng([17, tokens, heads, hd])
    D = heads * hd
    qkvs = []
    for _ in range(2):
        qkv = rng.standard_normal((batch * tokens, 3 * D)).astype(np.float32)
        qkv[:, :D] *= np.float32(2.75 / np.sqrt(hd))   # scores of standard deviation 2.75: inside +-16
        qkvs.append(vithip.from16(vithip.to16(qkv, dt), dt).reshape(qkv.shape))
    assert np.abs(AM.scores(qkvs[0], batch, tokens, heads, hd, tokens)).max() < 16
    r0 = rng.random((batch, tokens, tokens)) ** 4
    r0 = (r0 / r0.sum(-1, keepdims=True)).astype(np.float32)
    hm_rows = batch * tokens + 11 if hm else 0
    worst = 0.0
    for fusion in (RO.MEAN, RO.MAX):
        got = run_step(qkvs[0], batch, tokens, heads, hd, dt, fusion, r0, hm_rows)
        chain = None
        for k in range(4):
            chain = run_step(qkvs[k & 1], batch, tokens, heads, hd, dt, fusion, chain, hm_rows)
        assert np.isfinite(got).all() and np.isfinite(chain).all()
        worst = max(worst, ratio(got, RO.step64(qkvs[0], batch, tokens, heads, hd, fusion, r0)),
                    ratio(chain, RO.chain64([qkvs[k & 1] for k in range(4)], batch, tokens, heads, hd, fusion)))
    print(f"T {tokens} heads {heads} hd {hd} {NAME[dt]}: worst max|d| / max|ref| = {worst:.3e} (bound {BOUND:.3e})")
    assert BOUND < 1.0 / (8 * 640) and worst <= BOUND


# ---- context level -------------------------------------------------------------------------------------------------------------
SEED, EPS = 11, 1e-6
MICRO = S.CONFIGS["vit_micro"]
REG_ROPE = vithip.FLAG_REGISTERS(4) | vithip.FLAG_ROPE


def make_ctx(flags, dt, max_batch=3):
    blob = RR.make_blob(MICRO, SEED, flags, EPS)
    ctx = vithip.VitContext(MICRO, dtype=dt, max_batch=max_batch, flags=flags, ln_eps=EPS)
    ctx.load_weights(blob)
    return ctx, blob


@pytest.mark.parametrize("fusion", [RO.MEAN, RO.MAX], ids=["mean", "max"])
@pytest.mark.parametrize("flags", [0, REG_ROPE], ids=["plain", "reg4_rope"])
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_context(flags, dt, fusion):
    ctx, blob = make_ctx(flags, dt)
    L, H, hd, D, T = MICRO["layers"], MICRO["heads"], MICRO["dim"] // MICRO["heads"], MICRO["dim"], RR.tokens(MICRO, flags)
    lead, images = T - (S.tokens(MICRO) - 1), S.make_images(MICRO, 1, 3)
    logits = ctx.forward(images)
    qkvs = []   # the per-layer q|k|v of truncated forwards (debug tap 5): chained through the tap they must give the context's bits
    for k in range(1, L + 1):
        ctx.debug_set_layers(k)
        ctx.forward(images)
        qkvs.append(ctx.debug_read(5, 3 * T * 3 * D).reshape(3 * T, 3 * D))
    ctx.debug_set_layers(-1)
    ctx.set_rollout(1, -1, fusion)
    assert ctx.rollout() == (1, L, fusion) and np.array_equal(ctx.forward(images), logits)   # the logits keep their bits
    assert ctx.rollout_dims() == (3, T, T - lead, 1, L)
    full, tap = ctx.read_rollout(rows=T), None
    for q in qkvs:
        tap = run_step(q, 3, T, H, hd, dt, fusion, tap)
    assert AM.same_bits(full, tap)
    worst = ratio(full, RO.chain64(RO.model_qkv64(MICRO, blob, images, flags, EPS), 3, T, H, hd, fusion))
    print(f"flags {flags:#x} {NAME[dt]} fusion {fusion}: worst max|d| / max|ref| against the float64 model = {worst:.3e} (bound {MODEL_BOUND[dt]:.3e})")
    assert worst <= MODEL_BOUND[dt]
    # the read-out forms: the patch slice of row 0, the 16-bit roundings, the device calls
    patch2 = np.ascontiguousarray(full[:, :2, lead:])
    assert AM.same_bits(ctx.read_rollout(1, keys=PATCH), np.ascontiguousarray(patch2[:, :1]))
    for elem in (F16, B16):
        assert AM.same_bits(ctx.read_rollout(2, elem=elem), vithip.to16(full[:, :2], AM.ELEM_DTYPE[elem]).reshape(3, 2, T))
    out = Guarded(patch2.nbytes)
    for call in (ctx.read_rollout_device, ctx.read_rollout_device_async):
        call(vithip.Rollout(out.ptr, F32, 2, PATCH, 0))
        ctx.synchronize()
        assert AM.same_bits(out.read(np.float32, patch2.shape), patch2)
    out.free()
    # batch 1 against the same image inside batch 3; three streams (parts of one image each); eager against graph replay; a sub-range
    ctx.forward(images[1:2])
    assert AM.same_bits(ctx.read_rollout(rows=T), full[1:2])
    ctx.set_streams(3)
    ctx.forward(images)
    assert AM.same_bits(ctx.read_rollout(rows=T), full)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for rep in range(3):   # eager, captured, replayed
        ctx.forward(images)
        assert AM.same_bits(ctx.read_rollout(rows=T), full), rep
    ctx.set_graph(False)
    ctx.set_rollout(2, 2, fusion)
    ctx.forward(images)
    assert ctx.rollout_dims()[3:] == (2, 2) and AM.same_bits(ctx.read_rollout(rows=T), run_step(qkvs[1], 3, T, H, hd, dt, fusion))
    ctx.set_rollout(0)
    assert ctx.rollout()[0] == 0 and np.array_equal(ctx.forward(images), logits)
    ctx.close()


def test_rollout_does_not_depend_on_the_qkv_layout(monkeypatch):
    """ViT-B/16 bf16 at batch 224 keeps q|k|v head-major; a context created under VH_QKV_HM=0 keeps it row-major (debug tap 4 says
    which).  The same rollout, bit for bit, on one stream and on three (odd image offsets of the parts), and attention_rollout()."""
    cfg, batch = S.CONFIGS["vit_base"], 224
    din, dout = vithip.DeviceBuffer(batch * cfg["image_size"] ** 2 * cfg["channels"] * 4), vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    got, used = [], []
    for hm in ("1", "0"):
        monkeypatch.setenv("VH_QKV_HM", hm)
        ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=batch)
        ctx.init_weights_seeded(0)
        ctx.fill_input_seeded(1, batch, din.ptr)
        ctx.forward_device(din.ptr, batch, dout.ptr)
        with pytest.raises(vithip.VhError) as e:   # the first call sets layers 1 .. 12 itself and says so
            ctx.attention_rollout("max")
        assert e.value.code == VH_ERR_STATE and ctx.rollout() == (1, cfg["layers"], RO.MAX)
        ctx.forward_device(din.ptr, batch, dout.ptr)
        used.append(int(ctx.debug_read(4, 1)[0]))
        got.append(ctx.read_rollout(rows=2))
        assert AM.same_bits(ctx.attention_rollout("max").reshape(batch, 1, 196), np.ascontiguousarray(got[-1][:, :1, 1:]))
        ctx.set_streams(3)
        ctx.forward_device(din.ptr, batch, dout.ptr)
        got.append(ctx.read_rollout(rows=2))
        ctx.close()
    din.free(); dout.free()
    assert used == [1, 0] and np.isfinite(got[0]).all() and all(AM.same_bits(g, got[0]) for g in got[1:])
    assert np.abs(got[0].astype(np.float64).sum(-1) - 1).max() < 12 * (197 + 8) * 2.0 ** -23   # rows of R sum to 1


def test_refusals_on_a_live_context():
    ctx, _ = make_ctx(0, BF16)
    lib, L, T = vithip.lib(), MICRO["layers"], RR.tokens(MICRO, 0)
    host, images = np.full((2, T, T), np.float32(-7.0)), S.make_images(MICRO, 1, 2)
    dbuf = Guarded(host.nbytes)

    def read(code, text, elem=F32, rows=1, keys=ALL, reserved=0, device=None, out=True):
        desc = vithip.Rollout((device or host.ctypes.data) if out else None, elem, rows, keys, reserved)
        for call in ((lib.vh_read_rollout_device, lib.vh_read_rollout_device_async) if device else (lib.vh_read_rollout,)):
            assert call(ctx.h, C.byref(desc)) == code, text
            assert text in lib.vh_last_error(ctx.h).decode(), lib.vh_last_error(ctx.h).decode()
        assert (host == -7.0).all() and dbuf.untouched()

    for args, text in (((-1, -1, 0), "first_layer"), ((L + 1, -1, 0), "first_layer"), ((2, 1, 0), "last_layer"), ((1, L + 1, 0), "last_layer"), ((1, -1, 2), "fusion")):
        with pytest.raises(vithip.VhError) as e:
            ctx.set_rollout(*args)
        assert e.value.code == VH_ERR_INVALID and text in str(e.value)
    ctx.forward(images)
    read(VH_ERR_STATE, "no rollout was set")
    ctx.set_rollout(2, -1, RO.MEAN)
    read(VH_ERR_STATE, "no rollout was set")   # a new range clears what the last forward chained
    ctx.debug_set_layers(1)
    ctx.forward(images)
    read(VH_ERR_STATE, "did not reach layer 2")
    ctx.debug_set_layers(-1)
    ctx.forward(images)
    assert lib.vh_read_rollout(ctx.h, None) == VH_ERR_INVALID and "null descriptor" in lib.vh_last_error(ctx.h).decode()
    for text, kw in (("out is NULL", dict(out=False)), ("elem", dict(elem=vithip.ELEM_U8)), ("rows 0", dict(rows=0)), (f"rows {T + 1}", dict(rows=T + 1)),
                     ("keys", dict(keys=2)), ("reserved", dict(reserved=1)), ("16-byte aligned", dict(device=dbuf.ptr + 8))):
        read(VH_ERR_INVALID, text, **kw)
    assert np.isfinite(ctx.read_rollout(rows=T)).all()
    ctx.ring_create(2, 1)
    read(VH_ERR_STATE, "a ring exists")
    with pytest.raises(vithip.VhError) as e:
        ctx.set_rollout(1)
    assert e.value.code == VH_ERR_STATE
    ctx.close()
    ctx = vithip.VitContext(MICRO, dtype=BF16, max_batch=2, ln_eps=EPS)   # no weights yet: nothing has run
    ctx.set_rollout(1)
    read(VH_ERR_STATE, "no forward has run")
    ctx.close()
    for flag, text in ((vithip.FLAG_CLS_TAIL, "VH_FLAG_CLS_TAIL"), (vithip.FLAG_ATTN_BIAS, "VH_FLAG_ATTN_BIAS")):   # by kind of context
        ctx = vithip.VitContext(MICRO, dtype=BF16, max_batch=2, flags=flag, ln_eps=EPS)
        with pytest.raises(vithip.VhError) as e:
            ctx.set_rollout(1)
        assert e.value.code == VH_ERR_UNSUPPORTED and text in str(e.value)
        read(VH_ERR_UNSUPPORTED, text)
        read(VH_ERR_UNSUPPORTED, text, device=dbuf.ptr)
        ctx.close()
    dbuf.free()
