"""GPU suite of the SwiGLU model switch, VH_FLAG_SWIGLU: the gate pass through vh_op_swiglu (both output layouts, fp16 and bf16, a
per-element bound against float64, exact cases, a placement pattern, canaries around the output); whole forwards of the three Hugging
Face fixtures (identity head: the logits ARE pooler_output); forged blobs; a shape that keeps h in its tiled layout, against a child
process under VH_H_TILED=0; bit invariance across batch, streams and graph replay; token and layer features against the debug taps.
Tolerances: the project's model bounds (fp16 1e-3, bf16 1e-2 as the labelled regression bound); for the kernel
|got - ref| <= 1/2 ulp16(ref) + 2^-20 |ref| (at most eight fp32 roundings, plus exp2 and rcp at 1 ulp each)."""
import glob
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import swiglu_ref as W
import vh_synth as S
import vit_ref as R
from vh_testlib import _KEEP, _release_buffers, dev, rel, same_bits

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16"}
MANT = {BF16: 7, FP16: 10}                  # stored mantissa bits
MIN_NORMAL = {BF16: 2.0 ** -126, FP16: 2.0 ** -14}
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
SWIGLU, ROPE, REG = vithip.FLAG_SWIGLU, vithip.FLAG_ROPE, vithip.FLAG_REGISTERS
HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 64   # elements in front of and behind the output (a multiple of 8: the output stays 16-byte aligned)
SHAPES = [(rows, M) for M in (64, 192, 768) for rows in (16, 48, 272)]


def fixture(name):
    path, = glob.glob(os.path.join(HERE, "golden", "swiglu", name + "_s*.npz"))
    return np.load(path), W.fixture_cfg(name), W.fixture_flags(name), W.fixture_blob(name), W.fixture_eps(name)


# ---- 1. the kernel through vh_op_swiglu --------------------------------------------------------------------------------------------
def run(gu_bits, dt, rows, M, tiled):
    """gu [rows][2 M] as 16-bit bits through vh_op_swiglu, the output between CANARY elements of a pattern; returns h's bits [rows][M]
    in row-major order whichever layout was asked for (the tiled one through vithip.unpack_tiled, the GEMM tests' tap)."""
    pad = np.full(CANARY, 0x7B5A, np.uint16)
    out = dev(np.concatenate([pad, np.full(rows * M, 0x7B5A, np.uint16), pad]))
    src = np.ascontiguousarray(gu_bits).reshape(rows, 2 * M)
    d = dev(src)
    vithip.op_swiglu(d.ptr, dt, rows, M, out.ptr + pad.nbytes, tiled)
    got = out.to_numpy(np.uint16, (rows * M + 2 * CANARY,))
    assert np.array_equal(got[:CANARY], pad) and np.array_equal(got[-CANARY:], pad), "a canary element was written"
    assert np.array_equal(d.to_numpy(np.uint16, src.shape), src), "the input was written"
    body = got[CANARY:-CANARY]
    return vithip.unpack_tiled(body, rows, M) if tiled else body.reshape(rows, M)


def ref64(gu_bits, dt, M):
    v = vithip.from16(gu_bits, dt).astype(np.float64)
    return W.silu(v[:, :M]) * v[:, M:]


def bound(ref, dt):
    """1/2 ulp of the storage type at ref + 2^-20 |ref|; ulp16(ref) = 2^(floor(log2 |ref|) - mantissa bits), the smallest normal's below it."""
    a = np.maximum(np.abs(ref), MIN_NORMAL[dt])
    return 0.5 * 2.0 ** (np.floor(np.log2(a)) - MANT[dt]) + 2.0 ** -20 * np.abs(ref)


def seeded(dt, rows, M):
    # (the last seed word: the first for which every case of SHAPES passes the test's pre-check, "at most 1 % of the fp16 results are
    # subnormal"; the expected share on these ranges is 0.95 %, so a small case misses it on about every second seed)
    rng = np.random.default_rng([rows, M, dt, 6])
    gu = np.concatenate([rng.uniform(-12, 12, (rows, M)), rng.uniform(-4, 4, (rows, M))], 1).astype(np.float32)
    return vithip.to16(gu, dt)


def layouts(rows):
    return [False, True] if rows % 16 == 0 else [False]


@pytest.mark.parametrize("rows,M", SHAPES, ids=[f"r{r}_m{m}" for r, m in SHAPES])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_gate_kernel_against_float64(dt, rows, M):
    bits = seeded(dt, rows, M)
    ref = ref64(bits, dt, M)
    keep = ~((ref != 0) & (np.abs(ref) < MIN_NORMAL[dt]))      # the CPU pre-check: results in the subnormal range are not judged
    assert (~keep).mean() <= 0.01, float((~keep).mean())
    tol = bound(ref, dt)
    outs = []
    for tiled in layouts(rows):
        got_bits = run(bits, dt, rows, M, tiled)
        got = vithip.from16(got_bits, dt).astype(np.float64)
        err = np.abs(got - ref)
        worst = float((err / tol)[keep].max())
        print(f"\n[swiglu] kernel {NAME[dt]} rows {rows} M {M} {'tiled' if tiled else 'row-major'}: worst |d| / bound = {worst:.3f}, dropped {int((~keep).sum())}")
        assert np.isfinite(got).all() and not (err > tol)[keep].any(), (tiled, int((err > tol)[keep].sum()), worst)
        outs.append(got_bits)
    if len(outs) == 2:   # the tiled output is the tiling of the row-major output, bit for bit
        assert np.array_equal(vithip.pack_tiled(outs[0]), vithip.pack_tiled(outs[1])) and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_gate_kernel_exact_cases(dt):
    rows, M = 48, 192
    rng = np.random.default_rng([3, dt])
    # g = 0 gives h = 0 for every u, the largest finite ones included
    u = vithip.from16(vithip.to16(rng.uniform(-4, 4, (rows, M)).astype(np.float32), dt), dt)
    u[0, :4] = [65504.0, -65504.0, 1.0, -1.0]
    gu = np.concatenate([np.zeros((rows, M), np.float32), u], 1)
    gu[1, :M] = -0.0
    for tiled in (False, True):
        assert not vithip.from16(run(vithip.to16(gu, dt), dt, rows, M, tiled), dt).any()
    # g >= 32: the sigmoid is 1 in fp32 (1 + exp2(-46) rounds to 1, and rcp(1.0f) == 1.0f), so h = RNE16(g u), exact in fp32 for integer
    # u with |g u| <= 256
    g = vithip.from16(vithip.to16(rng.uniform(32, 64, (rows, M)).astype(np.float32), dt), dt)
    g[0, :3] = [32.0, 64.0, 32.25]
    k = np.floor(256.0 / g)
    u = np.rint(rng.uniform(-1, 1, (rows, M)) * k).astype(np.float32)
    u[0, :3] = [8.0, -4.0, 7.0]
    assert (np.abs(g * u) <= 256).all() and np.abs(u).max() >= 4
    want = vithip.to16(g * u, dt)      # the product of two 16-bit values is exact in fp32
    for tiled in (False, True):
        got = run(vithip.to16(np.concatenate([g, u], 1), dt), dt, rows, M, tiled)
        same = (got == want) | ((vithip.from16(got, dt) == 0) & (vithip.from16(want, dt) == 0))
        assert same.all(), (tiled, int((~same).sum()), vithip.from16(got[~same][:4], dt), vithip.from16(want[~same][:4], dt))


def pattern(rows, M, mul_r, mul_c, mod, dt):
    """u [rows][M] of values (1 + k / 8) 2^e, k = id % 8, e = id // 8 - 14, id = (row mul_r + col mul_c) % mod, mod <= 192 (32 u stays a
    normal fp16 value): two different ids are at least 8 ulp of either storage type apart (8 bf16 ulp of the larger between 1.875 2^e
    and 2^(e + 1)), and neighbours in a row or a column have different ids."""
    assert mod <= 192
    ident = (np.arange(rows)[:, None] * mul_r + np.arange(M)[None, :] * mul_c) % mod
    return ((1.0 + (ident % 8) / 8.0) * 2.0 ** (ident // 8 - 14)).astype(np.float32), ident


@pytest.mark.parametrize("rows,M", [(48, 192), (272, 768)], ids=["r48_m192", "r272_m768"])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_gate_kernel_places_every_chunk(dt, rows, M):
    """g = 32 (h = 32 u to well inside the bound) and two patterns of u: a 16-byte chunk that landed anywhere else fails the tolerance
    under at least one of them -- checked on the CPU first: no two chunks of the output carry the same pair of id sequences."""
    pats = [pattern(rows, M, 37, 101, 191, dt), pattern(rows, M, 101, 37, 181, dt)]
    for u, ident in pats:
        assert (ident[:, 1:] != ident[:, :-1]).all() and (ident[1:] != ident[:-1]).all()
    sig = np.concatenate([ident.reshape(rows, M // 8, 8) for _, ident in pats], -1).reshape(rows * (M // 8), 16)
    assert len(np.unique(sig, axis=0)) == len(sig)
    for u, _ in pats:
        bits = vithip.to16(np.concatenate([np.full((rows, M), 32.0, np.float32), u], 1), dt)
        assert np.array_equal(vithip.from16(bits, dt)[:, M:], u)                     # the pattern is exact in the storage type
        ref = ref64(bits, dt, M)
        tol = bound(ref, dt)
        assert (np.abs(np.diff(ref, axis=1)) > 8 * tol[:, 1:]).all() and (np.abs(np.diff(ref, axis=0)) > 8 * tol[1:]).all()   # > 4 ulp apart
        for tiled in layouts(rows):
            got = vithip.from16(run(bits, dt, rows, M, tiled), dt).astype(np.float64)
            bad = np.abs(got - ref) > tol
            assert not bad.any(), (tiled, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_gate_tap_refusals():
    d, h = dev(np.zeros(16 * 128 + 64, np.uint16)), dev(np.zeros(16 * 64 + 64, np.uint16))
    for args, text in (((FP8, 16, 64, h.ptr, False), "dtype is not"), ((BF16, 0, 64, h.ptr, False), "rows outside"),
                       ((BF16, -16, 64, h.ptr, False), "rows outside"), ((BF16, 16, 0, h.ptr, False), "mlp_dim must be a multiple of 64"),
                       ((BF16, 16, 96, h.ptr, False), "mlp_dim must be a multiple of 64"), ((BF16, 16, (1 << 16) + 64, h.ptr, False), "at most 2\\^16"),
                       ((BF16, 24, 64, h.ptr, True), "rows to be a multiple of 16"), ((BF16, 16, 64, None, False), "null pointer"),
                       ((BF16, 16, 64, h.ptr + 2, False), "16-byte aligned")):
        with pytest.raises(vithip.VhError, match=text):
            vithip.op_swiglu(d.ptr, *args)
    with pytest.raises(vithip.VhError, match="null pointer"):
        vithip.op_swiglu(None, BF16, 16, 64, h.ptr)
    with pytest.raises(vithip.VhError, match="16-byte aligned"):
        vithip.op_swiglu(d.ptr + 8, BF16, 16, 64, h.ptr)
    rc = vithip.lib().vh_op_swiglu(d.ptr, BF16, 16, 64, h.ptr, 2, None)
    assert rc == 1 and b"out_tiled must be 0 or 1" in vithip.lib().vh_last_error(None)


# ---- 2. whole forwards of the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_outputs(name, dt):
    """Identity head: the logits are pooler_output; so are debug tap 1 and vh_read_features' normalised class token; top-1 agrees.
    Measured on an MI355X (max |d| / max |ref|): fp16 a 2.6e-4, b 4.5e-4, c 7.5e-4; bf16 a 2.3e-3, b 4.1e-3, c 5.3e-3."""
    z, cfg, flags, blob, eps = fixture(name)
    images = z["images"]
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags, ln_eps=eps)
    ctx.load_weights(blob)
    got, fold = ctx.forward(images), ctx.ln_fold()
    tap = ctx.debug_read(1, got.size).reshape(got.shape)
    feat = ctx.read_features(cls=True, patch=False)["cls"]
    guard = ctx.ln_guard()
    ctx.close()
    e = rel(got, z["pooler_output"])
    print(f"\n[swiglu] fixture {name} {NAME[dt]} (fold {fold}, guard {guard}): pooler_output {e:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and e <= MODEL_TOL[dt], e
    assert np.array_equal(tap, got) and np.array_equal(feat, got)                       # the identity head passes its input through
    assert np.array_equal(got.argmax(1), z["pooler_output"].argmax(1))
    assert fold == (cfg["dim"] % 256 == 0)


@pytest.mark.parametrize("name", ["a", "c"])
def test_a_blob_whose_bit_differs_is_refused_by_name(name):
    z, cfg, flags, blob, eps = fixture(name)
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags, ln_eps=eps)
    ctx.load_weights(blob)
    want = ctx.forward(z["images"][:2])
    with pytest.raises(vithip.VhError, match=r"header bit 25 \(SwiGLU MLP\) is 0, the context's VH_FLAG_SWIGLU is 1") as e:
        ctx.load_weights(W.with_bit(blob, False))
    assert e.value.code == 1
    assert same_bits(ctx.forward(z["images"][:2]), want)                                # the refused load changed nothing
    ctx.close()
    plain = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags & ~SWIGLU, ln_eps=eps)
    with pytest.raises(vithip.VhError, match="bytes, expected"):                        # the flagged blob is longer: its size speaks
        plain.load_weights(blob)
    blob0 = R.make_blob(cfg, 5, flags & ~SWIGLU, eps)
    with pytest.raises(vithip.VhError, match=r"header bit 25 \(SwiGLU MLP\) is 1, the context's VH_FLAG_SWIGLU is 0"):
        plain.load_weights(W.with_bit(blob0, True))
    plain.load_weights(blob0)
    plain.close()


# ---- 3. the tiled hidden activation ------------------------------------------------------------------------------------------------
# The smallest shape around D = 256, M = 768 at which gemm_tiled_applies accepts (rows, 2 M, D), (rows, M, D) and (rows, D, M): whole
# 256-row tiles and at least 128 tiles of 256 x 256 in every one of them, i.e. rows / 256 * D / 256 >= 128: 32 768 rows = 1024 images of
# 32 tokens (16 patches, the class token, 15 registers).
TILED = dict(image_size=32, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=768, layers=2, classes=40)
TILED_FLAGS, TILED_BATCH = SWIGLU | REG(15), 1024

CHILD = """
import hashlib, sys
import numpy as np
import vithip
cfg, flags, batch = {cfg!r}, {flags}, {batch}
px = cfg["image_size"] ** 2 * cfg["channels"]
din, dout = vithip.DeviceBuffer(batch * px * 4), vithip.DeviceBuffer(batch * cfg["classes"] * 4)
ctx = vithip.VitContext(cfg, dtype={dt}, max_batch=batch, flags=flags)
ctx.init_weights_seeded(0)
ctx.fill_input_seeded(1, batch, din.ptr)
ctx.forward_device(din.ptr, batch, dout.ptr)
print("tiled", int(ctx.debug_read(3, 1)[0]), "sha", hashlib.sha256(dout.to_numpy(np.float32, (batch, cfg["classes"])).tobytes()).hexdigest())
ctx.close()
"""


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_tiled_hidden_activation_and_the_row_major_one_give_the_same_bits(dt):
    cfg, flags, batch = TILED, TILED_FLAGS, TILED_BATCH
    px = cfg["image_size"] ** 2 * cfg["channels"]
    din, dout = vithip.DeviceBuffer(batch * px * 4), vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=batch, flags=flags)
    ctx.init_weights_seeded(0)
    blob = ctx.export_weights()
    ctx.fill_input_seeded(1, batch, din.ptr)
    ctx.forward_device(din.ptr, batch, dout.ptr)
    tiled = int(ctx.debug_read(3, 1)[0])
    logits = dout.to_numpy(np.float32, (batch, cfg["classes"]))
    ctx.close()
    din.free(); dout.free()
    assert tiled == 1 and np.isfinite(logits).all()
    assert np.array_equal(blob, W.make_blob(cfg, 0, flags))                             # the seeded model: the longer fc1 from the same tensor ids
    pick = [0, 500, 1023]
    images = np.stack([S.fill(px, 1, 0x100, 0, start=i * px) for i in pick]).reshape(len(pick), cfg["image_size"], cfg["image_size"], cfg["channels"])
    e = rel(logits[pick], W.forward(cfg, blob, images, flags))
    print(f"\n[swiglu] tiled h, {NAME[dt]} b{batch}: {e:.3e} (bound {MODEL_TOL[dt]:g})")
    assert e <= MODEL_TOL[dt]
    # the same forward in a fresh process whose context was created under VH_H_TILED=0
    root = os.path.dirname(HERE)
    path = os.pathsep.join([HERE, os.path.join(root, "vit-fpga_amd", "python")])
    env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get("PYTHONPATH", ""), VH_H_TILED="0")
    r = subprocess.run([sys.executable, "-c", CHILD.format(cfg=cfg, flags=flags, batch=batch, dt=dt)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["tiled", "0", "sha", hashlib.sha256(logits.tobytes()).hexdigest()], r.stdout


# ---- 4. the same logit bits on every route into a forward; features ----------------------------------------------------------------
MID = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=40)       # folds; hd 64
SMALL = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=192, layers=2, classes=40)     # the fp32 residual path


def context(cfg, dt, flags, max_batch=5, seed=5):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=max_batch, flags=flags)
    ctx.load_weights(W.make_blob(cfg, seed, flags))
    return ctx


@pytest.mark.parametrize("cfg,dt,flags", [(MID, BF16, SWIGLU | REG(4)), (MID, FP16, SWIGLU | ROPE | REG(4)), (SMALL, FP16, SWIGLU)],
                         ids=["mid_bf16", "mid_rope_fp16", "small_fp16"])
def test_same_logit_bits_alone_in_a_batch_across_streams_and_graph_replay(cfg, dt, flags):
    images = S.make_images(cfg, 8, 5)
    ctx = context(cfg, dt, flags)
    five = ctx.forward(images)
    assert np.isfinite(five).all()
    assert rel(five, W.forward(cfg, W.make_blob(cfg, 5, flags), images, flags)) <= MODEL_TOL[dt]
    one = context(cfg, dt, flags, max_batch=1)
    assert same_bits(one.forward(images[2:3]), five[2:3])                             # image 2 alone at max_batch 1
    one.close()
    assert same_bits(ctx.forward(images[1:4]), five[1:4])
    ctx.set_streams(4)
    assert same_bits(ctx.forward(images), five)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert same_bits(ctx.forward(images), five)
    ctx.set_streams(4)
    for _ in range(3):
        assert same_bits(ctx.forward(images), five)
    ctx.set_graph(False)
    ctx.set_graph(True)   # new weights drop the captured graphs
    ctx.load_weights(W.make_blob(cfg, 6, flags))
    assert not same_bits(ctx.forward(images), five)
    ctx.load_weights(W.make_blob(cfg, 5, flags))
    assert same_bits(ctx.forward(images), five)
    ctx.close()


@pytest.mark.parametrize("cfg,dt", [(MID, BF16), (SMALL, FP16)], ids=["mid_bf16", "small_fp16"])
def test_token_and_layer_features_are_the_debug_taps(cfg, dt):
    flags, batch, D = SWIGLU | REG(4), 3, cfg["dim"]
    images = S.make_images(cfg, 8, batch)
    ctx = context(cfg, dt, flags)
    ctx.set_feature_layers([1])
    logits = ctx.forward(images)
    _, T, NP, _ = ctx.features_dims()
    assert T == NP + 5
    x = ctx.debug_read(0, batch * T * D).reshape(batch, T, D)
    rows = lambda f: np.concatenate([f["cls"][:, None], f["reg"], f["patch"]], 1)
    last = ctx.read_layer_features(-1, cls=True, patch=True, reg=True, norm=vithip.FEAT_RAW)
    first = ctx.read_layer_features(1, cls=True, patch=True, reg=True, norm=vithip.FEAT_RAW)
    assert same_bits(rows(last), x)
    assert same_bits(ctx.read_features(cls=False, patch=True, norm=vithip.FEAT_RAW)["patch"], x[:, 5:])
    assert same_bits(ctx.read_features(cls=True, patch=False)["cls"], ctx.debug_read(1, batch * D).reshape(batch, D))
    ref, hidden = W.forward(cfg, W.make_blob(cfg, 5, flags), images, flags, all_hidden=True)[::2]
    assert rel(logits, ref) <= MODEL_TOL[dt] and rel(rows(first).reshape(-1, D), hidden[1]) <= MODEL_TOL[dt]
    ctx.set_feature_layers([])
    ctx.debug_set_layers(1)
    ctx.forward(images)
    assert same_bits(ctx.debug_read(0, batch * T * D).reshape(batch, T, D), rows(first))
    ctx.close()
