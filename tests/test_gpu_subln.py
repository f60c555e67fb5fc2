"""GPU suite of VH_FLAG_SUB_LN: the gate pass with the inner LayerNorm through vh_op_swiglu_ln (both layouts, fp16 and bf16, canaries, a
per-element bound against float64 from the same 16-bit inputs, widths that end inside a 16-byte chunk, exact cases), the three EVA-02
fixtures (one of them with such a width) through a context, the seeded weights, and bit invariance across batch, streams and graph replay.
Kernel bound: |got - ref| <= 1/2 ulp16(ref) + K 2^-24 (|ref - b_j| + |w_j|).  K = 6.16 = 4 x 1.54, the worst fp32 term measured on an
MI355X over the first 64 cases (fp16, rows 272, M 4096, n 4096: profiles/subln_gpu_tests.txt); cases added since are held to the same K (their worst: 2.19)."""
import numpy as np
import pytest
import vithip

import subln_ref as U
import vh_synth as S
from vh_testlib import dev, rel, same_bits

pytestmark = pytest.mark.gpu

BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
NAME, MANT, MIN_NORMAL = {BF16: "bf16", FP16: "fp16"}, {BF16: 7, FP16: 10}, {BF16: 2.0 ** -126, FP16: 2.0 ** -14}
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}
CANARY, EPS, K = 64, 1e-6, 6.16
# (M, n): n = M; n a multiple of 8 inside M; n that ends inside a chunk (61 = 7 * 8 + 5; 2730 = 341 * 8 + 2, EVA-02-L's width)
WIDTHS = ((64, 64), (64, 61), (192, 192), (768, 688), (2816, 2730), (4096, 4096))
SHAPES = [(rows, M, n) for M, n in WIDTHS for rows in (1, 17, 16, 48, 272)]


def run(gu_bits, dt, rows, M, n, w, b, tiled, eps=EPS):
    """h's bits [rows][M] in row-major order, whichever layout was asked for; the output sits between canaries, the input is not written."""
    pad = np.full(CANARY, 0x7B5A, np.uint16)
    out, d = dev(np.concatenate([pad, np.full(rows * M, 0x7B5A, np.uint16), pad])), dev(np.ascontiguousarray(gu_bits))
    vithip.op_swiglu_ln(d.ptr, dt, rows, M, n, dev(w.astype(np.float32)).ptr, dev(b.astype(np.float32)).ptr, eps, out.ptr + pad.nbytes, tiled)
    got = out.to_numpy(np.uint16, (rows * M + 2 * CANARY,))
    assert np.array_equal(got[:CANARY], pad) and np.array_equal(got[-CANARY:], pad), "a canary element was written"
    assert np.array_equal(d.to_numpy(np.uint16, gu_bits.shape), gu_bits), "the input was written"
    return vithip.unpack_tiled(got[CANARY:-CANARY], rows, M) if tiled else got[CANARY:-CANARY].reshape(rows, M)


@pytest.mark.parametrize("rows,M,n", SHAPES, ids=[f"r{r}_m{m}_n{n}" for r, m, n in SHAPES])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_kernel_against_float64(dt, rows, M, n):
    """Seeded g, u, w, b with a placement pattern: w_j and b_j differ from column to column and rows differ, so a chunk that landed
    elsewhere misses the bound.  g, u, w and b are non-zero in the columns >= n too: those columns must be masked, not multiplied by
    zero, and come out as +0 bit for bit.  The tiled output is the tiling of the row-major one."""
    rng = np.random.default_rng([rows, M, n, dt])
    gu = np.concatenate([rng.uniform(-6, 6, (rows, M)), rng.uniform(-4, 4, (rows, M))], 1).astype(np.float32)
    gu[:, n:M], gu[:, M + n:] = 5.0, 3.0
    bits = vithip.to16(gu, dt)
    w = (1.0 + 0.5 * np.sin(np.arange(M) * 0.37)).astype(np.float32).astype(np.float64)
    b = (0.25 * np.cos(np.arange(M) * 0.11) + 0.3).astype(np.float32).astype(np.float64)
    ref = U.gate_ln(M, n, w, b, EPS)(vithip.from16(bits, dt).astype(np.float64))     # (reads columns < n only; zero from n on)
    keep = ~((ref != 0) & (np.abs(ref) < MIN_NORMAL[dt]))                      # the CPU pre-check: subnormal results are not judged
    assert (~keep).mean() <= 0.01
    half_ulp = 0.5 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), MIN_NORMAL[dt]))) - MANT[dt])
    unit = 2.0 ** -24 * (np.abs(ref - b) + np.abs(w))
    outs = []
    for tiled in ([False, True] if rows % 16 == 0 else [False]):
        got_bits = run(bits, dt, rows, M, n, w, b, tiled)
        got = vithip.from16(got_bits, dt).astype(np.float64)
        worst = float((np.maximum(np.abs(got - ref) - half_ulp, 0) / unit)[:, :n][keep[:, :n]].max())
        print(f"\n[subln] kernel {NAME[dt]} rows {rows} M {M} n {n} {'tiled' if tiled else 'row-major'}: fp32 term {worst:.2f} x 2^-24 (K = {K:g})")
        assert np.isfinite(got).all() and worst <= K
        assert not got_bits[:, n:].any(), "a column >= n is not +0"
        outs.append(got_bits)
    assert len(outs) == 1 or np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_a_row_of_equal_products_is_exactly_zero(dt):
    rows, M = 16, 192   # g = 32: the sigmoid is 1 in fp32, so every product is 48 and every partial sum an integer
    gu = np.concatenate([np.full((rows, M), 32.0), np.full((rows, M), 1.5)], 1).astype(np.float32)
    for tiled in (False, True):
        assert not run(vithip.to16(gu, dt), dt, rows, M, M, np.ones(M), np.zeros(M), tiled).any()


def test_tap_refusals():
    d, h, w = dev(np.zeros(16 * 128, np.uint16)), dev(np.zeros(16 * 64, np.uint16)), dev(np.zeros(64, np.float32))
    ok = dict(dtype=BF16, rows=16, mlp_dim=64, width=64, weight_ptr=w.ptr, bias_ptr=w.ptr, eps=EPS, h_ptr=h.ptr)
    for change, text in ((dict(dtype=vithip.DTYPE_FP8), "dtype is not"), (dict(rows=0), "rows outside"), (dict(mlp_dim=96), "multiple of 64"),
                         (dict(mlp_dim=4160), "mlp_dim above 4096"), (dict(width=0), "width outside"), (dict(width=65), "width outside"),
                         (dict(eps=0.0), "eps must be positive"), (dict(weight_ptr=None), "null weight or bias"), (dict(h_ptr=None), "null gu16 or h16"),
                         (dict(bias_ptr=w.ptr + 4), "weight and bias must be 16-byte aligned"), (dict(h_ptr=h.ptr + 2), "gu16 and h16 must be 16-byte"),
                         (dict(rows=24, out_tiled=True), "rows to be a multiple of 16")):
        with pytest.raises(vithip.VhError, match=text):
            vithip.op_swiglu_ln(d.ptr, **dict(ok, **change))


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_logits(name, dt):
    """c: the converter's padding and the context's forward where the width ends inside a chunk (346 = 43 * 8 + 2)."""
    z, cfg, flags, blob, _ = U.fixture(name)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(z["images"]), flags=flags, ln_eps=EPS)
    ctx.load_weights(blob)
    got, fold = ctx.forward(z["images"]), ctx.ln_fold()
    e = rel(got, z["logits"])
    print(f"\n[subln] fixture {name} {NAME[dt]} (fold {fold}): logits {e:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and e <= MODEL_TOL[dt] and np.array_equal(got.argmax(1), z["logits"].argmax(1))
    assert fold == (name == "b")
    ctx.close()
    # a context's own refusal: the blob without its three last tensors, bit 29 still set, into a context without the flag
    plain = vithip.VitContext(cfg, dtype=dt, max_batch=1, flags=flags & ~vithip.FLAG_SUB_LN, ln_eps=EPS)
    with pytest.raises(vithip.VhError, match=r"header bit 29 \(LayerNorm inside the SwiGLU MLP\) is 1, the context's VH_FLAG_SUB_LN is 0"):
        plain.load_weights(blob[:U.width_at(cfg, blob)].copy())
    plain.close()


def test_seeded_weights_and_a_forged_width_word_at_load():
    """vh_init_weights_seeded: n = M, weight 0.05 around 1, bias sigma 0.02.  A blob whose width word is forged is refused at load by
    name, and the refused load changes nothing."""
    cfg, flags = dict(U.SMALL, mlp_dim=192), vithip.FLAG_ROPE | vithip.FLAG_SWIGLU | vithip.FLAG_SUB_LN
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=3, flags=flags, ln_eps=EPS)
    ctx.init_weights_seeded(7)
    blob = ctx.export_weights()
    t, at = U.unpack_blob(cfg, blob, flags), U.width_at(cfg, blob)
    assert t["subln.width"][0] == 192 and abs(t["subln.weight"].mean() - 1) < 0.01 and 0.03 < t["subln.weight"].std() < 0.07
    assert abs(t["subln.bias"].mean()) < 0.005 and 0.01 < t["subln.bias"].std() < 0.03
    images = S.make_images(cfg, 8, 3)
    got = ctx.forward(images)
    for word in (0.0, 193.0, 2.5):
        blob[at:at + 4] = np.array([word], np.float32).view(np.uint8)
        with pytest.raises(vithip.VhError, match=r"subln.width is [0-9.]+, not an integer in 1 .. mlp_dim = 192"):
            ctx.load_weights(blob)
    assert np.isfinite(got).all() and same_bits(ctx.forward(images), got)
    ctx.close()


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_same_logit_bits_alone_in_a_batch_across_streams_and_graph_replay(dt):
    z, cfg, flags, blob, _ = U.fixture("b")
    images = np.concatenate([z["images"], z["images"][:2][:, ::-1]])
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=5, flags=flags, ln_eps=EPS)
    ctx.load_weights(blob)
    five = ctx.forward(images)
    assert same_bits(five[:3], ctx.forward(images[:3])) and same_bits(ctx.forward(images[2:3]), five[2:3])
    ctx.set_streams(3)
    assert same_bits(ctx.forward(images), five)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert same_bits(ctx.forward(images), five)
    ctx.close()
