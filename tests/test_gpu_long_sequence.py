"""GPU parity beyond 640 tokens: the K/V-streaming attention kernel (kernels_attn_hd.hip at head dim 64) through vh_op_attention, through
its own tap vh_op_attention_stream at every token count, and inside whole forwards of long-sequence models, against the CPU
oracle.  Tolerances are the existing ones: ATT_TOL of test_gpu_ops for the operator, the model-level bounds of test_gpu_vit
(fp16 1e-3, bf16 1e-2) and test_gpu_fp8 (fp8) for forwards.  The long-sequence configurations are defined here (not in
vh_synth.CONFIGS, whose every entry other tests run)."""
import numpy as np
import pytest

import oracle_lib as O
import vh_synth as S
from vh_testlib import _KEEP, _release_buffers, dev, rel

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
DT = [BF16, FP16]
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
ATT_TOL = {BF16: 1.2e-2, FP16: 1.5e-3}   # test_gpu_ops.ATT_TOL: P and O are rounded to 16 bit
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}     # test_gpu_vit.TOL (bf16: a regression bound, not the north star's tolerance)
Q_SCALE = np.float32(0.125 * 1.4426950408889634)   # VH_ATTN_Q_SCALE


def _cfg(image, patch, dim, heads, mlp, layers, classes=40):
    return dict(image_size=image, patch_size=patch, channels=3, dim=dim, heads=heads, mlp_dim=mlp, layers=layers, classes=classes)


TINY_512_16 = _cfg(512, 16, 256, 4, 512, 2)    # 1025 tokens
TINY_256_8 = _cfg(256, 8, 128, 2, 256, 3)      # 1025 tokens (patch 8)
TINY_448_16 = _cfg(448, 16, 256, 4, 512, 2)    # 785 tokens
VIT_B16_512 = _cfg(512, 16, 768, 12, 3072, 12, classes=1000)


def rnd16(a, dt):
    return O.round_bf16(a) if dt == BF16 else O.round_fp16(a)


def prescale_q(qkv, D, dt):
    """q columns x VH_ATTN_Q_SCALE rounded to 16 bit as the q|k|v GEMM delivers them; the oracle gets the same q back in its
    own convention (it scales by 64^-1/2 itself and works in base e) -- test_gpu_ops.prescale_q."""
    pre = qkv.copy()
    pre[:, :D] = rnd16(pre[:, :D] * Q_SCALE, dt)
    ref_in = pre.astype(np.float64)
    ref_in[:, :D] /= np.float64(Q_SCALE)
    return pre, ref_in.astype(np.float32)


def make_qkv(batch, tokens, heads, dt, seed):
    D = heads * 64
    qkv = rnd16((S.fill(batch * tokens * 3 * D, seed, tokens, 0) * 1.5).reshape(batch * tokens, 3 * D), dt)
    return prescale_q(qkv, D, dt)


def run_attention(op, pre, batch, tokens, heads, dt):
    D = heads * 64
    out = vithip.DeviceBuffer(batch * tokens * D * 2)
    _KEEP.append(out)
    op(dev(vithip.to16(pre, dt)).ptr, batch, tokens, heads, out.ptr, dt)
    return vithip.from16(out.to_numpy(np.uint16, (batch * tokens, D)), dt)


# ---- operator level ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_op_attention_beyond_640_tokens(dt):
    # tile edges (672 = 21 whole tiles, 673 one key into the next), the ViT-B/16 448 / 512 / 1024 token counts, 2049; and
    # (3, 1057, 2): 30 workgroups over 6 heads x 5 query slabs, whose K/V streams are read by every slab of the head
    for tokens, batch, heads in ((641, 1, 1), (672, 2, 1), (673, 1, 2), (785, 2, 1), (1025, 1, 2), (1057, 3, 2), (2049, 1, 1),
                                 (4097, 1, 1)):
        pre, qkv = make_qkv(batch, tokens, heads, dt, 21)
        ref = O.attention(qkv, batch, tokens, heads)
        got = run_attention(vithip.op_attention, pre, batch, tokens, heads, dt)
        err = np.abs(got - ref).reshape(batch, -1).max(1) / np.abs(ref).max()
        assert np.isfinite(got).all() and err.max() <= ATT_TOL[dt], (tokens, batch, heads, int(err.argmax()), float(err.max()))


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_stream_tap_at_short_token_counts(dt):
    # the streaming kernel where the resident forms run too: one tile, partial tiles, one wave to eight per workgroup, several
    # slabs; at 197 and 577 also against the resident forms (within the tolerance; bit equality is not part of the contract)
    for tokens, batch, heads in ((1, 2, 1), (17, 2, 2), (32, 1, 1), (33, 3, 1), (64, 1, 2), (65, 2, 1), (197, 2, 3), (577, 1, 2),
                                 (640, 1, 1)):
        pre, qkv = make_qkv(batch, tokens, heads, dt, 22)
        ref = O.attention(qkv, batch, tokens, heads)
        got = run_attention(vithip.op_attention_stream, pre, batch, tokens, heads, dt)
        assert np.isfinite(got).all()
        assert rel(got, ref) <= ATT_TOL[dt], (tokens, rel(got, ref))
        if tokens in (197, 577):
            res = run_attention(vithip.op_attention, pre, batch, tokens, heads, dt)
            assert np.abs(got - res).max() / np.abs(ref).max() <= ATT_TOL[dt], tokens


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_stream_spiked_scores_force_rescale_in_a_late_tile(dt):
    # test_gpu_ops.test_attention_spiked_scores_force_rescale at 1025 tokens: query 5 meets key 1000 (tile 31) with a score far
    # above its tile-0 shift, so the deferred rescale runs in a late key tile; query 40's larger score sits early (key 3)
    batch, heads, tokens, D = 1, 1, 1025, 64
    qkv = (S.fill(tokens * 3 * D, 11, 1, 0) * 0.5).reshape(tokens, 3 * D)
    qkv[5, :D] = 4.0
    qkv[1000, D:2 * D] = 4.0
    qkv[40, :D] = -3.0
    qkv[3, D:2 * D] = -3.0
    qkv = rnd16(qkv, dt)
    pre, qkv = prescale_q(qkv, D, dt)
    ref = O.attention(qkv, batch, tokens, heads)
    for op in (vithip.op_attention, vithip.op_attention_stream):
        got = run_attention(op, pre, batch, tokens, heads, dt)
        assert np.isfinite(got).all()
        assert rel(got, ref) <= ATT_TOL[dt]
        # query 5 attends essentially only to key 1000
        ulp = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
        assert np.abs(got[5] - qkv[1000, 2 * D:]).max() <= 2 * ulp * np.abs(qkv[1000, 2 * D:]).max() + 1e-6


@pytest.mark.parametrize("tokens,batch,heads", [(785, 2, 2), (97, 1, 2)])
def test_stream_e4m3_output(tokens, batch, heads):
    # bf16 in, e4m3 out (the VH_DTYPE_FP8 contexts' instantiation): op_attention above 640 tokens, the tap below
    D = heads * 64
    pre, qkv = make_qkv(batch, tokens, heads, BF16, 23)
    ref = O.attention(qkv, batch, tokens, heads)
    o8 = vithip.DeviceBuffer(batch * tokens * D)
    _KEEP.append(o8)
    op = vithip.op_attention if tokens > 640 else vithip.op_attention_stream
    op(dev(vithip.to16(pre, BF16)).ptr, batch, tokens, heads, o8.ptr, FP8)
    got = vithip.from_e4m3(o8.to_numpy(np.uint8, (batch * tokens, D)))
    want = O.quant_e4m3(ref)
    assert np.isfinite(got).all()
    # the oracle rounded to e4m3: equal except where bf16 P / O rounding moved a value across an e4m3 rounding boundary
    assert (got == want).mean() >= 0.75, float((got == want).mean())
    # bf16 P/O rounding inside the kernel (ATT_TOL) plus half an e4m3 step on the way out (test_gpu_fp8)
    assert np.all(np.abs(got - ref) <= 2.0 ** -4 * np.abs(ref) + ATT_TOL[BF16] * np.abs(ref).max())


# ---- model level -------------------------------------------------------------------------------------------------------

def _forward(cfg, blob, images, dt, flags=0):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags)
    ctx.load_weights(blob)
    got = ctx.forward(images)
    fold = ctx.ln_fold()
    ctx.close()
    return got, fold


FLAGS = [(0, "default"), (vithip.FLAG_LN_FOLD_OFF, "fold_off"), (vithip.FLAG_LN_FOLD_ON, "fold_on")]


@pytest.mark.parametrize("name,cfg", [("tiny_512_16", TINY_512_16), ("tiny_256_8", TINY_256_8), ("tiny_448_16", TINY_448_16)])
def test_long_sequence_forwards_match_the_oracle(name, cfg):
    blob, images = S.make_blob(cfg, 3), S.make_images(cfg, 4, 2)
    ref = O.vit_forward(cfg, blob, images)
    for dt in DT:
        for flags, label in FLAGS:
            got, _ = _forward(cfg, blob, images, dt, flags)
            e = rel(got, ref)
            print(f"\n[long] {name} T={S.tokens(cfg)} {NAME[dt]} {label}: logits {e:.3e}")
            assert np.isfinite(got).all() and e <= MODEL_TOL[dt], (NAME[dt], label, e)


@pytest.mark.parametrize("name,cfg", [("tiny_512_16", TINY_512_16), ("tiny_448_16", TINY_448_16)])
def test_long_sequence_fp8_forwards_track_the_emulation(name, cfg):
    # test_gpu_fp8.test_logits_track_the_fp8_emulation_and_the_fp32_forward's statistics (dims multiples of 128)
    blob, images = S.make_blob(cfg, 3), S.make_images(cfg, 4, 2)
    ref32 = O.vit_forward(cfg, blob, images)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    emu = {}
    for flags, label in FLAGS:
        got, folded = _forward(cfg, blob, images, FP8, flags)
        if folded not in emu:
            emu[folded] = O.vit_forward(cfg, blob, images, fp8="folded" if folded else True)
        r_emu32, r_gpu32, r_gpuemu = rms(emu[folded], ref32), rms(got, ref32), rms(got, emu[folded])
        print(f"\n[long fp8] {name} {label} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
        assert np.isfinite(got).all()
        assert r_gpu32 <= 1.5 * r_emu32 + 1e-3, label
        assert r_gpuemu <= 1.5 * r_emu32 + 1e-3, label
        assert rel(got, ref32) <= 0.25, label


@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_class_token_tail_runs_at_785_and_falls_back_at_1025(dt):
    # VH_FLAG_CLS_TAIL: at 785 tokens the one-query tail runs (logits to rounding); above 1024 the forward falls back to the
    # full last layer, i.e. exactly the default launch sequence (same bits)
    for cfg, runs in ((TINY_448_16, True), (TINY_512_16, False)):
        blob, images = S.make_blob(cfg, 5), S.make_images(cfg, 6, 2)
        base, _ = _forward(cfg, blob, images, dt, vithip.FLAG_LN_FOLD_ON)
        tail, _ = _forward(cfg, blob, images, dt, vithip.FLAG_LN_FOLD_ON | vithip.FLAG_CLS_TAIL)
        assert np.isfinite(tail).all()
        if runs:
            assert rel(tail, base) <= MODEL_TOL[dt], rel(tail, base)
        else:
            assert np.array_equal(tail, base)


def test_same_bits_across_batch_streams_and_graph_replay():
    cfg = TINY_256_8
    ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=3)
    ctx.load_weights(S.make_blob(cfg, 7))
    images = S.make_images(cfg, 8, 3)
    one = ctx.forward(images[:1])
    three = ctx.forward(images)
    assert np.isfinite(three).all()
    assert np.array_equal(three[:1], one)
    ctx.set_streams(2)
    assert np.array_equal(ctx.forward(images), three)
    ctx.set_streams(1)
    ctx.set_graph(True)
    for _ in range(3):   # eager, captured, replayed
        assert np.array_equal(ctx.forward(images), three)
    ctx.set_streams(2)
    for _ in range(3):
        assert np.array_equal(ctx.forward(images), three)
    ctx.set_graph(False)
    ctx.close()


_B512 = {}


def _b512():
    if not _B512:
        blob, images = S.make_blob(VIT_B16_512, 0), S.make_images(VIT_B16_512, 1, 4)
        _B512.update(blob=blob, images=images, ref=O.vit_forward(VIT_B16_512, blob, images))
    return _B512


def test_vit_b16_512_bf16_matches_the_oracle():
    d = _b512()
    got, _ = _forward(VIT_B16_512, d["blob"], d["images"], BF16)
    e = rel(got, d["ref"])
    print(f"\n[long] ViT-B/16-512 bf16 b4: logits {e:.3e}")
    assert np.isfinite(got).all() and e <= MODEL_TOL[BF16], e


def test_vit_b16_512_fp16_inside_the_north_star_tolerance():
    # 16 images (tools/long_seq_bench.py --parity 16, profiles/long_seq_vit_b16_512_parity.txt): median 7.5e-4, worst 8.6e-4,
    # all 16 inside 1e-3; these are the first 4 of them
    d = _b512()
    got, _ = _forward(VIT_B16_512, d["blob"], d["images"], FP16)
    assert np.isfinite(got).all()
    per = np.abs(got - d["ref"]).max(1) / np.abs(d["ref"]).max()
    print(f"\n[long] ViT-B/16-512 fp16 b4: per-image {np.array2string(per, precision=3)}")
    assert np.median(per) <= 1e-3 and per.max() <= MODEL_TOL[FP16], per
