"""GPU suite of the rotary model switch, VH_FLAG_ROPE: the rotation kernel through vh_op_rope (both q|k|v layouts, every head dim
class, exact assertions on tables of zeros and ones, one 16-bit ulp against float64 on seeded tables, canaries around everything it
may not write); whole forwards of the three Hugging Face DINOv3 fixtures (identity head: the logits ARE pooler_output, and so are debug tap 1 and
vh_read_features' normalised class token), which the same blob with the flag cleared misses by far; both q|k|v layouts of a ViT-B/16 forward;
bit invariance across batch, streams and graph replay; attention maps; forged blobs.  Tolerances: the project's model bounds (fp16
1e-3, bf16 1e-2, fp8 `1.5 x emulation + 1e-3`), the operator bound for the kernel, test_gpu_attention_maps.TOL for the maps."""
import glob
import os

import numpy as np
import pytest

import hf_state_dicts as HF
import vh_synth as S
import vit_ref as R
from test_gpu_attention_maps import TOL as MAPS_TOL
from vh_testlib import _KEEP, _release_buffers, dev, rel, same_bits

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16", FP8: "fp8"}
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}   # test_gpu_ops.ULP
MODEL_TOL = {FP16: 1e-3, BF16: 1e-2}        # test_gpu_vit.TOL
ROPE, REG = vithip.FLAG_ROPE, vithip.FLAG_REGISTERS
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = HF.DINOV3_EPS
CANARY = 4   # rows in front of and behind the buffer the kernel is given


def fixture(name):
    path, = glob.glob(os.path.join(HERE, "golden", "dinov3", name + "_s*.npz"))
    return np.load(path), HF.fixture_cfg(name), HF.fixture_flags(name), HF.fixture_blob(name)


# ---- 1. the kernel through vh_op_rope -----------------------------------------------------------------------------------------------
def _inputs(dt, batch, tokens, heads, hd, seed):
    """Row-major q|k|v [batch * tokens][3 heads hd] as 16-bit bits and as the float32 values they hold; no zero among them (a product
    with a zero table entry may not flip the sign of a zero)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((batch * tokens, 3 * heads * hd)).astype(np.float32) * np.float32(1.5)
    bits = vithip.to16(v, dt)
    val = vithip.from16(bits, dt)
    bits[val == 0] = vithip.to16(np.ones(1, np.float32), dt)[0]
    return bits, vithip.from16(bits, dt)


def _run(bits, dt, batch, tokens, heads, hd, lead, hm_rows, cos, sin):
    """The buffer with CANARY rows of a pattern around it through vh_op_rope; returns the whole buffer's bits afterwards."""
    flat = np.ascontiguousarray(bits).reshape(-1)
    width = 64 if hm_rows else 3 * heads * hd
    pad = np.full(CANARY * width, 0x7B5A, np.uint16)
    d = dev(np.concatenate([pad, flat, pad]))
    vithip.op_rope(d.ptr + pad.nbytes, dt, batch, tokens, heads, hd, lead, hm_rows, dev(cos).ptr, dev(sin).ptr)
    out = d.to_numpy(np.uint16, (flat.size + 2 * pad.size,))
    assert np.array_equal(out[:pad.size], pad) and np.array_equal(out[-pad.size:], pad), "a canary row was written"
    return out[pad.size:-pad.size].reshape(bits.shape)


KERNEL_CASES = [("row", 32), ("row", 64), ("row", 80), ("row", 128), ("hm", 64), ("hm_padded", 64)]


@pytest.mark.parametrize("layout,hd", KERNEL_CASES, ids=[f"{l}_hd{h}" for l, h in KERNEL_CASES])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_rope_kernel(dt, layout, hd):
    batch, heads, worst = 3, (2 if hd == 128 else 3), 0.0
    for lead in (0, 1, 5):
        for NP in (9, 16):
            tokens, half = lead + NP, hd // 2
            rows = batch * tokens
            hm_rows = 0 if layout == "row" else rows if layout == "hm" else 256
            bits, val = _inputs(dt, batch, tokens, heads, hd, [hd, lead, NP, dt])
            buf = vithip.pack_head_major(bits, heads, hm_rows, fill=0x3C11) if hm_rows else bits

            def rowmajor(out):   # what the kernel left, back as [batch, tokens, 3, heads, hd]; the padding rows checked on the way
                if hm_rows:
                    assert np.array_equal(out[:, :, rows:], buf[:, :, rows:]), "a tile-padding row was written"
                    out = out[:, :, :rows].transpose(2, 0, 1, 3)
                return np.ascontiguousarray(out).reshape(batch, tokens, 3, heads, hd)

            x = bits.reshape(batch, tokens, 3, heads, hd)
            one, zero = np.ones((NP, half), np.float32), np.zeros((NP, half), np.float32)
            # cos 1, sin 0: nothing changes
            assert np.array_equal(rowmajor(_run(buf, dt, batch, tokens, heads, hd, lead, hm_rows, one, zero)), x), (lead, NP)
            # cos 0, sin 1: out[d] = -x[d + hd/2], out[d + hd/2] = x[d], exactly; v and the lead rows as they were
            got = rowmajor(_run(buf, dt, batch, tokens, heads, hd, lead, hm_rows, zero, one))
            want = x.copy()
            want[:, lead:, :2, :, :half] = x[:, lead:, :2, :, half:] ^ np.uint16(0x8000)
            want[:, lead:, :2, :, half:] = x[:, lead:, :2, :, :half]
            assert np.array_equal(got, want), (lead, NP)
            # seeded tables against float64 of the stated function
            a = np.pi * S.fill(NP * half, 1000 + NP + lead, R.TID_ROPE, 0).astype(np.float64).reshape(NP, half)
            cos, sin = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
            got = rowmajor(_run(buf, dt, batch, tokens, heads, hd, lead, hm_rows, cos, sin))
            assert np.array_equal(got[:, :lead], x[:, :lead]) and np.array_equal(got[:, :, 2], x[:, :, 2]), "v or a lead row was written"
            v64 = val.astype(np.float64).reshape(batch, tokens, 3, heads, hd)[:, lead:, :2]
            ref = R.rotate_rows(v64.transpose(0, 2, 3, 1, 4), cos.astype(np.float64), sin.astype(np.float64)).transpose(0, 3, 1, 2, 4)
            g = vithip.from16(got, dt).astype(np.float64).reshape(got.shape)[:, lead:, :2]
            tol = ULP[dt] * (np.abs(ref) + np.abs(ref).max(-1, keepdims=True))
            bad = np.abs(g - ref) > tol
            worst = max(worst, float((np.abs(g - ref) / tol).max()))
            assert not bad.any(), (lead, NP, int(bad.sum()), float(np.abs(g - ref).max()))
            for b in _KEEP:
                b.free()
            del _KEEP[:]
    print(f"\n[rope] kernel {NAME[dt]} {layout} hd {hd}: worst |d| / bound = {worst:.3f}")


def test_rope_tap_refusals():
    d, t = dev(np.zeros(4096, np.uint16)), dev(np.zeros(4096, np.float32))
    for args, text in (((FP8, 1, 4, 1, 64, 1, 0), "dtype is not"), ((BF16, 0, 4, 1, 64, 1, 0), "batch must be positive"),
                       ((BF16, 1, 4, 1, 72, 1, 0), "head_dim must be"), ((BF16, 1, 4, 1, 64, 4, 0), "lead outside"),
                       ((BF16, 1, 4, 1, 80, 1, 8), "exists at head_dim 64 only"),
                       ((BF16, 2, 4, 1, 64, 1, 7), "hm_rows holds fewer than batch")):
        with pytest.raises(vithip.VhError, match=text):
            vithip.op_rope(d.ptr, *args, t.ptr, t.ptr)
    with pytest.raises(vithip.VhError, match="16-byte aligned"):
        vithip.op_rope(d.ptr + 2, BF16, 1, 4, 1, 64, 1, 0, t.ptr, t.ptr)
    with pytest.raises(vithip.VhError, match="null pointer"):
        vithip.op_rope(d.ptr, BF16, 1, 4, 1, 64, 1, 0, None, t.ptr)


# ---- 2., 3. whole forwards of the fixtures, with the flag and without ------------------------------------------------------------------
@pytest.mark.parametrize("lnf", [0, vithip.FLAG_LN_FOLD_OFF], ids=["default", "fold_off"])
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_outputs(name, dt, lnf):
    """Identity head: the logits are pooler_output; so are debug tap 1 (the head's input) and vh_read_features' normalised class token."""
    z, cfg, flags, blob = fixture(name)
    images = z["images"]
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags | lnf, ln_eps=EPS)
    ctx.load_weights(blob)
    got, fold = ctx.forward(images), ctx.ln_fold()
    tap = ctx.debug_read(1, got.size).reshape(got.shape)
    feat = ctx.read_features(cls=True, patch=False)["cls"]
    ctx.close()
    e = rel(got, z["pooler_output"])
    print(f"\n[rope] fixture {name} {NAME[dt]} (fold {fold}): pooler_output {e:.3e} (bound {MODEL_TOL[dt]:g}); tap 1 {rel(tap, z['pooler_output']):.3e}")
    assert np.isfinite(got).all() and e <= MODEL_TOL[dt], e
    assert rel(tap, z["pooler_output"]) <= MODEL_TOL[dt] and rel(feat, z["pooler_output"]) <= MODEL_TOL[dt]
    assert fold == (cfg["dim"] % 256 == 0 and not lnf)


@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_is_missed_with_the_flag_cleared(name, dt):
    """The same blob minus its two tensors on a context without the flag: another function, more than ten bounds away."""
    z, cfg, flags, blob = fixture(name)
    blob0, flags0 = R.without_rope(cfg, blob, flags)
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(z["images"]), flags=flags0, ln_eps=EPS)
    ctx.load_weights(blob0)
    got = ctx.forward(z["images"])
    ctx.close()
    e = rel(got, z["pooler_output"])
    print(f"\n[rope] fixture {name} {NAME[dt]} without the flag: {e:.3e} (bound {MODEL_TOL[dt]:g})")
    assert np.isfinite(got).all() and e > 10 * MODEL_TOL[dt], e


@pytest.mark.parametrize("lnf", [0, vithip.FLAG_LN_FOLD_OFF], ids=["default", "fold_off"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_fp8_forwards_track_the_emulation(name, lnf):
    z, cfg, flags, blob = fixture(name)
    images = z["images"]
    ref32 = z["pooler_output"].astype(np.float32)
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
    ctx = vithip.VitContext(cfg, dtype=FP8, max_batch=len(images), flags=flags | lnf, ln_eps=EPS)
    ctx.load_weights(blob)
    got, folded = ctx.forward(images), ctx.ln_fold()
    ctx.close()
    emu = R.forward(cfg, blob, images, flags, EPS, fp8="folded" if folded else "plain")
    r_emu32, r_gpu32, r_gpuemu = rms(emu, ref32), rms(got, ref32), rms(got, emu)
    print(f"\n[rope fp8] {name} (folded {folded}): rms emu-fp32 {r_emu32:.3e} gpu-fp32 {r_gpu32:.3e} gpu-emu {r_gpuemu:.3e}")
    assert np.isfinite(got).all()
    assert r_gpu32 <= 1.5 * r_emu32 + 1e-3 and r_gpuemu <= 1.5 * r_emu32 + 1e-3


# ---- 4. both q|k|v layouts ---------------------------------------------------------------------------------------------------------------
def test_both_qkv_layouts_of_a_vit_b16_forward(monkeypatch):
    """ViT-B/16 shape, two layers, bf16 at batch 224 keeps q|k|v head-major; a context created under VH_QKV_HM=0 keeps it row-major
    (test_gpu_attention_maps).  With FLAG_ROPE both are the same bits, and three of the images are within the bf16 bound of vit_ref
    (an image's logits do not depend on the batch, so the reference runs those three alone)."""
    cfg = dict(S.CONFIGS["vit_base"], layers=2)
    batch, pick = 224, [0, 100, 223]
    px = cfg["image_size"] ** 2 * cfg["channels"]
    din, dout = vithip.DeviceBuffer(batch * px * 4), vithip.DeviceBuffer(batch * cfg["classes"] * 4)
    used, logits, blob = [], [], None
    for hm in ("1", "0"):
        monkeypatch.setenv("VH_QKV_HM", hm)
        ctx = vithip.VitContext(cfg, dtype=BF16, max_batch=batch, flags=ROPE)
        ctx.init_weights_seeded(0)
        blob = ctx.export_weights()
        ctx.fill_input_seeded(1, batch, din.ptr)
        ctx.forward_device(din.ptr, batch, dout.ptr)
        used.append(int(ctx.debug_read(4, 1)[0]))
        logits.append(dout.to_numpy(np.float32, (batch, cfg["classes"])))
        ctx.close()
    first = din.to_numpy(np.float32, (px,))
    din.free(); dout.free()
    assert used == [1, 0], used
    assert np.isfinite(logits[0]).all() and np.array_equal(logits[0], logits[1])
    # the seeded tables are the reference's (host cosine and sine of the same angles: the same floats but for libm's last bit)
    t = R.unpack_blob(cfg, blob, ROPE)
    cos, sin = R.seeded_tables(cfg, 0)
    assert np.abs(t["rope.cos"] - cos).max() <= 2.0 ** -24 and np.abs(t["rope.sin"] - sin).max() <= 2.0 ** -24
    images = np.stack([S.fill(px, 1, 0x100, 0, start=i * px) for i in pick]).reshape(len(pick), cfg["image_size"], cfg["image_size"], cfg["channels"])
    assert np.array_equal(images[0].reshape(-1), first)
    ref = R.forward(cfg, blob, images, ROPE)
    e = rel(logits[0][pick], ref)
    print(f"\n[rope] ViT-B/16 x 2 layers bf16 b{batch}, head-major and row-major: {e:.3e} (bound {MODEL_TOL[BF16]:g})")
    assert e <= MODEL_TOL[BF16]
    # and the flag matters at this shape too
    assert rel(R.forward(cfg, R.without_rope(cfg, blob, ROPE)[0], images, 0), ref) > 10 * MODEL_TOL[BF16]


# ---- 5. the same logit bits on every route into a forward ---------------------------------------------------------------------------------
MID = dict(image_size=40, patch_size=8, channels=3, dim=256, heads=4, mlp_dim=512, layers=2, classes=40)       # folds; hd 64
SMALL = dict(image_size=32, patch_size=8, channels=3, dim=128, heads=2, mlp_dim=256, layers=2, classes=40)     # the fp32 residual path
HD80 = dict(image_size=24, patch_size=8, channels=3, dim=320, heads=4, mlp_dim=384, layers=2, classes=40)      # the head-dim kernel


def context(cfg, dt, flags, max_batch=5, seed=5):
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=max_batch, flags=flags, ln_eps=EPS)
    ctx.load_weights(R.make_blob(cfg, seed, flags, EPS))
    return ctx


@pytest.mark.parametrize("cfg,dt", [(MID, BF16), (MID, FP8), (SMALL, FP16), (HD80, BF16)], ids=["mid_bf16", "mid_fp8", "small_fp16", "hd80_bf16"])
def test_same_logit_bits_alone_in_a_batch_across_streams_and_graph_replay(cfg, dt):
    flags = ROPE | REG(4)
    images = S.make_images(cfg, 8, 5)
    ctx = context(cfg, dt, flags)
    five = ctx.forward(images)
    assert np.isfinite(five).all()
    if dt != FP8:   # a seeded model with a seeded head against the reference, at the model bound
        assert rel(five, R.forward(cfg, R.make_blob(cfg, 5, flags, EPS), images, flags, EPS)) <= MODEL_TOL[dt]
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
    # new weights drop the captured graphs: another seed is another function, the first seed again the first bits
    ctx.set_graph(True)
    ctx.load_weights(R.make_blob(cfg, 6, flags, EPS))
    assert not same_bits(ctx.forward(images), five)
    ctx.load_weights(R.make_blob(cfg, 5, flags, EPS))
    assert same_bits(ctx.forward(images), five)
    ctx.close()


# ---- 6. attention maps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [FP16, BF16], ids=lambda d: NAME[d])
def test_attention_maps_are_of_the_rotated_q_and_k(dt):
    z, cfg, flags, blob = fixture("a")
    images, L = z["images"], cfg["layers"]
    ctx = vithip.VitContext(cfg, dtype=dt, max_batch=len(images), flags=flags, ln_eps=EPS)
    ctx.load_weights(blob)
    ctx.set_attention_layers(list(range(1, L + 1)), vithip.ATTN_Q_LEAD)
    ctx.forward(images)
    Q = ctx.attention_dims()[2]
    assert Q == 5
    blob0, flags0 = R.without_rope(cfg, blob, flags)
    for k in range(1, L + 1):
        got = ctx.read_attention(k)["probs"]
        ref = R.forward(cfg, blob, images, flags, EPS, lead_probs=(k, Q))
        unrotated = R.forward(cfg, blob0, images, flags0, EPS, lead_probs=(k, Q))
        err = float(np.abs(got - ref).max())
        print(f"\n[rope] maps {NAME[dt]} layer {k}: max |p - p_ref| = {err:.3e} (tol {MAPS_TOL[dt]:.3e}); the unrotated model's rows differ by {np.abs(unrotated - ref).max():.3e}")
        assert got.shape == ref.shape and err <= MAPS_TOL[dt]
        assert np.abs(unrotated - ref).max() > 10 * MAPS_TOL[dt]                      # the test can tell the two apart
    ctx.close()


# ---- 7. a blob of another model is refused; the seeded tensors ---------------------------------------------------------------------------
def test_a_blob_whose_bit_differs_is_refused_by_name(tmp_path):
    cfg, flags = SMALL, ROPE | REG(4)
    ctx = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=flags, ln_eps=EPS)
    ctx.init_weights_seeded(17)
    blob = ctx.export_weights()
    want_blob = R.make_blob(cfg, 17, flags, EPS)
    n = 2 * 4 * int(np.prod(R.rope_shape(cfg)))
    assert np.array_equal(blob[:-n], want_blob[:-n])                                  # header bit 23 and every other tensor
    assert np.abs(blob[-n:].view(np.float32) - want_blob[-n:].view(np.float32)).max() <= 2.0 ** -24
    path = str(tmp_path / "m.vhblob")
    ctx.save_weights_file(path)
    assert vithip.blob_file_flags(path) == flags
    images = S.make_images(cfg, 2, 2)
    want = ctx.forward(images)
    ctx.load_weights_file(path)
    assert same_bits(ctx.forward(images), want)
    forged = blob.copy()
    forged[52:56] = np.array([int(REG(4))], np.uint32).view(np.uint8)                 # the right size, bit 23 cleared
    with pytest.raises(vithip.VhError, match=r"header bit 23 \(rotary position embedding\) is 0, the context's VH_FLAG_ROPE is 1") as e:
        ctx.load_weights(forged)
    assert e.value.code == 1
    with pytest.raises(vithip.VhError, match="bytes, expected"):                      # the blob of the model without the flag: its size speaks
        ctx.load_weights(R.without_rope(cfg, blob, flags)[0])
    assert same_bits(ctx.forward(images), want)                                       # the refused loads changed nothing
    ctx.close()
    plain = vithip.VitContext(cfg, dtype=FP16, max_batch=2, flags=REG(4), ln_eps=EPS)  # and the reverse
    blob0 = R.without_rope(cfg, blob, flags)[0]
    forged0 = blob0.copy()
    forged0[52:56] = np.array([int(REG(4)) | ROPE], np.uint32).view(np.uint8)
    with pytest.raises(vithip.VhError, match=r"header bit 23 \(rotary position embedding\) is 1, the context's VH_FLAG_ROPE is 0"):
        plain.load_weights(forged0)
    with pytest.raises(vithip.VhError, match="bytes, expected"):
        plain.load_weights(blob)
    plain.load_weights(blob0)
    assert not same_bits(plain.forward(images), want)                                 # the same tensors without the rotation: another function
    plain.close()
