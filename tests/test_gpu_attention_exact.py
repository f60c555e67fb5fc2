"""GPU, per element: every attention launch path against exactly predictable inputs (tests/attn_exact.py).

The operator tests of test_gpu_ops / test_gpu_long_sequence / test_gpu_head_dim bound ONE number, max|d| / max|ref|, on inputs
whose softmax is nearly flat: an unmasked padded key, a dropped last key or a fault confined to small outputs stays below it at
long sequences, and the deferred rescale runs for one query.  Here the scores are exact integers, so every element has to be the
correctly rounded quotient (uniform and graded designs: the key masks at every tail remainder, probabilities up to 2^8 under a
stale shift) or a V row bit for bit (permutation design: rescales in every wave, several per row).  test_attention_exact.py
proves on the CPU that these assertions fail for one key too many, one too few and a neighbouring head's V.

Every output buffer is pre-filled with 0xFF bytes (an unwritten element reads back as NaN, which assert_elements refuses) and
carries one guard row in front of and behind it that must stay 0xFF.
"""
import numpy as np
import pytest

import attn_exact as X
from vh_testlib import _release_buffers, dev

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8 = X.BF16, X.FP16, X.FP8
DT = [BF16, FP16]
HEAD_DIMS = [32, 48, 64, 80, 96, 112, 128]   # test_gpu_head_dim.HEAD_DIMS
# test_gpu_ops.test_attention_token_counts_around_every_kernel_boundary
BOUNDARY_T = [33, 64, 65, 96, 97, 100, 128, 129, 160, 161, 193, 200, 208, 209, 224, 225, 256, 289, 384, 385, 512, 513, 608, 609, 640]

_CASES = {}
_WORST = {}   # (tap, type) -> worst (|d| - step * |ref|) / max|V| seen: the margin under attn_exact.EXTRA_REL


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    for (tap, dt), v in sorted(_WORST.items()):
        print(f"\nworst (|d| - step*|ref|) / max|V|  {tap:<10} {X.NAME[dt]:<5} {v:+.3e}   (extra = {X.EXTRA_REL:.3e})", end="")
    print()


def case_ref(design, batch, tokens, heads, hd=64, vdtype=FP16, rows=None):
    """A case and its float64 reference, generated once and shared unchanged (the integer designs serve both types)."""
    key = (design, batch, tokens, heads, hd, vdtype if design == "permutation" else None, None if rows is None else tuple(rows))
    if key not in _CASES:
        if len(_CASES) > 64:   # the sweeps visit hundreds of shapes once each: keep the cache small
            _CASES.clear()
        case = X.make_case(design, batch, tokens, heads, hd, seed=tokens + hd, vdtype=vdtype)
        ref = None if design == "permutation" else X.reference(case, rows)
        case.qkv.setflags(write=False)
        if ref is not None:
            ref.setflags(write=False)
        _CASES[key] = (case, ref)
    return _CASES[key]


def launch(tap, case, dt, rows_out=None, twice=False):
    """Run one tap on a case; returns the stored result [rows][dim] (uint16, or e4m3 bytes for FP8) after checking the guards."""
    B, T, H, hd, D = case.batch, case.tokens, case.heads, case.hd, case.dim
    rows = B * T if rows_out is None else rows_out
    esz = 1 if dt == FP8 else 2
    src = dev(vithip.to16(case.qkv, BF16 if dt == FP8 else dt))
    buf = dev(np.full((rows + 2) * D * esz, 0xFF, dtype=np.uint8))
    out = buf.ptr + D * esz
    for _ in range(2 if twice else 1):
        if tap == "resident":
            vithip.op_attention(src.ptr, B, T, H, out, dt)
        elif tap == "stream":
            vithip.op_attention_stream(src.ptr, B, T, H, out, dt)
        elif tap == "hd":
            vithip.op_attention_hd(src.ptr, B, T, H, hd, out, dt)
        elif tap == "cls":
            vithip.op_attention_cls(src.ptr, B, T, H, out, dt)
        else:
            raise ValueError(tap)
    raw = buf.to_numpy(np.uint8, ((rows + 2), D * esz))
    assert np.all(raw[0] == 0xFF) and np.all(raw[-1] == 0xFF), f"{tap} T = {T}: a guard row around the output was written"
    body = raw[1:-1]
    return body if dt == FP8 else np.ascontiguousarray(body).view(np.uint16)


def values(bits, dt):
    return vithip.from_e4m3(bits) if dt == FP8 else vithip.from16(bits, dt)


def check(tap, design, dt, batch, tokens, heads, hd=64, twice=False):
    """One launch, one design: bit equality for the permutation design, the per-element bound for the others."""
    cls = tap == "cls"
    case, ref = case_ref(design, batch, tokens, heads, hd, vdtype=dt, rows=[0] if cls else None)
    bits = launch(tap, case, dt, rows_out=batch if cls else None, twice=twice)
    rpi = 1 if cls else None
    if design == "permutation":
        want = case.expected_permutation()
        if cls:
            want = want[::tokens]
        X.assert_bits(bits, X.to_bits(want, dt), case, dt, tap, rows_per_image=rpi)
    else:
        got = values(bits, dt)
        X.assert_elements(got, ref, dt, case, tap, rows_per_image=rpi)
        _WORST[(tap, dt)] = max(_WORST.get((tap, dt), -1.0), X.excess(got, ref, dt))


# ---- key masks at every tail remainder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["uniform", "graded"])
@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
def test_mask_sweep_resident_dispatcher(dt, design):
    # every T in 1..256 (all 32 remainders in the one-shot, staged-ring and ring forms, all four values of ng), the boundary
    # counts of test_attention_token_counts_around_every_kernel_boundary, and 609..640 up to the LDS limit
    for tokens in sorted(set(range(1, 257)) | set(BOUNDARY_T) | set(range(609, 641))):
        check("resident", design, dt, 2, tokens, 2)


@pytest.mark.parametrize("design", ["uniform", "graded"])
@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
def test_mask_sweep_stream_tap(dt, design):
    # 1..96: fewer than four waves share the DMA pieces, 1, 2 and 3 tiles (the ring depth); 641..672: every remainder just above
    # the dispatcher's threshold; two slabs and more at 1025 / 1057; the longest sequence
    for tokens in list(range(1, 97)) + list(range(641, 673)):
        check("stream", design, dt, 2, tokens, 2)
    for tokens in (1025, 1057):
        check("stream", design, dt, 3, tokens, 2)
    check("stream", design, dt, 1, 4097, 2)


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_mask_sweep_head_dim_tap(hd, dt):
    for design in ("uniform", "graded"):
        for tokens in list(range(1, 65)) + [197, 257, 1025]:
            check("hd", design, dt, 2, tokens, 2, hd)
        if hd in (48, 80, 128):
            check("hd", design, dt, 1, 4097, 2, hd)


# ---- the deferred rescale in every wave: bit equality ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("tokens", [33, 97, 197, 577, 640])
def test_rescale_permutation_resident_dispatcher(tokens, dt):
    check("resident", "permutation", dt, 2, tokens, 2)


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("tokens", [65, 1025, 4097])
def test_rescale_permutation_stream_tap(tokens, dt):
    check("stream", "permutation", dt, 2, tokens, 2)


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_rescale_permutation_head_dim_tap(hd, dt):
    for tokens in (257, 1025):
        check("hd", "permutation", dt, 2, tokens, 2, hd)


# ---- persistent paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["permutation", "uniform"])
@pytest.mark.parametrize("batch,tokens,heads", [(92, 197, 12), (25, 577, 12)])   # test_attention_persistent_workgroups_walk_several_items
def test_persistent_paths(batch, tokens, heads, design):
    # staged ring: two static items per workgroup, then tickets from the work queue; plain ring: K/V shared by a head's slabs and
    # refilled for the next head.  Launched twice: the queue counter is re-armed by every launch.
    check("resident", design, FP16, batch, tokens, heads, twice=True)


# ---- e4m3 output (bf16 q|k|v in) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["permutation", "graded"])
@pytest.mark.parametrize("tap,tokens,hd", [("resident", 197, 64), ("resident", 785, 64), ("stream", 97, 64),
                                           ("hd", 257, 48), ("hd", 257, 80), ("hd", 257, 128)])
def test_e4m3_output(tap, tokens, hd, design):
    check(tap, design, FP8, 2, tokens, 2, hd)


# ---- the class-token kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", X.DESIGNS)
@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
def test_class_token_tap(dt, design):
    # batch * heads = 15 is no multiple of the four waves of a workgroup; query row 0 only, against row 0 of the reference
    for tokens in list(range(1, 131)) + [197, 577, 785, 1024]:
        check("cls", design, dt, 5, tokens, 3)


def test_class_token_tap_refusals():
    case, _ = case_ref("uniform", 1, 1025, 1)
    src = dev(vithip.to16(case.qkv, FP16))
    out = dev(np.full(64 * 2, 0xFF, dtype=np.uint8))
    for args in ((src.ptr, 1, 1025, 1, out.ptr, FP16), (src.ptr, 1, 64, 1, out.ptr, FP8), (None, 1, 64, 1, out.ptr, FP16),
                 (src.ptr, 1, 64, 1, None, FP16), (src.ptr, 0, 64, 1, out.ptr, FP16)):
        with pytest.raises(vithip.VhError) as e:
            vithip.op_attention_cls(*args)
        assert e.value.code == 1, args   # VH_ERR_INVALID, on the host, before any launch
    assert np.all(out.to_numpy(np.uint8, (128,)) == 0xFF)


# ---- head-major input, 16-row-blocked output ------------------------------------------------------------------------------
def run_layout(case, dt, out_tiled, head_major, hm_rows):
    B, T, H, D = case.batch, case.tokens, case.heads, case.dim
    rows, esz, chunk = B * T, (1 if dt == FP8 else 2), (16 if dt == FP8 else 8)
    q16 = vithip.to16(case.qkv, BF16 if dt == FP8 else dt)
    src = dev(vithip.pack_head_major(q16, H, hm_rows, fill=0xFFFF) if head_major else q16)   # padding rows: NaN if ever read
    nrows = (rows + 15) // 16 * 16 if out_tiled else rows
    slab = 16 * D * esz                                   # one row block in front of and behind the buffer
    buf = dev(np.full(2 * slab + nrows * D * esz, 0xFF, dtype=np.uint8))
    vithip.op_attention_layout(src.ptr, B, T, H, buf.ptr + slab, dt, out_tiled, hm_rows if head_major else 0)
    raw = buf.to_numpy(np.uint8, (2 * slab + nrows * D * esz,))
    assert np.all(raw[:slab] == 0xFF) and np.all(raw[-slab:] == 0xFF), "a canary slab around the output was written"
    body = raw[slab:-slab] if dt == FP8 else np.ascontiguousarray(raw[slab:-slab]).view(np.uint16)
    if not out_tiled:
        return body.reshape(rows, D)
    full = vithip.unpack_tiled(body, nrows, D, chunk)
    assert np.all(full[rows:] == (0xFF if dt == FP8 else 0xFFFF)), "rows of the last 16-row block beyond batch * T were written"
    return full[:rows]


@pytest.mark.parametrize("padded", [False, True], ids=["exact_rows", "rows_padded_to_256"])
@pytest.mark.parametrize("dt", [FP16, BF16, FP8], ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("batch,tokens,heads", [(4, 197, 2), (2, 577, 2), (3, 200, 4)])
def test_layout_tap(batch, tokens, heads, dt, padded):
    hm_rows = (batch * tokens + 255) // 256 * 256 if padded else batch * tokens
    for design in ("permutation", "graded"):
        case, ref = case_ref(design, batch, tokens, heads, 64, vdtype=dt)
        base = launch("resident", case, dt)   # vh_op_attention on the same data
        for out_tiled, head_major in ((False, False), (True, False), (True, True)):
            bits = run_layout(case, dt, out_tiled, head_major, hm_rows)
            what = f"layout(tiled={out_tiled}, head_major={head_major}, hm_rows={hm_rows})"
            if design == "permutation":
                X.assert_bits(bits, X.to_bits(case.expected_permutation(), dt), case, dt, what)
            else:
                X.assert_elements(values(bits, dt), ref, dt, case, what)
                _WORST[("layout", dt)] = max(_WORST.get(("layout", dt), -1.0), X.excess(values(bits, dt), ref, dt))
            X.assert_bits(bits, base, case, dt, what + " vs op_attention")


def test_layout_tap_refusals():
    case, _ = case_ref("uniform", 2, 197, 2)
    src = dev(vithip.to16(case.qkv, FP16))
    out = dev(np.full(400 * 128 * 2, 0xFF, dtype=np.uint8))
    rows = 2 * 197
    bad = [(src.ptr, 2, 197, 2, out.ptr, FP16, False, rows),        # head-major without the tiled output
           (src.ptr, 2, 197, 2, out.ptr, FP16, True, rows - 1),     # in_hm_rows < batch * tokens
           (src.ptr, 2, 33, 2, out.ptr, FP16, True, 0),             # the one-shot form has no tiled output
           (src.ptr, 2, 197, 3, out.ptr, FP16, True, 0),            # odd head count
           (src.ptr, 1, 785, 2, out.ptr, FP16, True, 0),            # beyond the LDS limit: the streaming kernel, row-major only
           (None, 2, 197, 2, out.ptr, FP16, True, 0), (src.ptr, 2, 197, 2, None, FP16, True, 0)]
    for args in bad:
        with pytest.raises(vithip.VhError) as e:
            vithip.op_attention_layout(*args)
        assert e.value.code == 1, args   # VH_ERR_INVALID, on the host, before any launch
    assert np.all(out.to_numpy(np.uint8, (400 * 128 * 2,)) == 0xFF)
