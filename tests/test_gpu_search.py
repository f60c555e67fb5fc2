"""GPU suite of the embedding search (include/vithip.h, "Embedding search").  On small-integer operands every product and partial sum
is exact, so index and score must equal the float64 reference bit for bit, ties included; on real values the scores are bounded by
the roundings of the fp32 sum; a context's search is pinned, bit for bit, to the tap on the rows the head multiplied."""
import ctypes as C
import functools

import numpy as np
import pytest

import features_ref as R
import search_ref as SR
import vh_synth as S
import vit_ref
import vithip

pytestmark = pytest.mark.gpu

VH_ERR_INVALID = 1
BF16, FP16 = vithip.DTYPE_BF16, vithip.DTYPE_FP16
TYPES = pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
EPS = 1e-6


def dev(a):
    return vithip.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def run_tap(q, d_bank, n, k, dtype, normalise=0):
    """vh_op_search of fp32 rows q against a device bank -> (index, score); the outputs start as garbage."""
    nq, w = q.shape
    bufs = [dev(q.astype(np.float32)), vithip.DeviceBuffer(vithip.op_search_workspace_bytes(nq, n, k)),
            dev(np.full(nq * k, -7, np.int32)), dev(np.full(nq * k, np.nan, np.float32))]
    vithip.op_search(bufs[0].ptr, nq, w, normalise, d_bank.ptr, n, dtype, k, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
    out = bufs[2].to_numpy(np.int32, (nq, k)), bufs[3].to_numpy(np.float32, (nq, k))
    for b in bufs:
        b.free()
    return out


def assert_exact(got, ref, what):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].astype(np.float64), ref[1]), what


# ---- 1. exact, operator level -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_case(w):
    """Operands in -3 .. 3 (exact in both types, |sum| <= 9 w < 2^24) and the reference's first 32 per n, computed once."""
    rng = np.random.default_rng(w)
    nmax = 70001 if w <= 1040 else 1000   # 2064: the 16-query block, at the small sizes
    q, b = rng.integers(-3, 4, (200, w)).astype(np.float64), rng.integers(-3, 4, (nmax, w)).astype(np.float64)
    s = (q.astype(np.float32) @ b.astype(np.float32).T).astype(np.float64)   # (exact in fp32 too, and twice as fast)
    return q, b, {n: SR.topk(s[:, :n], 32) for n in (1, 31, 33, 1000, 70001) if n <= nmax}   # (a query's result does not depend on nq)


@pytest.mark.parametrize("w", [16, 80, 1040, 2064])   # query blocks of 64, 64, 32 and 16 rows
@TYPES
def test_op_search_is_exact_on_small_integers(dtype, w):
    q, b, refs = integer_case(w)
    assert vithip.op_search_slabs(200, 70001) > 1   # several slabs, the last one ending in a partial tile
    d_bank = dev(vithip.to16(b.astype(np.float32), dtype))
    for n, (index, score) in refs.items():
        for nq in (1, 33, 65, 200):
            for k in (1, 5, 32):   # the first k of the first 32; with n < k the tail is -1 / -inf
                assert_exact(run_tap(q[:nq], d_bank, n, k, dtype), (index[:nq, :k], score[:nq, :k]), (n, nq, k))
    d_bank.free()


# ---- 2. placements that exercise the selection --------------------------------------------------------------------------------
def placed(kind, n=4129, nq=33):
    """q [nq, 16] and b [n, 16] whose scores are exact integers placed as `kind` says."""
    rng = np.random.default_rng(7)
    q, b = np.zeros((nq, 16)), np.zeros((n, 16))
    m = np.arange(n)
    if kind in ("ascending", "descending"):   # score = +-m + i: every item (no item) passes the running threshold
        q[:, 0], q[:, 1], q[:, 2] = 1, 64, np.arange(nq)
        b[:, 0], b[:, 1], b[:, 2] = m % 64, m // 64, 1
        if kind == "descending":
            b[:, :2] *= -1
    elif kind == "equal":
        q[:, 0], b[:, 0] = 2, 3
    else:   # random small scores, and 32 winners 300 above them: the last rows (a partial tile) or the first tile
        q[:, :15], b[:, :15] = rng.integers(-3, 4, (nq, 15)), rng.integers(-3, 4, (n, 15))
        q[:, 15] = 3
        b[n - 32:n if kind == "last" else 32, 15] = 100
        b[:32 if kind == "first" else 0, 15] = 100
    return q, b


@pytest.mark.parametrize("kind", ["ascending", "descending", "equal", "last", "first"])
@TYPES
def test_op_search_placements(dtype, kind):
    q, b = placed(kind)
    ref = SR.topk(q @ b.T, 32)
    if kind == "equal":
        assert np.array_equal(ref[0], np.tile(np.arange(32), (33, 1)))
    if kind in ("last", "first"):
        assert np.array_equal(np.sort(ref[0], axis=1), np.tile(np.arange(32) + (4129 - 32 if kind == "last" else 0), (33, 1)))
    d_bank = dev(vithip.to16(b.astype(np.float32), dtype))
    assert_exact(run_tap(q, d_bank, 4129, 32, dtype), ref, kind)
    d_bank.free()


# ---- 3. real values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [0, 1], ids=["raw_queries", "normalised_queries"])
@TYPES
def test_op_search_on_real_values(dtype, normalise):
    """B = (W / 16 + 16) 2^-23 sum_j |q16 b16| -- one fp32 rounding per k-step plus at most 16 inside the instruction, doubled -- and,
    with the device-side norm, one ulp of the 16-bit query (2^-8 bf16, 2^-11 fp16) times the same sum."""
    w, n, nq, k = 768, 5000, 48, 20
    rng = np.random.default_rng(3)
    q, b = rng.standard_normal((nq, w)).astype(np.float32), SR.unit_rows(rng.standard_normal((n, w))).astype(np.float32)
    index, score = run_tap(q, dev(vithip.to16(b, dtype)), n, k, dtype, normalise)
    ref = SR.scores(q, b, dtype, normalise)
    q16 = SR.operand(SR.unit_rows(q) if normalise else q, dtype)
    bound = ((w / 16 + 16) * 2.0 ** -23 + normalise * (2.0 ** -8 if dtype == BF16 else 2.0 ** -11)) * (np.abs(q16) @ np.abs(SR.operand(b, dtype)).T)
    assert index.min() >= 0 and all(len(set(r)) == k for r in index.tolist())   # no index twice
    rows = np.arange(nq)[:, None]
    d, B = np.abs(score - ref[rows, index]), bound[rows, index]
    print(f"search real values {'bf16' if dtype == BF16 else 'fp16'} normalise={normalise}: worst |d| / B = {(d / B).max():.3e}")
    assert (d <= B).all()
    assert (score >= SR.topk(ref, k)[1][:, -1:] - B).all()


# ---- 4. through a context -------------------------------------------------------------------------------------------------------
MICRO = dict(S.CONFIGS["vit_micro"], classes=48)   # (a class count the bank of a CLIP-style search can have: a multiple of 16)


@pytest.mark.parametrize("flags", [0, vithip.FLAG_POOL(vithip.POOL_CLS_AVG)], ids=["cls", "cls_avg"])
@TYPES
def test_search_through_a_context(dtype, flags):
    cfg, L = MICRO, vithip.lib()
    w = cfg["dim"] * (2 if flags else 1)
    rng = np.random.default_rng(w)
    bank, n, k = rng.standard_normal((2500, w)).astype(np.float32), 2500, 5   # two slabs
    ctx = vithip.VitContext(cfg, dtype=dtype, max_batch=3, flags=flags, ln_eps=EPS)
    ctx.load_weights(vit_ref.make_blob(cfg, 5, flags, EPS))
    images = S.make_images(cfg, 3, 3)
    plain = ctx.forward(images)
    assert ctx.bank_dims() == (0, 0)
    unit = SR.unit_rows(bank)
    if dtype == FP16:   # the library normalises in float64 and rounds once: numpy's float64 -> float16
        ctx.set_bank(bank, normalise=True)
        bank16 = unit.astype(np.float16).view(np.uint16)
    else:               # (numpy has no float64 -> bf16 in one rounding: the fp32 rows go in normalised)
        ctx.set_bank(unit.astype(np.float32), normalise=False)
        bank16 = vithip.to16(unit.astype(np.float32), dtype)
    assert ctx.bank_dims() == (n, w) and vithip.op_search_slabs(3, n) == 2
    assert np.array_equal(R.bits(ctx.forward(images)), R.bits(plain))   # the forward does not see the bank
    got = ctx.search(k)
    # (a) bit for bit the tap on the rows the head multiplied, against the bank normalised in float64 and rounded once
    rows = ctx.debug_read(1, 3 * w).reshape(3, w)
    d_bank = dev(bank16)
    tap = run_tap(rows, d_bank, n, k, dtype, 1)
    assert np.array_equal(got[0], tap[0]) and np.array_equal(R.bits(got[1]), R.bits(tap[1]))
    assert (np.diff(got[1], axis=1) <= 0).all() and got[0].min() >= 0
    # (b) image 0: the same bits at batch 1, and after a graph replay through the device entry points
    ctx.forward(images[:1])
    one = ctx.search(k)
    assert np.array_equal(one[0], got[0][:1]) and np.array_equal(R.bits(one[1]), R.bits(got[1][:1]))
    d_in, d_out, d_i, d_s = dev(images), vithip.DeviceBuffer(3 * cfg["classes"] * 4), dev(np.zeros(3 * k, np.int32)), dev(np.zeros(3 * k, np.float32))
    ctx.set_graph(True)
    ctx.forward_device_async(d_in.ptr, 3, d_out.ptr, steps=2)
    ctx.search_device_async(vithip.Search(vithip.SEARCH_HEAD_INPUT, k, 1, 3, None, d_i.ptr, d_s.ptr))
    ctx.synchronize()
    assert np.array_equal(d_i.to_numpy(np.int32, (3, k)), got[0]) and np.array_equal(R.bits(d_s.to_numpy(np.float32, (3, k))), R.bits(got[1]))
    assert np.array_equal(R.bits(d_out.to_numpy(np.float32, plain.shape)), R.bits(plain))
    # (c) refusals, each with a message of its own
    d = vithip.Search(vithip.SEARCH_HEAD_INPUT, 3, 1, 3, None, d_i.ptr, d_s.ptr)
    msgs = set()

    def refused(rc):
        assert rc == VH_ERR_INVALID, (rc, L.vh_last_error(ctx.h))
        msgs.add(L.vh_last_error(ctx.h).decode())

    def with_field(field, value):
        return C.byref(vithip.Search(*(value if f == field else getattr(d, f) for f, _ in vithip.Search._fields_)))
    for field, value in (("source", 2), ("k", 0), ("normalise", 2), ("nq", 4), ("index", None), ("score", d_s.ptr + 4)):
        refused(L.vh_search_bank_device(ctx.h, with_field(field, value)))
    refused(L.vh_search_bank_device(ctx.h, C.byref(vithip.Search(vithip.SEARCH_ROWS, 3, 1, 3, None, d_i.ptr, d_s.ptr))))   # null rows
    for args in ((0, 16, vithip.ELEM_F32, 1), (10, 24, vithip.ELEM_F32, 1), (10, 16, vithip.ELEM_U8, 1), (10, 16, vithip.ELEM_F32, 2)):
        refused(L.vh_set_bank(ctx.h, bank.ctypes.data, *args))
    # (d) the CLIP-style path: the context's own logits as the caller's rows, against a bank of their width
    texts = rng.standard_normal((100, cfg["classes"])).astype(np.float32)
    ctx.set_bank(texts, normalise=False)
    d_t = dev(vithip.to16(texts, dtype))
    assert_exact(ctx.search(3, rows=plain), tuple(a.astype(t) for a, t in zip(run_tap(plain, d_t, 100, 3, dtype, 1), (np.int32, np.float64))), "rows")
    refused(L.vh_search_bank_device(ctx.h, C.byref(d)))   # the head input is not 48 wide
    ctx.set_bank(None)
    assert ctx.bank_dims() == (0, 0)
    refused(L.vh_search_bank_device(ctx.h, C.byref(d)))   # no bank
    assert len(msgs) == 13, msgs
    for buf in (d_bank, d_in, d_out, d_i, d_s, d_t):
        buf.free()
    ctx.close()


def test_search_before_the_first_forward():
    """VH_SEARCH_ROWS is legal before any forward; VH_SEARCH_HEAD_INPUT is refused."""
    ctx = vithip.VitContext(MICRO, dtype=BF16, max_batch=2, ln_eps=EPS, flags=vithip.FLAG_LN_FOLD_OFF)   # (no calibration forward at the load)
    ctx.load_weights(S.make_blob(MICRO, 5, EPS))
    q, b = placed("first", 40, 4)
    ctx.set_bank(b.astype(np.float32), normalise=False)
    assert_exact(ctx.search(32, rows=q, normalise=False), SR.topk(q @ b.T, 32), "rows before a forward")
    with pytest.raises(vithip.VhError, match="no forward has run"):
        ctx.search(5)
    ctx.close()
