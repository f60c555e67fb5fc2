"""GPU, per element: the one-wave-per-row kernels of kernels_rows.hip on exactly predictable rows (tests/rows_exact.py).

The operator tests of test_gpu_ops / test_gpu_clip / test_gpu_fp8 run these kernels on smooth random rows at a few dims and
hold them to relative bounds; the guards, the fp32 head, layernorm_split, fold_ln_f8 and fake_quant_rows were reachable only
through whole forwards.  Here every dim stands on a class boundary of the register kernels (or next to one), the row counts
cover the four-waves-per-workgroup tail, and the inputs are built so that (mean, rstd), the planes, the guard words and the
logits are known BIT FOR BIT whatever the summation order; what is not bit equality is held to a bound derived in
rows_exact.py.  test_rows_exact.py proves on the CPU that these assertions fail for a one-pass variance, a dropped chunk, a
class one too small, gamma indexed by lane, a misplaced eps, the other type's lo scale, a guard that counts padding rows, misses
the last real row or stores instead of taking the maximum, garbage in place of missing blocks, a mishandled 17th image, a
dropped class tail and c summed from unrounded weights.  The sweeps are rows_exact's: the CPU self-test runs the same ones.

Every output buffer is exactly sized, pre-filled with 0xFF (an unwritten element differs in bits from anything expected) and
carries a guard of at least one row in front of and behind it that must stay 0xFF; outputs passed as NULL own no memory, so the
guards around the others vouch for them.  Guard words start from every preset of rows_exact.PRESETS and are read after each of
two launches.
"""
import numpy as np
import pytest

import rows_exact as X
from vh_testlib import _KEEP, dev

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
BF16, FP16, FP8, F32 = X.BF16, X.FP16, X.FP8, X.F32
ESZ = {BF16: 2, FP16: 2, FP8: 1, F32: 4}


def release():
    for b in _KEEP:
        b.free()
    _KEEP.clear()


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    X.report_margins()


class Out:
    """An exactly sized output of `rows` rows of `rowbytes` bytes, 0xFF everywhere, between two guards of at least one row."""

    def __init__(self, rows, rowbytes, what):
        self.g = max(256, -(-rowbytes // 16) * 16)
        self.n, self.what = rows * rowbytes, what
        self.buf = dev(np.full(2 * self.g + self.n, 0xFF, dtype=np.uint8))
        self.ptr = self.buf.ptr + self.g

    def read(self, dtype, shape):
        raw = self.buf.to_numpy(np.uint8, (2 * self.g + self.n,))
        assert np.all(raw[:self.g] == 0xFF) and np.all(raw[self.g + self.n:] == 0xFF), f"{self.what}: a guard around the output was written"
        return raw[self.g:self.g + self.n].view(dtype).reshape(shape).copy()


class Word(Out):
    """A guard word on the device, canaries around it."""

    def __init__(self, what):
        super().__init__(1, 4, what)

    def set(self, value):
        host = np.full(2 * self.g + 4, 0xFF, dtype=np.uint8)
        host[self.g:self.g + 4] = np.array([value], dtype=np.uint32).view(np.uint8)
        vithip._check(vithip.lib().vh_memcpy_h2d(0, self.buf.ptr, host.ctypes.data, host.nbytes))

    def get(self):
        return int(self.read(np.uint32, (1,))[0])


def with_presets(presets, words, launch):
    """For every preset: set the words, launch twice, read the words after each.  -> [{preset: [w1, w2]} per word] (None: no word)."""
    res = [{} if w is not None else None for w in words]
    for p in (presets if presets is not None else (None,)):
        for w in words:
            if w is not None:
                w.set(p)
        for w, r in zip(words, res):
            if w is not None:
                r[p] = []
        for _ in range(2 if p is not None else 1):
            launch()
            for w, r in zip(words, res):
                if w is not None:
                    r[p].append(w.get())
    return res


class Gpu:
    """rows_exact's backend interface on the taps."""

    def layernorm(self, xflat, rows, dim, stride, gamma, beta, eps, dt):
        out = Out(rows, dim * ESZ[dt], "layernorm")
        if dt == F32:
            vithip.op_layernorm_f32(dev(xflat).ptr, rows, dim, stride, dev(gamma).ptr, dev(beta).ptr, eps, out.ptr)
        else:
            vithip.op_layernorm(dev(xflat).ptr, rows, dim, stride, dev(gamma).ptr, dev(beta).ptr, eps, out.ptr, dt)
        return out.read(X.BITS_DT[dt], (rows, dim))

    def rowstats(self, x, eps, dt, split, guard_rows=0, amax0=None):
        rows, dim = x.shape
        xd = dev(x)
        hi, st = Out(rows, dim * ESZ[dt], "rowstats hi"), Out(rows, 8, "rowstats stats")
        lo = Out(rows, dim * ESZ[X.lo_dt(dt)], "rowstats lo") if split else None
        word = Word("rowstats |x| word") if amax0 is not None else None

        def launch():
            if word is not None:
                vithip.op_rowstats_guard(xd.ptr, rows, dim, eps, hi.ptr, lo.ptr if split else None, st.ptr, dt, guard_rows, word.ptr)
            elif split:
                vithip.op_rowstats_split(xd.ptr, rows, dim, eps, hi.ptr, lo.ptr, st.ptr, dt)
            else:
                vithip.op_rowstats_cast(xd.ptr, rows, dim, eps, hi.ptr, st.ptr, dt)
        amax, = with_presets(amax0, [word], launch)
        return dict(hi=hi.read(X.BITS_DT[dt], (rows, dim)), lo=lo.read(X.BITS_DT[X.lo_dt(dt)], (rows, dim)) if split else None,
                    stats=st.read(np.float32, (rows, 2)), amax=amax)

    def pre_ln(self, x, gamma, beta, eps, dt, outs, guard_rows=0, guard0=None, amax0=None, in_place=False):
        rows, dim = x.shape
        y32 = Out(rows, dim * 4, "pre_layernorm y32") if "y32" in outs else None
        if in_place:      # x aliases y32: the rows start inside the output buffer
            vithip._check(vithip.lib().vh_memcpy_h2d(0, y32.ptr, np.ascontiguousarray(x).ctypes.data, x.nbytes))
            xptr = y32.ptr
        else:
            xptr = dev(x).ptr
        hi = Out(rows, dim * ESZ[dt], "pre_layernorm hi") if "hi" in outs else None
        lo = Out(rows, dim * ESZ[X.lo_dt(dt)], "pre_layernorm lo") if "lo" in outs else None
        st = Out(rows, 8, "pre_layernorm stats") if "stats" in outs else None
        gw = Word("pre_layernorm ratio word") if guard0 is not None else None
        aw = Word("pre_layernorm |y| word") if amax0 is not None else None
        g, b = dev(gamma), dev(beta)
        p = lambda o: o.ptr if o is not None else None

        def launch():
            if gw is None and aw is None:
                vithip.op_pre_layernorm(xptr, rows, dim, g.ptr, b.ptr, eps, p(y32), p(hi), p(lo), p(st), dt)
            else:
                vithip.op_pre_layernorm_guard(xptr, rows, dim, g.ptr, b.ptr, eps, p(y32), p(hi), p(lo), p(st), dt, guard_rows, p(gw), p(aw))
        guard, amax = with_presets(guard0 if guard0 is not None else amax0, [gw, aw], launch)
        return dict(y32=y32.read(np.uint32, (rows, dim)) if y32 else None, hi=hi.read(X.BITS_DT[dt], (rows, dim)) if hi else None,
                    lo=lo.read(X.BITS_DT[X.lo_dt(dt)], (rows, dim)) if lo else None,
                    stats=st.read(np.float32, (rows, 2)) if st else None, guard=guard, amax=amax)

    def finalize(self, part, dim, eps, guard_rows=0, guard0=None, amax0=None):
        nblk, rows = part.shape[0], part.shape[1]
        pd, st = dev(part), Out(rows, 8, "finalize_stats stats")
        gw = Word("finalize_stats ratio word") if guard0 is not None else None
        aw = Word("finalize_stats block word") if amax0 is not None else None

        def launch():
            if gw is None and aw is None:
                vithip.op_finalize_stats(pd.ptr, nblk, rows, dim, eps, st.ptr)
            else:
                vithip.op_finalize_stats_guard(pd.ptr, nblk, rows, dim, eps, st.ptr, guard_rows, gw.ptr if gw else None, aw.ptr if aw else None)
        guard, amax = with_presets(guard0 if guard0 is not None else amax0, [gw, aw], launch)
        return dict(stats=st.read(np.float32, (rows, 2)), guard=guard, amax=amax)

    def ln_guard(self, stats, rows, guard0):
        sd, w = dev(stats), Word("ln_guard word")
        return with_presets(guard0, [w], lambda: vithip.op_ln_guard(sd.ptr, rows, w.ptr))[0]

    def ln_split(self, hi, lo, rows, dim, stride, gamma, beta, eps, dt):
        out = Out(rows, dim * 4, "layernorm_split")
        vithip.op_layernorm_split(dev(hi).ptr, dev(lo).ptr, rows, dim, stride, dev(gamma).ptr, dev(beta).ptr, eps, out.ptr, dt)
        return out.read(np.uint32, (rows, dim))

    def head(self, y, w, bias):
        batch, dim = y.shape
        classes = w.shape[0]
        out = Out(batch, classes * 4, "head_f32")
        vithip.op_head_f32(dev(y).ptr, dev(w).ptr, dev(bias).ptr, out.ptr, batch, classes, dim)
        return out.read(np.uint32, (batch, classes))

    def fold(self, w, b, gamma, beta, scale, dt):
        rows, dim = w.shape
        w16, c, d = Out(rows, dim * 2, "fold_ln w16"), Out(rows, 4, "fold_ln c"), Out(rows, 4, "fold_ln d")
        vithip.op_fold_ln(dev(w).ptr, dev(b).ptr, dev(gamma).ptr, dev(beta).ptr, rows, dim, scale, w16.ptr, c.ptr, d.ptr, dt)
        return dict(w16=w16.read(np.uint16, (rows, dim)), c=c.read(np.float32, (rows,)), d=d.read(np.float32, (rows,)))

    def fold_f8(self, w, b, gamma, beta, scale):
        rows, dim = w.shape
        w8, ws, c, d = Out(rows, dim, "fold_ln_f8 w8"), Out(rows, 4, "fold_ln_f8 wscale"), Out(rows, 4, "fold_ln_f8 c"), Out(rows, 4, "fold_ln_f8 d")
        vithip.op_fold_ln_f8(dev(w).ptr, dev(b).ptr, dev(gamma).ptr, dev(beta).ptr, rows, dim, scale, w8.ptr, ws.ptr, c.ptr, d.ptr)
        return dict(w8=w8.read(np.uint8, (rows, dim)), wscale=ws.read(np.float32, (rows,)), c=c.read(np.float32, (rows,)),
                    d=d.read(np.float32, (rows,)))

    def fake_quant(self, w):
        rows, cols = w.shape
        out = Out(rows, cols * 4, "fake_quant_rows")
        vithip.op_fake_quant_rows(dev(w).ptr, rows, cols, out.ptr)
        return out.read(np.float32, (rows, cols))


class Releasing:
    """The backend, freeing the device buffers of a call once its results are on the host (a sweep makes thousands of calls)."""

    def __init__(self):
        self.be = Gpu()

    def __getattr__(self, name):
        fn = getattr(self.be, name)

        def call(*a, **k):
            try:
                return fn(*a, **k)
            finally:
                release()
        return call


GPU = Releasing()


@pytest.mark.parametrize("dim", X.DIMS)
def test_layernorm(dim):
    X.sweep_layernorm(GPU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_rowstats_cast_and_split(dim):
    X.sweep_rowstats(GPU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_pre_layernorm(dim):
    for dt, c, res in X.sweep_pre_ln(GPU, dim):
        # layer 0's statistics are the bits the row-statistics kernel gives on y32 (one pass instead of two)
        again = GPU.rowstats(X.from_bits(res["y32"], F32), c.eps, dt, True)
        X.assert_bits(X.to_bits(res["stats"], F32), X.to_bits(again["stats"], F32), f"pre_layernorm {X.NAME[dt]} stats = rowstats(y32)", dim)
        X.assert_bits(res["hi"], again["hi"], f"pre_layernorm {X.NAME[dt]} hi = rowstats(y32) hi", dim)
        X.assert_bits(res["lo"], again["lo"], f"pre_layernorm {X.NAME[dt]} lo = rowstats(y32) lo", dim)


@pytest.mark.parametrize("dt", X.PLANE_DT, ids=lambda d: X.NAME[d])
def test_pre_layernorm_in_place(dt):
    """x may alias y32: a lane reads its chunks before it writes them."""
    for rows, dim in ((5, 260), (203, 1284), (7, 2048)):
        c = X.two_level(rows, dim, dim)
        res = GPU.pre_ln(c.x, c.gamma, c.beta, c.eps, dt, ("y32", "hi", "lo", "stats"), in_place=True)
        X.assert_bits(res["y32"], X.to_bits(c.y, F32), f"pre_layernorm in place {X.NAME[dt]} rows {rows} y32", dim)
        X.assert_bits(res["hi"], X.to_bits(c.y, dt), f"pre_layernorm in place {X.NAME[dt]} rows {rows} hi", dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_layernorm_split(dim):
    X.sweep_ln_split(GPU, dim)


@pytest.mark.parametrize("nblk", X.NBLK)
def test_finalize_stats(nblk):
    X.sweep_finalize(GPU, nblk)


def test_ln_guard():
    X.sweep_ln_guard(GPU)


@pytest.mark.parametrize("dim", X.HEAD_DIMS)
def test_head_f32(dim):
    X.sweep_head(GPU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_fold_ln_and_row_quantiser(dim):
    X.sweep_fold(GPU, dim)


def test_refusals_leave_every_canary_whole():
    """Every row tap, new and old: dim % 4, dim > 2048, rows = 0, null pointers, undocumented dtypes (100 on vh_op_layernorm
    included), head classes % 4 and dim % 16 -> VH_ERR_INVALID, nothing launched, nothing written."""
    n = 1 << 16
    pin, pout = dev(np.zeros(n, dtype=np.uint8)), dev(np.full(n, 0xFF, dtype=np.uint8))
    calls = X.refusal_calls(pin.ptr, pout.ptr)
    assert len(calls) > 120
    for label, call in calls:
        assert call() == 1, label
    assert np.all(pout.to_numpy(np.uint8, (n,)) == 0xFF), "a refused call wrote to an output"
    assert not pin.to_numpy(np.uint8, (n,)).any(), "a refused call wrote to an input"
