"""Exactly predictable inputs for the one-wave-per-row kernels of kernels_rows.hip, their closed-form expectations, a numpy
emulation of every kernel in the kernel's own order (with named mutants), the float64 references with derived bounds, and the
checks that test_rows_exact.py (CPU, on the emulation) and test_gpu_rows_exact.py (GPU, on the taps) both run.  No GPU, no
oracle.

Exactness must not depend on summation order or FMA contraction, so every sum of the bit-exact designs is exactly representable
in fp32 (the CPU self-test runs the emulation, which adds in the kernels' chunk and butterfly order, against the closed forms).

  two-level rows   x[r, k] = m_r +- a_r, two of each sign in every float4 chunk (a seeded arrangement per chunk), m_r a small
                   integer (one row has |m| = 4096 with a = 1/4: the row a one-pass variance destroys), a_r = 2^e, e in -2..3.
                   mean = m, var = a^2, rstd = 1 / a: with eps = 2^-40 (absorbed by a^2 >= 2^-4) the stored (mean, rstd) are
                   (m, 1 / a) bit for bit and the guard ratio |m| / a is exact.
  coded affine     gamma in {1, 1.5, 2, 3}, beta in {-0.5, 0, 0.5, 1} per column, seeded: y = +-gamma[k] + beta[k] is exact in
                   e4m3, bf16, fp16 and fp32, and a chunk or column mix-up changes bits.
  constant rows    var = 0: rstd = 2^20 with eps = 2^-40 and y = beta exactly; a kernel that drops eps gives NaN.
  big-eps rows     a = 3/4, eps = 7/16: var + eps = 1, rstd = 1, gamma in {2, 4}: y = +-1.5 / +-3 (+ beta).  Pins that eps is
                   added to the variance.
  uniform affine   (pre-LayerNorm) gamma = g0 = 2^e, beta = b0: the normalised row is two-level again, so the second-stage
                   (ymean, yrstd) = (b0, 1 / g0) and the guard |b0| / g0 are bit-exact (constant rows: (b0, 2^20)).
  residue rows     x = h + rho, h exact in the 16-bit type and no power of two, rho a multiple of ulp(h) / 16 with |rho| <=
                   7/16 ulp(h): hi = h and the lo byte = to_lo8(rho) bit for bit; plus the underflow tie 2^-10 of the scaled
                   byte, the value just above it, and residues beyond the byte's saturation at 448 (|x| <= 16384).
  split planes     (layernorm_split) (a) hi = m, lo = +-rho, rho a power of two the scaled byte holds; (b) hi = m +- a, lo = 0;
                   (c) mixed planes against float64 under ln_bound().
  partials         (finalize_stats) integer per-block (sum, sumsq) that differ per block, sum = dim m, sumsq = dim (m^2 + a^2):
                   mean = m and var = a^2 exactly even in the one-pass form; the largest block of the maximal guarded row is a
                   perfect square.
  head             y integers in [-4, 4], W integers in [-3, 3], bias = c / 4: logits exact in fp32.
  fold             scale gamma w = 1 + 2^-9 / 1 + 3 2^-9 (bf16; 2^-12 for fp16) and the true ties 1 + 2^-8 / 1 + 3 2^-8 (2^-11):
                   the rounded sums are small dyadic numbers, c is bit-exact and differs from the unrounded sum by dim 2^-9.

Bounds that are not bit equality are derived next to their use (ln_bound, stats_bound, head_bound, check_f8); the worst
|d| / bound seen under each is kept in MARGINS and printed by report_margins().
"""
import types

import numpy as np

import vithip

BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
F32 = 3   # the fp32 result of layernorm_kernel: a code of this module, never passed to the library
NAME = {BF16: "bf16", FP16: "fp16", FP8: "e4m3", F32: "fp32"}
f32 = np.float32
U = 2.0 ** -24
EPS_TINY = 2.0 ** -40
INF_BITS, NAN_WORD = 0x7F800000, 0x7FC00000

DIMS = [4, 8, 60, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024, 1028, 1276, 1280, 1284, 1664, 2044, 2048]
ROWS = [1, 2, 3, 4, 5, 7, 203]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 600]
NBLK = [1, 2, 15, 16, 17, 31, 32, 33]
HEAD_BATCH, HEAD_CLASSES, HEAD_DIMS = [1, 15, 16, 17, 33], [4, 60, 64, 68, 1000], [16, 48, 192, 1280]
POSITIONS = ("first", "middle", "last")
CH_CLASSES = (1, 2, 3, 4, 5, 8)   # the one ladder of kernels_rows.hip: float4 chunks per lane

MUTANTS = ("one_pass", "drop_last_chunk", "ch_small", "gamma_by_lane", "no_eps", "eps_on_sigma", "lo_scale_other",
           "guard_incl_pad", "guard_miss_last", "guard_store", "garbage_blocks", "head_no_batch_clamp", "head_image_wrap",
           "head_drop_class_tail", "c_unrounded")

MARGINS = {}


def _rng(seed, *key):
    return np.random.default_rng([int(seed)] + [int(k) for k in key])


def ch_class(dim):
    return next(c for c in CH_CLASSES if dim <= 256 * c)


def pos_index(pos, n):
    return {"first": 0, "middle": n // 2, "last": n - 1}[pos]


# ---- stored forms ---------------------------------------------------------------------------------------------------------
BITS_DT = {BF16: np.uint16, FP16: np.uint16, FP8: np.uint8, F32: np.uint32}


def to_bits(a, dt):
    """fp32 -> the stored form of `dt` (round to nearest even; e4m3 saturates like pack4_e4m3)."""
    a = np.ascontiguousarray(a, dtype=f32)
    if dt == F32:
        return a.view(np.uint32).copy()
    if dt == FP8:
        return vithip.to_e4m3(a)
    with np.errstate(over="ignore"):
        return vithip.to16(a, dt)


def from_bits(b, dt):
    if dt == F32:
        return np.ascontiguousarray(b, dtype=np.uint32).view(f32)
    return vithip.from_e4m3(b) if dt == FP8 else vithip.from16(b, dt)


def canary(shape, dt):
    return np.full(shape, np.iinfo(BITS_DT[dt]).max, dtype=BITS_DT[dt])


def lo_of(x, hi_bits, dt, scale_dt=None):
    """The lo plane the kernels keep next to hi = T(x): one scaled e4m3 byte (16-bit T) or bf16 (T = e4m3) of the fp32 difference."""
    res = (np.asarray(x, dtype=f32) - from_bits(hi_bits, dt)).astype(f32)
    return vithip.to_bf16_bits(res) if dt == FP8 else vithip.to_lo8(res, dt if scale_dt is None else scale_dt)


def lo_dt(dt):
    return BF16 if dt == FP8 else FP8   # stored type of the lo plane (bits: uint16 / uint8)


def word_of(v):
    return int(np.asarray(v, dtype=f32).reshape(1).view(np.uint32)[0]) & 0x7FFFFFFF


# ---- assertions -----------------------------------------------------------------------------------------------------------
def assert_bits(got, want, what, dim=None):
    """Bit equality of stored results; a failure names row, column and dim of the first differing element."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        r, c = (idx + (0,))[:2]
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} / {bad.size} elements differ in bits; first at row {r} column {c} "
                             f"(dim = {dim if dim is not None else got.shape[-1]}): got 0x{int(got[idx]):x}, want 0x{int(want[idx]):x}")


def assert_close(got, ref, tol, what, dim=None, label=None):
    """|got - ref| <= tol per element and everything finite; names the worst element; records worst |d| / tol under `label`."""
    got, ref, tol = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = np.broadcast_to(tol, ref.shape)
    fin = np.isfinite(got)
    if not fin.all():
        idx = tuple(int(i) for i in np.argwhere(~fin)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~fin)} / {got.size} elements not finite (unwritten or NaN), first at row "
                             f"{(idx + (0,))[0]} column {(idx + (0,))[1]} (dim = {dim})")
    d = np.abs(got - ref)
    ratio = d / np.maximum(tol, 1e-300)
    if label is not None:
        MARGINS[label] = max(MARGINS.get(label, 0.0), float(ratio.max()))
    if (d > tol).any():
        idx = np.unravel_index(int(np.argmax(ratio)), d.shape)
        r, c = (tuple(int(i) for i in idx) + (0,))[:2]
        raise AssertionError(f"{what}: {np.count_nonzero(d > tol)} / {d.size} elements outside the bound; worst at row {r} column {c} "
                             f"(dim = {dim}): got {got[idx]!r}, ref {ref[idx]!r}, |d| {d[idx]:.3e} > {tol[idx]:.3e}")


def assert_word(got, want, what):
    assert int(got) == int(want), f"{what}: guard word 0x{int(got):08x}, want 0x{int(want):08x}"


def report_margins():
    for k in sorted(MARGINS):
        print(f"\nworst |d| / bound  {k:<34} {MARGINS[k]:.3e}", end="")
    print()


# ---- derived bounds -------------------------------------------------------------------------------------------------------
def _ln_terms(x64, eps):
    """First-order error terms of the two-pass statistics of fp32 rows x (float64 copies), n = dim, u = 2^-24.
      sum:   any order of n - 1 additions: |S^ - S| <= n u sum|x|;  mean^ = fl(S^ / n):  dm = u sum|x| + u |mean|
      d^ = fl(x - mean^): |d^ - d| <= dm + u |d|
      V^ = sum fl(d^ d^): |V^ - V| <= 2 dm sum|d| + n dm^2 + (n + 3) u V      (squares, n - 1 additions)
      var^ = fl(fl(V^ / n) + eps), rstd^ = fl(1 / fl(sqrt(var^))): three correctly rounded operations on top of V^ / n:
      rel(rstd) <= rel(V) / 2 + 3 u."""
    n = x64.shape[1]
    mean = x64.mean(1)
    d = x64 - mean[:, None]
    V = (d * d).sum(1)
    dm = U * np.abs(x64).sum(1) + U * np.abs(mean)
    relv = (2 * dm * np.abs(d).sum(1) + n * dm * dm + (n + 3) * U * V) / (V + n * eps)
    rstd = 1.0 / np.sqrt(V / n + eps)
    return mean, d, rstd, dm, relv / 2 + 3 * U


def stats_bound(x64, eps):
    """-> (mean, rstd) in float64 and their bounds (dm, rstd * rel), times 1.01 for the second-order terms."""
    mean, _, rstd, dm, rel = _ln_terms(x64, eps)
    return np.stack([mean, rstd], 1), 1.01 * np.stack([dm, rstd * rel], 1)


def ln_bound(x64, gamma, beta, eps):
    """float64 LayerNorm of fp32 rows and the per-element bound of the kernels' expression fl(fl(fl(d^ rstd^) g) + b): the error
    of d^ scaled by rstd |g|, the relative error of rstd^ and of the two products on |d rstd g|, one rounding of the result (an
    FMA only removes roundings); times 1.01 for the second-order terms."""
    mean, d, rstd, dm, rel = _ln_terms(x64, eps)
    g, b = np.asarray(gamma, dtype=np.float64)[None, :], np.asarray(beta, dtype=np.float64)[None, :]
    t = d * rstd[:, None] * g
    y = t + b
    tol = np.abs(g) * rstd[:, None] * (dm[:, None] + U * np.abs(d)) + np.abs(t) * (rel[:, None] + 2 * U) + U * np.abs(y)
    return y, 1.01 * tol


def head_bound(y, w, dim):
    """dim * 2^-24 * sum_k |y w|: dim fused multiply-adds, each rounding at most u times the running sum of magnitudes."""
    return dim * U * (np.abs(y.astype(np.float64)) @ np.abs(w.astype(np.float64)).T)


# ---- designs ---------------------------------------------------------------------------------------------------------------
_PAT = np.array([[1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1], [-1, 1, 1, -1], [-1, 1, -1, 1], [-1, -1, 1, 1]], dtype=f32)


def coded_affine(dim, seed, big_eps=False):
    r = _rng(seed, 11, dim)
    gamma = r.choice([2.0, 4.0] if big_eps else [1.0, 1.5, 2.0, 3.0], size=dim).astype(f32)
    beta = r.choice([-0.5, 0.0, 0.5, 1.0], size=dim).astype(f32)
    return gamma, beta


def two_level(rows, dim, seed, kind="tiny", maxpos="first", pad=False, uniform=None, const="some"):
    """The two-level / constant / big-eps rows with their closed forms.  maxpos: where the |m| = 4096, a = 1/4 row stands among
    the `rows` real rows.  pad: three more rows behind them (rows >= guard_rows): a two-level row with a larger |x| and ratio
    (m = -8192, a = 1/4), a row with one +Inf and a row with one NaN.  uniform = (g0, b0): the pre-LayerNorm's uniform affine.
    const: "some" (every fifth row), "none", "only_max" (the row at maxpos is the only constant one), "all_but_max", "all", or
    "pad_only" (no real row, but the first row behind them)."""
    r = _rng(seed, 1, rows, dim)
    n = rows + (1 if pad else 0)
    sign = _PAT[r.integers(0, 6, size=(n, dim // 4))].reshape(n, dim)
    big = kind == "bigeps"
    if big:
        m = r.choice([-5.0, 0.0, 2.0, 9.0], size=n)
        a = np.full(n, 0.75)
        eps = 7.0 / 16.0
    else:
        m = r.choice([-12.0, 0.0, 3.0, 1024.0, -7.0, 100.0], size=n)
        a = 2.0 ** r.integers(-2, 4, size=n)
        eps = EPS_TINY
        p = pos_index(maxpos, rows)
        m[p], a[p] = (4096.0 if seed % 2 else -4096.0), 0.25
        idx = np.arange(n)
        if const == "some":
            a[(idx % 5 == 2) & (idx != p)] = 0.0
        elif const == "only_max":
            a[p] = 0.0
        elif const == "all_but_max":
            a[idx != p] = 0.0
        elif const == "all":
            a[:] = 0.0
        if pad:
            m[rows], a[rows] = -8192.0, (0.0 if const == "pad_only" else 0.25)
    x = (m[:, None] + sign * a[:, None]).astype(f32)
    assert np.array_equal(x.astype(np.float64), m[:, None] + sign.astype(np.float64) * a[:, None])
    rstd = 1.0 / np.sqrt(a * a + eps)
    if not big:
        rstd = np.where(a > 0, 1.0 / np.where(a > 0, a, 1.0), 2.0 ** 20)
    if uniform is None:
        gamma, beta = coded_affine(dim, seed, big)
    else:
        gamma, beta = np.full(dim, uniform[0], dtype=f32), np.full(dim, uniform[1], dtype=f32)
    y = (sign * (a * rstd)[:, None] * gamma[None, :] + beta[None, :]).astype(f32)
    c = types.SimpleNamespace(rows=rows, dim=dim, eps=eps, gamma=gamma, beta=beta, sign=sign, m=m.astype(f32), a=a.astype(f32),
                              stats=np.stack([m, rstd], 1).astype(f32), y=y, ncheck=n, kind=kind)
    if pad:
        bad = np.repeat(x[:1], 2, axis=0).copy()
        bad[0, int(r.integers(0, dim))] = np.inf
        bad[1, int(r.integers(0, dim))] = np.nan
        x = np.concatenate([x, bad])
    c.x = x
    if uniform is not None:   # second-stage statistics of the normalised rows
        g0, b0 = float(uniform[0]), float(uniform[1])
        c.ystats = np.stack([np.full(n, b0), np.where(a > 0, 1.0 / g0, 2.0 ** 20)], 1).astype(f32)
        c.ratio = (abs(b0) * c.ystats[:, 1]).astype(f32)
    return c


def strided(x, stride):
    """Rows of x at a row stride > dim; what lies between the rows is large and must never be read."""
    rows, dim = x.shape
    full = np.full((rows, stride), 3.0e30, dtype=x.dtype) if x.dtype == f32 else np.full((rows, stride), 0x7B, dtype=x.dtype)
    full[:, :dim] = x
    return full.reshape(-1)[:(rows - 1) * stride + dim].copy()


def residue_rows(rows, dim, dt, seed):
    """x = h + rho for the 16-bit lo planes (module docstring), with the edge elements in the first row's first columns."""
    r = _rng(seed, 2, rows, dim, dt)
    mbits = 7 if dt == BF16 else 10
    e = r.integers(-3, 13, size=(rows, dim))
    frac = r.integers(1, 2 ** mbits, size=(rows, dim))                    # no power of two
    h = (1.0 + frac / 2.0 ** mbits) * 2.0 ** e * r.choice([-1.0, 1.0], size=(rows, dim))
    ulp = 2.0 ** (e - mbits)
    rho = r.integers(-7, 8, size=(rows, dim)) * ulp / 16.0
    x = h + rho
    scale = vithip.LO8_SCALE[dt]
    tie = 2.0 ** -10 / scale
    edges = [(1.5, tie), (1.5, -tie), (1.5, tie * 1.125), (-1.5, -tie * 1.125),                # underflow tie -> 0, just above -> 2^-9
             (6144.0, 480.0 / scale), (-6144.0, -480.0 / scale), (6144.0, 448.0 / scale)]    # beyond 448: saturates; 448 itself
    k = min(len(edges), dim)
    for j in range(k):
        x[0, j], h[0, j], rho[0, j] = edges[j][0] + edges[j][1], edges[j][0], edges[j][1]
    xf = x.astype(f32)
    assert np.array_equal(xf.astype(np.float64), x) and np.abs(x).max() <= 16384
    hi = to_bits(h, dt)
    assert np.array_equal(from_bits(hi, dt).astype(np.float64), h)
    lo = vithip.to_lo8(rho.astype(f32), dt)
    if k == len(edges):
        assert list(lo[0, :k]) == [0x00, 0x80, 0x01, 0x81, 0x7E, 0xFE, 0x7E], [hex(v) for v in lo[0, :k]]
    return types.SimpleNamespace(x=xf, hi=hi, lo=lo, rows=rows, dim=dim)


def split_planes(rows, dim, dt, form, seed):
    """Planes for layernorm_split.  form "a": hi = m, lo = +-rho; "b": hi = m +- a, lo = 0; "c": mixed (float64 under ln_bound)."""
    r = _rng(seed, 3, rows, dim, dt)
    gamma, beta = coded_affine(dim, seed)
    c = types.SimpleNamespace(rows=rows, dim=dim, gamma=gamma, beta=beta, eps=EPS_TINY, form=form, y=None)
    if form == "c":
        c.eps = 1e-6
        xr = (r.standard_normal((rows, dim)) * 1.5 + r.uniform(-2, 2, size=(rows, 1))).astype(f32)
        c.gamma = (1.0 + 0.2 * r.standard_normal(dim)).astype(f32)
        c.beta = (0.2 * r.standard_normal(dim)).astype(f32)
        c.hi = to_bits(xr, dt)
        c.lo = lo_of(xr, c.hi, dt)
        return c
    sign = np.where(np.argsort(r.random((rows, dim)), axis=1) % 2 == 0, 1.0, -1.0)   # dim / 2 of each sign, free pattern
    if form == "a":
        m = r.choice([-12.0, -3.0, 0.0, 2.0, 8.0], size=rows)
        a = 2.0 ** r.integers(-5, 1, size=rows)
        hi_v, lo_v = np.repeat(m[:, None], dim, 1), sign * a[:, None]
    else:
        m, a = np.array([(0.0, 1.0), (2.0, 1.0), (-3.0, 1.0), (8.0, 4.0), (1.0, 0.5), (0.0, 0.25)])[r.integers(0, 6, size=rows)].T
        hi_v, lo_v = m[:, None] + sign * a[:, None], np.zeros((rows, dim))
    c.hi = to_bits(hi_v, dt)
    c.lo = vithip.to_bf16_bits(lo_v.astype(f32)) if dt == FP8 else vithip.to_lo8(lo_v.astype(f32), dt)
    assert np.array_equal(from_bits(c.hi, dt), hi_v.astype(f32))
    assert np.array_equal(vithip.from_bf16_bits(c.lo) if dt == FP8 else vithip.from_lo8(c.lo, dt), lo_v.astype(f32))
    c.y = (sign * gamma[None, :] + beta[None, :]).astype(f32)
    return c


def partials_rows(nblk, rows, seed, maxpos="first", nan_row=False):
    """Integer per-block (sum, sumsq) [nblk][rows + 3][2] with dim = 64 nblk (module docstring); the three rows behind the real
    ones carry a larger ratio and block, +Inf and NaN.  nan_row: the real row at maxpos carries a NaN sum instead."""
    r = _rng(seed, 4, nblk, rows)
    dim, n = 64 * nblk, rows + 3
    m = r.integers(-12, 13, size=n).astype(np.float64)
    a = r.choice([0.5, 1.0, 2.0, 4.0], size=n)
    p = pos_index(maxpos, rows)
    m[p], a[p] = 60.0, (0.5 if nblk > 1 else 0.0)
    m[rows], a[rows] = 70.0, (0.5 if nblk > 1 else 0.0)     # (33 blocks: dim (m^2 + a^2) stays below 2^24)
    part = np.zeros((nblk, n, 2))
    for i in range(n):
        S1, S2 = dim * m[i], dim * (m[i] ** 2 + a[i] ** 2)
        s1, s2 = np.full(nblk, 64 * m[i]), np.full(nblk, S2 / nblk)
        if nblk > 1:
            dl = r.integers(-9, 10, size=nblk).astype(np.float64)
            dl[-1] -= dl.sum()
            s1 += dl
            avg = S2 / nblk
            q = np.ceil(np.sqrt(avg)) + 1
            k = float(min(5, avg // (4 * nblk)))
            j = r.integers(-int(k), int(k) + 1, size=nblk - 1).astype(np.float64) if k >= 1 else np.zeros(nblk - 1)
            if i in (p, rows):     # the largest block is a perfect square, the others share the rest
                base = np.floor((S2 - q * q) / (nblk - 1))
                oth = base + j
                oth[-1] += (S2 - q * q) - oth.sum()
                bi = int(r.integers(0, nblk))
                s2 = np.insert(oth, bi, q * q)
                assert oth.max() < q * q and oth.min() >= 0
            else:
                s2[:-1] += j
                s2[-1] -= j.sum()
        assert s1.sum() == S1 and s2.sum() == S2 and np.array_equal(s1, np.round(s1)) and np.array_equal(s2, np.round(s2))
        part[:, i, 0], part[:, i, 1] = s1, s2
    part[:, rows + 1] = part[:, 0]
    part[int(r.integers(0, nblk)), rows + 1] = (np.inf, np.inf)
    part[:, rows + 2] = part[:, 0]
    part[int(r.integers(0, nblk)), rows + 2] = (np.nan, np.nan)
    if nan_row:
        part[int(r.integers(0, nblk)), p, 0] = np.nan
    rstd = np.where(a > 0, 1.0 / np.where(a > 0, a, 1.0), 2.0 ** 20)
    stats = np.stack([m, rstd], 1).astype(f32)
    b2 = part[:, :rows, 1].max(0)
    return types.SimpleNamespace(part=part.astype(f32), nblk=nblk, rows=rows, dim=dim, stats=stats, ncheck=rows + 1,
                                 ratio=(np.abs(m) * rstd).astype(f32), bound=np.sqrt(b2.astype(f32)), p=p)


def head_case(batch, classes, dim, seed, random=False):
    r = _rng(seed, 5, batch, classes, dim)
    if random:
        y = r.standard_normal((batch, dim)).astype(f32)
        w = (0.05 * r.standard_normal((classes, dim))).astype(f32)
        bias = (0.1 * r.standard_normal(classes)).astype(f32)
    else:
        y = r.integers(-4, 5, size=(batch, dim)).astype(f32)
        w = r.integers(-3, 4, size=(classes, dim)).astype(f32)
        bias = (np.arange(classes) / 4.0).astype(f32)
    ref = y.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)[None, :]
    return types.SimpleNamespace(y=y, w=w, bias=bias, ref=ref, batch=batch, classes=classes, dim=dim)


def fold_case(rows, dim, dt, seed, ties=True):
    """ties: scale gamma w on the rounding edges of `dt` (beta = 0: d = scale b exactly); else integer w, beta and b."""
    r = _rng(seed, 6, rows, dim, dt)
    scale = 0.125
    gamma = 2.0 ** r.integers(-1, 3, size=dim)
    if ties:
        s = 2.0 ** (-9 if dt == BF16 else -12)
        # s = a quarter of the type's step at 1.  Positive entries lose s (1 + s -> 1) or 2 s (the tie 1 + 2 s -> 1, even), negative
        # ones lose s (-(1 + 3 s) -> -(1 + 4 s)) or 2 s (the tie -(1 + 6 s) -> -(1 + 8 s), even): every rounding error has the same
        # sign, so the sum of the unrounded values exceeds c by about dim s
        pos = np.array([1 + s, 1 + 2 * s, 0.5, 1.25])
        neg = -np.array([1 + 3 * s, 1 + 6 * s, 0.5, 1.25])
        pick = r.integers(0, 4, size=(rows, dim))
        t = np.where(r.random((rows, dim)) < 0.5, pos[pick], neg[pick])
        beta, b = np.zeros(dim), r.integers(-8, 9, size=rows).astype(np.float64)
    else:
        t = r.integers(-3, 4, size=(rows, dim)).astype(np.float64)
        beta, b = r.integers(-2, 3, size=dim).astype(np.float64), r.integers(-8, 9, size=rows).astype(np.float64)
        t = t * (scale * gamma)[None, :]           # (w is the integer itself)
    w = t / (scale * gamma)[None, :]
    c = types.SimpleNamespace(w=w.astype(f32), b=b.astype(f32), gamma=gamma.astype(f32), beta=beta.astype(f32), scale=scale, rows=rows,
                              dim=dim, ties=ties)
    assert np.array_equal(c.w.astype(np.float64), w)
    c.w16 = to_bits(t, dt)
    rounded = from_bits(c.w16, dt).astype(np.float64)
    c.c = rounded.sum(1).astype(f32)
    assert np.array_equal(c.c.astype(np.float64), rounded.sum(1))
    c.c_unrounded = t.sum(1)
    d = scale * ((w * beta[None, :]).sum(1) + b)
    c.d = d.astype(f32)
    assert np.array_equal(c.d.astype(np.float64), d)
    return c


def f8_rows(rows, dim, seed):
    """Rows for the e4m3 row quantiser: even rows `exact` (w = 2^e t, t an integer e4m3 holds, 448 among them: the decoded values
    are integers and their sum is exact in any order; the caller divides them by its gamma), odd rows random, the LAST row all
    zero (s0 = 1)."""
    r = _rng(seed, 7, rows, dim)
    w = (r.standard_normal((rows, dim)) * 0.05).astype(np.float64)
    exact = np.arange(rows) % 2 == 0
    t = r.choice([0.0, 1.0, -1.0, 2.0, -3.0, 4.0, 6.0, -8.0, 16.0, -28.0, 448.0], size=(rows, dim))
    t[:, 0] = 448.0
    e = 2.0 ** r.integers(-6, 3, size=(rows, 1))
    w = np.where(exact[:, None], t * e, w)
    w[rows - 1] = 0.0
    exact[rows - 1] = True
    return w.astype(f32), exact


# ---- numpy emulation of the kernels, in their order ----------------------------------------------------------------------
_LANES = np.arange(64)


def _butterfly(s, op=np.add):
    for o in (32, 16, 8, 4, 2, 1):
        s = op(s, s[..., _LANES ^ o]).astype(f32)
    return s[..., 0]


def _layout(x, dim, CH, mutant, classes):
    """[rows][dim] -> registers [rows][CH][64 lanes][4] (zeros beyond the row) and the mask of the chunks a lane owns."""
    rows = x.shape[0]
    nchunk = dim // 4 - (1 if mutant == "drop_last_chunk" else 0)
    limit = 64 * CH
    if mutant == "ch_small":
        i = classes.index(CH)
        limit = 64 * classes[i - 1] if i > 0 else limit
    v = np.zeros((rows, CH * 256), dtype=f32)
    v[:, :dim] = x
    chunk = (_LANES[None, :] + 64 * np.arange(CH)[:, None])          # [CH][64]
    ok = (chunk < nchunk) & (chunk < limit)
    v = np.where(ok[None, :, :, None], v.reshape(rows, CH, 64, 4), f32(0))
    return v, ok


def _unlayout(v, ok, dim, fill_bits):
    """registers [rows][CH][64][4] of stored bits -> [rows][dim]; chunks no lane owns keep the canary."""
    rows = v.shape[0]
    out = np.where(ok[None, :, :, None], v, fill_bits).reshape(rows, -1)[:, :dim]
    return np.ascontiguousarray(out)


def _two_pass(v, ok, dim, eps, mutant):
    rows, CH = v.shape[0], v.shape[1]
    with np.errstate(all="ignore"):
        s = np.zeros((rows, 64), dtype=f32)
        for i in range(CH):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        mean = _butterfly(s) / f32(dim)
        q = np.zeros((rows, 64), dtype=f32)
        for i in range(CH):
            for j in range(4):
                if mutant == "one_pass":
                    q = q + np.where(ok[i][None, :], v[:, i, :, j] * v[:, i, :, j], f32(0))
                else:
                    d = v[:, i, :, j] - mean[:, None]
                    q = q + np.where(ok[i][None, :], d * d, f32(0))
        var = _butterfly(q) / f32(dim)
        if mutant == "one_pass":
            var = np.maximum(var - mean * mean, f32(0))
        return mean.astype(f32), _rstd(var, eps, mutant)


def _rstd(var, eps, mutant):
    with np.errstate(all="ignore"):
        if mutant == "no_eps":
            return (f32(1) / np.sqrt(var.astype(f32))).astype(f32)
        if mutant == "eps_on_sigma":
            return (f32(1) / (np.sqrt(var.astype(f32)) + f32(eps))).astype(f32)
        return (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)


def _affine(v, ok, mean, rstd, gamma, beta, dim, CH, mutant):
    g = np.zeros(CH * 256, dtype=f32)
    b = np.zeros(CH * 256, dtype=f32)
    g[:dim], b[:dim] = gamma, beta
    g, b = g.reshape(CH, 64, 4), b.reshape(CH, 64, 4)
    if mutant == "gamma_by_lane":
        g, b = np.repeat(g[:1], CH, 0), np.repeat(b[:1], CH, 0)
    with np.errstate(all="ignore"):
        y = ((v - mean[:, None, None, None]) * rstd[:, None, None, None] * g[None] + b[None]).astype(f32)
    return np.where(ok[None, :, :, None], y, f32(0))


def _guard(word0, vals, nreal, mutant):
    vals = np.asarray(vals, dtype=f32)
    n = len(vals) if mutant == "guard_incl_pad" else nreal - (1 if mutant == "guard_miss_last" else 0)
    mx = int((vals[:n].view(np.uint32) & np.uint32(0x7FFFFFFF)).max()) if n > 0 else 0
    return mx if mutant == "guard_store" else max(int(word0), mx)


def _twice(presets, fn):
    """{preset: the guard word after each of two identical launches that started from it} (None: no word given)."""
    if presets is None:
        return None
    return {w0: [fn(w0), fn(fn(w0))] for w0 in presets}


PRESETS = (0, 0x3F000000, 0x7149F2CA, NAN_WORD)   # nothing yet, below every expected maximum (0.5), above it (1e30: kept), a NaN word (kept)


class Emulation:
    """The taps' interface on the numpy emulation; `mutant` names the one deviation it carries (None: the kernels as written)."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.mutant = mutant

    def layernorm(self, xflat, rows, dim, stride, gamma, beta, eps, dt):
        x = np.stack([xflat[r * stride:r * stride + dim] for r in range(rows)])
        CH = ch_class(dim)
        v, ok = _layout(x, dim, CH, self.mutant, CH_CLASSES)
        mean, rstd = _two_pass(v, ok, dim, eps, self.mutant)
        y = _affine(v, ok, mean, rstd, gamma, beta, dim, CH, self.mutant)
        return _unlayout(to_bits(y, dt), ok, dim, canary((), dt))

    def rowstats(self, x, eps, dt, split, guard_rows=0, amax0=None):
        rows, dim = x.shape
        CH = ch_class(dim)
        v, ok = _layout(x, dim, CH, self.mutant, CH_CLASSES)
        mean, rstd = _two_pass(v, ok, dim, eps, self.mutant)
        hi = to_bits(np.nan_to_num(v), dt)
        other = {BF16: FP16, FP16: BF16}.get(dt) if self.mutant == "lo_scale_other" else None
        lo = _unlayout(lo_of(np.nan_to_num(v), hi, dt, other), ok, dim, canary((), lo_dt(dt))) if split else None
        with np.errstate(all="ignore"):
            amax = np.fmax.reduce(np.abs(v).reshape(rows, -1), axis=1, initial=0.0).astype(f32)     # fmaxf drops a NaN operand
        return dict(hi=_unlayout(hi, ok, dim, canary((), dt)), lo=lo, stats=np.stack([mean, rstd], 1),
                    amax=_twice(amax0, lambda w: _guard(w, amax, guard_rows, self.mutant)))

    def pre_ln(self, x, gamma, beta, eps, dt, outs, guard_rows=0, guard0=None, amax0=None):
        rows, dim = x.shape
        CH = ch_class(dim)
        v, ok = _layout(x, dim, CH, self.mutant, CH_CLASSES)
        mean, rstd = _two_pass(v, ok, dim, eps, self.mutant)
        y = _affine(v, ok, mean, rstd, gamma, beta, dim, CH, self.mutant)
        res = dict(y32=None, hi=None, lo=None, stats=None, guard=None, amax=None)
        if "y32" in outs:
            res["y32"] = _unlayout(to_bits(y, F32), ok, dim, canary((), F32))
        if "hi" not in outs and "stats" not in outs:
            return res
        ymean, yrstd = _two_pass(y, ok, dim, eps, self.mutant)
        if "hi" in outs:
            hi = to_bits(np.nan_to_num(y), dt)
            res["hi"] = _unlayout(hi, ok, dim, canary((), dt))
            if "lo" in outs:
                other = {BF16: FP16, FP16: BF16}.get(dt) if self.mutant == "lo_scale_other" else None
                res["lo"] = _unlayout(lo_of(np.nan_to_num(y), hi, dt, other), ok, dim, canary((), lo_dt(dt)))
        if "stats" in outs:
            res["stats"] = np.stack([ymean, yrstd], 1)
        with np.errstate(all="ignore"):
            ratio = (np.abs(ymean) * yrstd).astype(f32)
            amax = np.fmax.reduce(np.abs(y).reshape(rows, -1), axis=1, initial=0.0).astype(f32)
        res["guard"] = _twice(guard0, lambda w: _guard(w, ratio, guard_rows, self.mutant))
        res["amax"] = _twice(amax0, lambda w: _guard(w, amax, guard_rows, self.mutant))
        return res

    def finalize(self, part, dim, eps, guard_rows=0, guard0=None, amax0=None):
        nblk, rows = part.shape[0], part.shape[1]
        s1, s2, b2 = np.zeros(rows, dtype=f32), np.zeros(rows, dtype=f32), np.zeros(rows, dtype=f32)
        with np.errstate(all="ignore"):
            for b in range(-(-nblk // 16) * 16):
                if b < nblk:
                    p = part[b]
                elif self.mutant == "garbage_blocks":
                    p = np.full((rows, 2), 7.0, dtype=f32)
                else:
                    p = np.zeros((rows, 2), dtype=f32)
                s1, s2 = s1 + p[:, 0], s2 + p[:, 1]
                b2 = np.where(np.isnan(p[:, 1]), b2, np.maximum(b2, p[:, 1]))   # fmaxf drops a NaN operand
            mean = s1 / f32(dim)
            var = s2 / f32(dim) - mean * mean
            var = np.where(np.isnan(var), f32(0), np.maximum(var, f32(0)))       # fmaxf(NaN, 0) = 0
            rstd = _rstd(var.astype(f32), eps, self.mutant)
            ratio, bound = (np.abs(mean) * rstd).astype(f32), np.sqrt(b2)
        return dict(stats=np.stack([mean, rstd], 1).astype(f32),
                    guard=_twice(guard0, lambda w: _guard(w, ratio, guard_rows, self.mutant)),
                    amax=_twice(amax0, lambda w: _guard(w, bound, guard_rows, self.mutant)))

    def ln_guard(self, stats, rows, guard0):
        with np.errstate(all="ignore"):
            ratio = (np.abs(stats[:, 0]) * stats[:, 1]).astype(f32)
        return _twice(guard0, lambda w: _guard(w, ratio, rows, self.mutant))

    def ln_split(self, hi, lo, rows, dim, stride, gamma, beta, eps, dt):
        hi = np.stack([hi[r * stride:r * stride + dim] for r in range(rows)])
        lo = np.stack([lo[r * stride:r * stride + dim] for r in range(rows)])
        sdt = {BF16: FP16, FP16: BF16}.get(dt, dt) if self.mutant == "lo_scale_other" else dt
        x = (from_bits(hi, dt) + (vithip.from_bf16_bits(lo) if dt == FP8 else vithip.from_lo8(lo, sdt))).astype(f32)
        n = dim - (1 if self.mutant == "drop_last_chunk" else 0)       # (this kernel walks single elements)
        T = -(-dim // 64)
        ok = (np.arange(T * 64) < n).reshape(T, 64)
        v = np.zeros((rows, T * 64), dtype=f32)
        v[:, :n] = x[:, :n]
        v = v.reshape(rows, T, 64)
        s, q = np.zeros((rows, 64), dtype=f32), np.zeros((rows, 64), dtype=f32)
        for t in range(T):
            s = s + v[:, t]
        mean = _butterfly(s) / f32(dim)
        for t in range(T):
            d = v[:, t] - mean[:, None]
            q = q + np.where(ok[t][None, :], (v[:, t] * v[:, t]) if self.mutant == "one_pass" else d * d, f32(0))
        var = _butterfly(q) / f32(dim)
        if self.mutant == "one_pass":
            var = np.maximum(var - mean * mean, f32(0))
        rstd = _rstd(var, eps, self.mutant)
        y = ((x - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :]).astype(f32)
        out = to_bits(y, F32)
        out[:, n:] = canary((), F32)
        return out

    def head(self, y, w, bias):
        batch, dim = y.shape
        classes = w.shape[0]
        nb = -(-batch // 16) * 16                    # a wave multiplies 16 image columns; those behind the batch run the clamped last image
        src = np.minimum(np.arange(nb), batch - 1)
        if self.mutant == "head_image_wrap":
            src = src % 16
        y64, w64 = y[src].astype(np.float64), w.astype(np.float64)
        if self.mutant == "head_no_batch_clamp":     # columns behind the batch hold whatever lies behind y
            y64[batch:] = np.nan
        acc = np.zeros((nb, classes), dtype=f32)
        with np.errstate(invalid="ignore"):
            for k in range(dim):
                acc = (acc.astype(np.float64) + y64[:, k:k + 1] * w64[None, :, k]).astype(f32)   # one rounding per fma
        out = to_bits(acc[:batch] + bias[None, :], F32)   # (only the images that exist are stored)
        if self.mutant == "head_drop_class_tail" and classes % 64:
            out[:, classes - classes % 64:] = canary((), F32)
        return out

    def _lane_sum(self, a, fma=None):
        rows, dim = a.shape
        T = -(-dim // 64)
        v = np.zeros((rows, T * 64), dtype=np.float64)
        v[:, :dim] = a
        v = v.reshape(rows, T, 64)
        s = np.zeros((rows, 64), dtype=f32)
        for t in range(T):
            s = (s.astype(np.float64) + v[:, t]).astype(f32)
        return _butterfly(s)

    def fold(self, w, b, gamma, beta, scale, dt):
        t = ((f32(scale) * gamma)[None, :] * w).astype(f32)
        w16 = to_bits(t, dt)
        cs = self._lane_sum(t if self.mutant == "c_unrounded" else from_bits(w16, dt))
        ds = self._lane_sum(beta.astype(np.float64)[None, :] * w.astype(np.float64))
        return dict(w16=w16, c=cs, d=(f32(scale) * (ds + b)).astype(f32))

    @staticmethod
    def _quant(t):
        amax = np.abs(t).max(1)
        s0 = np.where(amax > 0, (amax * f32(1.0 / 448.0)).astype(f32), f32(1)).astype(f32)
        q = vithip.to_e4m3((t / s0[:, None]).astype(f32))
        return q, s0

    def fold_f8(self, w, b, gamma, beta, scale):
        rows, dim = w.shape
        t = ((f32(scale) * gamma)[None, :] * w).astype(f32)
        q, s0 = self._quant(t)
        dec = vithip.from_e4m3(q).reshape(rows, dim // 4, 4)
        ch = ((dec[:, :, 0] + dec[:, :, 1]) + (dec[:, :, 2] + dec[:, :, 3])).astype(f32)     # a lane's float4, then lane + 64 i
        if self.mutant == "c_unrounded":
            ch = (t / s0[:, None]).astype(f32).reshape(rows, dim // 4, 4).sum(2).astype(f32)
        cs = self._lane_sum(ch)
        ds = self._lane_sum(beta.astype(np.float64)[None, :] * w.astype(np.float64))
        return dict(w8=q, wscale=s0, c=(s0 * cs).astype(f32), d=(f32(scale) * (ds + b)).astype(f32))

    def fake_quant(self, w):
        q, s0 = self._quant(w)
        return (vithip.from_e4m3(q) * s0[:, None]).astype(f32)


# ---- the checks: what both test files assert, on any backend with the interface of Emulation ---------------------------------
def check_layernorm(be, rows, dim, dt, kind="tiny", stride=None, seed=0):
    c = two_level(rows, dim, seed + dim, kind)
    st = stride or dim
    out = be.layernorm(strided(c.x, st), rows, dim, st, c.gamma, c.beta, c.eps, dt)
    assert_bits(out, to_bits(c.y, dt), f"layernorm {NAME[dt]} {kind} rows {rows} stride {st}", dim)


def check_rowstats(be, rows, dim, dt, split, maxpos="first", seed=0):
    """Two-level rows through the cast / split kernels: planes from the host helpers, (mean, rstd) = (m, 1 / a) bit for bit,
    and (e4m3) the |x| guard over the real rows only, from every preset of PRESETS, read after each of two launches."""
    c = two_level(rows, dim, seed + dim, "tiny", maxpos=maxpos, pad=True)
    what = f"rowstats_{'split' if split else 'cast'} {NAME[dt]} rows {rows}+3 max {maxpos}"
    want_amax = word_of(np.abs(c.x[:rows]).max())
    res = be.rowstats(c.x, c.eps, dt, split, rows, PRESETS if dt == FP8 else None)
    n = c.ncheck
    hi = to_bits(c.x[:n], dt)
    assert_bits(res["hi"][:n], hi, what + " hi", dim)
    if split:
        assert_bits(res["lo"][:n], lo_of(c.x[:n], hi, dt), what + " lo", dim)
    else:
        assert res["lo"] is None
    assert_bits(to_bits(res["stats"][:n], F32), to_bits(c.stats, F32), what + " (mean, rstd)", dim)
    for preset, words in (res["amax"] or {}).items():
        for i, w in enumerate(words):
            assert_word(w, max(preset, want_amax), f"{what} |x| guard preset 0x{preset:08x} launch {i + 1}")


def check_rowstats_residue(be, rows, dim, dt, seed=0):
    """Residue rows: hi = h and lo = to_lo8(rho) bit for bit (underflow tie, saturation); statistics against float64."""
    c = residue_rows(rows, dim, dt, seed + dim)
    res = be.rowstats(c.x, 1e-6, dt, True)
    what = f"rowstats_split residue {NAME[dt]} rows {rows}"
    assert_bits(res["hi"], c.hi, what + " hi", dim)
    assert_bits(res["lo"], c.lo, what + " lo", dim)
    ref, tol = stats_bound(c.x.astype(np.float64), 1e-6)
    assert_close(res["stats"], ref, tol, what + " (mean, rstd)", dim, "rowstats residue stats")


def check_pre_ln_uniform(be, rows, dim, dt, design, maxpos="first", seed=0, presets=None):
    """Uniform affine: every output bit-exact, second-stage statistics included, and both guards.  design "ratio": the row at
    maxpos is the only constant one (ratio |b0| 2^20, the others |b0| / g0); "amax": it is the only two-level one (|y| = g0 +
    |b0|, the others |b0|); "ratio_pad" / "amax_pad": no real row is constant / two-level, but the first row behind guard_rows
    is and would win.  Behind it: a row with +Inf and a row with NaN."""
    g0, b0 = (2.0, -3.0) if seed % 2 == 0 else (0.5, 1.0)
    c = two_level(rows, dim, seed + dim, "tiny", maxpos=maxpos, pad=True, uniform=(g0, b0),
                  const={"ratio": "only_max", "amax": "all_but_max", "ratio_pad": "pad_only", "amax_pad": "all"}[design])
    n = c.ncheck
    want_ratio = word_of(c.ratio[:rows].max())
    want_amax = word_of(np.abs(c.y[:rows]).max())
    what = f"pre_layernorm uniform {NAME[dt]} rows {rows}+3 {design} max {maxpos}"
    ps = PRESETS if presets is None else tuple(PRESETS[i] for i in presets)
    res = be.pre_ln(c.x, c.gamma, c.beta, c.eps, dt, ("y32", "hi", "lo", "stats"), rows, ps, ps if dt == FP8 else None)
    assert_bits(res["y32"][:n], to_bits(c.y, F32), what + " y32", dim)
    hi = to_bits(c.y, dt)
    assert_bits(res["hi"][:n], hi, what + " hi", dim)
    assert_bits(res["lo"][:n], lo_of(c.y, hi, dt), what + " lo", dim)
    assert_bits(to_bits(res["stats"][:n], F32), to_bits(c.ystats, F32), what + " (ymean, yrstd)", dim)
    for name, want in (("guard", want_ratio), ("amax", want_amax)):
        for preset, words in (res[name] or {}).items():
            for i, w in enumerate(words):
                assert_word(w, max(preset, want), f"{what} {name} word preset 0x{preset:08x} launch {i + 1}")


def check_pre_ln_nan_row(be, rows, dim, dt, maxpos, seed=0):
    """A REAL row with a NaN raises the ratio word above +Inf's bits."""
    c = two_level(rows, dim, seed + dim, "tiny", maxpos=maxpos, uniform=(2.0, -3.0), const="none")
    x = c.x.copy()
    x[pos_index(maxpos, rows), dim // 2] = np.nan
    res = be.pre_ln(x, c.gamma, c.beta, c.eps, dt, ("hi", "stats"), rows, (0,), None)
    for i, w in enumerate(res["guard"][0]):
        assert w > INF_BITS, f"pre_layernorm {NAME[dt]} rows {rows} dim {dim}: NaN row at {maxpos}, ratio word 0x{w:08x} after launch {i + 1}"


def check_pre_ln_coded(be, rows, dim, dt, outs, kind="tiny", seed=0):
    """Coded affine: y32 / hi / lo bit-exact; the second-stage statistics against float64 of the exact y (stats_bound) -- the GPU
    file adds bit equality with the row-statistics kernel run on y32.  `outs`: the outputs asked for (the others are NULL)."""
    c = two_level(rows, dim, seed + dim, kind)
    res = be.pre_ln(c.x, c.gamma, c.beta, c.eps, dt, outs)
    what = f"pre_layernorm coded {NAME[dt]} {kind} rows {rows} outs {'+'.join(outs)}"
    hi = to_bits(c.y, dt)
    for name, want in (("y32", to_bits(c.y, F32)), ("hi", hi), ("lo", lo_of(c.y, hi, dt))):
        if name in outs:
            assert_bits(res[name], want, f"{what} {name}", dim)
        else:
            assert res[name] is None
    if "stats" in outs:
        ref, tol = stats_bound(c.y.astype(np.float64), c.eps)
        assert_close(res["stats"], ref, tol, what + " (ymean, yrstd)", dim, "pre_layernorm coded stats")
    return c, res


def check_finalize(be, nblk, rows, maxpos="first", seed=0):
    c = partials_rows(nblk, rows, seed + nblk, maxpos)
    want_ratio, want_amax = word_of(c.ratio[:rows].max()), word_of(c.bound.max())
    assert word_of(c.ratio[rows]) > want_ratio and c.part[:, rows, 1].max() > c.part[:, :rows, 1].max()
    what = f"finalize_stats nblk {nblk} rows {rows}+3 max {maxpos}"
    res = be.finalize(c.part, c.dim, EPS_TINY, rows, PRESETS, PRESETS)
    assert_bits(to_bits(res["stats"][:c.ncheck], F32), to_bits(c.stats[:c.ncheck], F32), what + " (mean, rstd)", c.dim)
    for preset in PRESETS:
        for i in range(2):
            assert_word(res["guard"][preset][i], max(preset, want_ratio), f"{what} ratio guard preset 0x{preset:08x} launch {i + 1}")
            assert_word(res["amax"][preset][i], max(preset, want_amax), f"{what} block guard preset 0x{preset:08x} launch {i + 1}")
    res = be.finalize(c.part, c.dim, EPS_TINY)      # no guard words at all
    assert res["guard"] is None and res["amax"] is None
    assert_bits(to_bits(res["stats"][:c.ncheck], F32), to_bits(c.stats[:c.ncheck], F32), what + " (mean, rstd), no guards", c.dim)
    cn = partials_rows(nblk, rows, seed + nblk, maxpos, nan_row=True)
    for i, w in enumerate(be.finalize(cn.part, cn.dim, EPS_TINY, rows, (0,), None)["guard"][0]):
        assert w > INF_BITS, f"{what}: NaN row, ratio word 0x{w:08x} after launch {i + 1}"


def check_ln_guard(be, rows, maxpos="first", seed=0):
    r = _rng(seed, 8, rows)
    n = rows + 5
    stats = np.stack([r.integers(-50, 51, size=n), 2.0 ** r.integers(-3, 4, size=n)], 1).astype(f32)
    stats[pos_index(maxpos, rows)] = (-99.0, 16.0)
    stats[rows:] = [(1.0e6, 64.0), (np.inf, 1.0), (np.nan, 1.0), (-1.0e6, 64.0), (3.0, np.inf)]   # behind the rows: never read
    what = f"ln_guard rows {rows} max {maxpos}"
    for preset, words in be.ln_guard(stats, rows, PRESETS).items():
        for i, w in enumerate(words):
            assert_word(w, max(preset, word_of(99.0 * 16.0)), f"{what} preset 0x{preset:08x} launch {i + 1}")
    stats[pos_index(maxpos, rows), 0] = np.nan
    for i, w in enumerate(be.ln_guard(stats, rows, (0,))[0]):
        assert w > INF_BITS, f"{what}: NaN row, word 0x{w:08x} after launch {i + 1}"


def check_ln_split(be, rows, dim, dt, form, stride=None, seed=0):
    c = split_planes(rows, dim, dt, form, seed + dim)
    st = stride or dim
    out = be.ln_split(strided(c.hi, st), strided(c.lo, st), rows, dim, st, c.gamma, c.beta, c.eps, dt)
    what = f"layernorm_split {NAME[dt]} form {form} rows {rows} stride {st}"
    if form == "c":
        x = (from_bits(c.hi, dt) + (vithip.from_bf16_bits(c.lo) if dt == FP8 else vithip.from_lo8(c.lo, dt))).astype(f32)   # ONE fp32 add
        ref, tol = ln_bound(x.astype(np.float64), c.gamma, c.beta, c.eps)
        assert_close(from_bits(out, F32), ref, tol, what, dim, "layernorm_split mixed")
    else:
        assert_bits(out, to_bits(c.y, F32), what, dim)


def check_head(be, batch, classes, dim, seed=0):
    c = head_case(batch, classes, dim, seed)
    out = be.head(c.y, c.w, c.bias)
    assert_bits(out, to_bits(c.ref.astype(f32), F32), f"head_f32 batch {batch} classes {classes}", dim)


def check_head_random(be, batch, classes, dim, seed=0):
    c = head_case(batch, classes, dim, seed, random=True)
    out = from_bits(be.head(c.y, c.w, c.bias), F32)
    assert_close(out, c.ref, head_bound(c.y, c.w, dim), f"head_f32 random batch {batch} classes {classes}", dim, "head_f32 random")


def check_fold(be, rows, dim, dt, ties, seed=0):
    c = fold_case(rows, dim, dt, seed + dim, ties)
    res = be.fold(c.w, c.b, c.gamma, c.beta, c.scale, dt)
    what = f"fold_ln {NAME[dt]} {'ties' if ties else 'integers'} rows {rows}"
    assert_bits(res["w16"], c.w16, what + " w16", dim)
    assert_bits(to_bits(res["c"], F32)[:, None], to_bits(c.c, F32)[:, None], what + " c (the sum of the ROUNDED weights)", dim)
    assert_bits(to_bits(res["d"], F32)[:, None], to_bits(c.d, F32)[:, None], what + " d", dim)
    return c


def check_f8(be, rows, dim, seed=0):
    """fold_ln_f8 and fake_quant_rows against the numpy emulation of the same expressions: bytes, scales and dequantised values bit
    for bit; c bit for bit on the rows whose decoded sum is exact, else within dim 2^-24 s0 sum|decode| (any order of dim - 1
    additions, each rounding at most u times the running sum of magnitudes); d within (dim + 2) 2^-24 |scale| (sum|beta w| + |b|)."""
    w, exact = f8_rows(rows, dim, seed + dim)
    r = _rng(seed, 9, rows, dim)
    gamma = (2.0 ** r.integers(-1, 2, size=dim)).astype(f32)
    beta, b = r.integers(-2, 3, size=dim).astype(f32), r.integers(-8, 9, size=rows).astype(f32)
    scale = 0.125
    w = np.where(exact[:, None], w / gamma[None, :], w).astype(f32)     # exact rows: scale gamma w = scale 2^e t in every column
    emu = Emulation().fold_f8(w, b, gamma, beta, scale)
    dec = vithip.from_e4m3(emu["w8"]).astype(np.float64)
    assert all(np.array_equal(dec[i], np.round(dec[i])) and np.abs(dec[i]).sum() < 2 ** 24 for i in np.nonzero(exact)[0])
    assert emu["wscale"][rows - 1] == 1.0 and not emu["w8"][rows - 1].any()
    res = be.fold_f8(w, b, gamma, beta, scale)
    what = f"fold_ln_f8 rows {rows}"
    assert_bits(res["w8"], emu["w8"], what + " bytes", dim)
    assert_bits(to_bits(res["wscale"], F32)[:, None], to_bits(emu["wscale"], F32)[:, None], what + " wscale", dim)
    s0 = emu["wscale"].astype(np.float64)
    c_exact = (s0 * dec.sum(1)).astype(f32)
    assert_bits(to_bits(res["c"][exact], F32)[:, None], to_bits(c_exact[exact], F32)[:, None], what + " c, exact rows", dim)
    assert_close(res["c"][:, None], (s0 * dec.sum(1))[:, None], (dim * U * s0 * np.abs(dec).sum(1) + 1e-300)[:, None], what + " c", dim,
                 "fold_ln_f8 c")
    bw = np.abs(beta.astype(np.float64)[None, :] * w).sum(1) + np.abs(b)
    d_ref = scale * ((beta.astype(np.float64)[None, :] * w).sum(1) + b)
    assert_close(res["d"][:, None], d_ref[:, None], ((dim + 2) * U * scale * bw + 1e-300)[:, None], what + " d", dim, "fold_ln_f8 d")
    t = ((f32(scale) * gamma)[None, :] * w).astype(f32)
    assert_bits(to_bits(be.fake_quant(t), F32), to_bits(Emulation().fake_quant(t), F32), f"fake_quant_rows rows {rows}", dim)


# ---- the sweeps: every shape of the GPU file, run by the CPU self-test on the emulation as well ------------------------------
ALL_DT, PLANE_DT = (BF16, FP16, FP8, F32), (BF16, FP16, FP8)


def sweep_layernorm(be, dim, rows_list=ROWS):
    for i, rows in enumerate(rows_list):
        for dt in ALL_DT:
            check_layernorm(be, rows, dim, dt)
            check_layernorm(be, rows, dim, dt, "bigeps")
            if rows in (5, 203) or dt == ALL_DT[i % 4]:
                check_layernorm(be, rows, dim, dt, stride=dim + 4 * (1 + i % 3))


def sweep_rowstats(be, dim, rows_list=ROWS):
    for i, rows in enumerate(rows_list):
        for dt in PLANE_DT:
            for split in (False, True):
                for pos in (POSITIONS if rows == 203 else (POSITIONS[(i + split) % 3],)):
                    check_rowstats(be, rows, dim, dt, split, pos)
            if dt != FP8:
                check_rowstats_residue(be, rows, dim, dt)


def sweep_pre_ln(be, dim, rows_list=ROWS):
    """-> the (case, result) pairs of the coded launches that asked for y32 and stats (the GPU file re-derives the statistics
    from y32 with the row-statistics kernel)."""
    coded = []
    for i, rows in enumerate(rows_list):
        for dt in PLANE_DT:
            for design in ("ratio", "ratio_pad") + (("amax", "amax_pad") if dt == FP8 else ()):
                for pos in (POSITIONS if rows == 203 and design in ("ratio", "amax") else (POSITIONS[i % 3],)):
                    check_pre_ln_uniform(be, rows, dim, dt, design, pos, seed=i, presets=None if rows in (4, 203) else (i % 4,))
            check_pre_ln_nan_row(be, rows, dim, dt, POSITIONS[i % 3])
            coded.append((dt,) + check_pre_ln_coded(be, rows, dim, dt, ("y32", "hi", "lo", "stats")))
            check_pre_ln_coded(be, rows, dim, dt, ("y32",), "bigeps")
            check_pre_ln_coded(be, rows, dim, dt, (("hi", "stats"), ("hi", "lo"), ("y32", "stats"), ("hi",))[i % 4], ("tiny", "bigeps")[i % 2])
    return coded


def sweep_ln_split(be, dim, rows_list=ROWS):
    for i, rows in enumerate(rows_list):
        for dt in PLANE_DT:
            for form in "abc":
                check_ln_split(be, rows, dim, dt, form)
                if rows in (5, 203) or form == "abc"[i % 3]:
                    check_ln_split(be, rows, dim, dt, form, stride=dim + 8 * (1 + i % 3))


def sweep_finalize(be, nblk, counts=COUNTS):
    for i, rows in enumerate(counts):
        for pos in (POSITIONS if rows in (257, 600) else (POSITIONS[i % 3],)):
            check_finalize(be, nblk, rows, pos)


def sweep_ln_guard(be, counts=COUNTS):
    for rows in counts:
        for pos in POSITIONS:
            check_ln_guard(be, rows, pos)


def sweep_head(be, dim):
    for batch in HEAD_BATCH:
        for classes in HEAD_CLASSES:
            check_head(be, batch, classes, dim)
            if batch in (17, 33):
                check_head_random(be, batch, classes, dim)
    if dim <= 192:     # the row counts of the other per-thread kernels, at one narrow and one ragged class count
        for i, batch in enumerate(COUNTS):
            check_head(be, batch, (4, 68)[i % 2], dim)


def sweep_fold(be, dim):
    for rows in (1, 5, 70):
        for dt in (BF16, FP16):
            check_fold(be, rows, dim, dt, True)
            check_fold(be, rows, dim, dt, False)
        check_f8(be, rows, dim)


class Recorder:
    """Wraps a backend and keeps every array / word it returns, as bits: two runs can then be compared for IDENTITY."""

    def __init__(self, be):
        self.be, self.log = be, []

    def _keep(self, v):
        if isinstance(v, dict):
            for k in sorted(v):
                self._keep(v[k])
        elif isinstance(v, np.ndarray):
            self.log.append(np.ascontiguousarray(v).view(np.uint8).copy())
        elif v is not None:
            self.log.append(np.asarray(v, dtype=np.uint64).view(np.uint8).copy())

    def __getattr__(self, name):
        fn = getattr(self.be, name)

        def call(*a, **k):
            res = fn(*a, **k)
            self._keep(res)
            return res
        return call

    def same_as(self, other):
        return len(self.log) == len(other.log) and all(np.array_equal(a, b) for a, b in zip(self.log, other.log))


# ---- refusals: every row tap, VH_ERR_INVALID before anything is launched --------------------------------------------------
def refusal_calls(pin, pout):
    """-> [(label, thunk returning the tap's status)] for every row tap: each thunk is a valid call (4 rows, dim 64; pointers pin
    for inputs, pout for outputs) with ONE argument spoiled.  Nothing is launched, so the pointers are never followed."""
    L = vithip.lib()
    e = 1e-6
    taps = {   # name: (function, valid arguments, {label: (index, value)})
        "layernorm": (L.vh_op_layernorm, [pin, 4, 64, 64, pin, pin, e, pout, BF16, None],
                      {"dtype 100": (8, 100), "dtype 7": (8, 7), "dtype -1": (8, -1), "row_stride % 4": (3, 66)}),
        "layernorm_f32": (L.vh_op_layernorm_f32, [pin, 4, 64, 64, pin, pin, e, pout, None], {"row_stride < dim": (3, 60)}),
        "layernorm_split": (L.vh_op_layernorm_split, [pin, pin, 4, 64, 64, pin, pin, e, pout, BF16, None],
                            {"dtype 100": (9, 100), "dtype 7": (9, 7), "row_stride < dim": (4, 60)}),
        "rowstats_cast": (L.vh_op_rowstats_cast, [pin, 4, 64, e, pout, pout, BF16, None], {"dtype 100": (6, 100), "dtype 7": (6, 7)}),
        "rowstats_split": (L.vh_op_rowstats_split, [pin, 4, 64, e, pout, pout, pout, BF16, None], {"dtype 100": (7, 100), "dtype 7": (7, 7)}),
        "rowstats_guard": (L.vh_op_rowstats_guard, [pin, 4, 64, e, pout, pout, pout, FP8, 4, pout, None],
                           {"dtype 100": (7, 100), "dtype 7": (7, 7), "guard_rows > rows": (8, 5), "guard_rows < 0": (8, -1),
                            "amax_guard with a 16-bit dtype": (7, BF16), "null lo is the cast form, not a refusal": None, "null amax is allowed": None}),
        "pre_layernorm": (L.vh_op_pre_layernorm, [pin, 4, 64, pin, pin, e, pout, pout, pout, pout, BF16, None],
                          {"dtype 100": (10, 100), "dtype 7": (10, 7), "eps 0": (5, 0.0), "lo without hi": (7, None),
                           "null y32/lo/stats are allowed": None}),
        "pre_layernorm_guard": (L.vh_op_pre_layernorm_guard, [pin, 4, 64, pin, pin, e, pout, pout, pout, pout, FP8, 4, pout, pout, None],
                                {"dtype 100": (10, 100), "eps 0": (5, 0.0), "lo without hi": (7, None), "guard_rows > rows": (11, 5),
                                 "amax_guard with a 16-bit dtype": (10, FP16), "null y32/lo/stats/guards are allowed": None}),
        "finalize_stats": (L.vh_op_finalize_stats, [pin, 2, 4, 128, e, pout, None], {"nblk 0": (1, 0), "dim 0": (3, 0)}),
        "finalize_stats_guard": (L.vh_op_finalize_stats_guard, [pin, 2, 4, 128, e, pout, 4, pout, pout, None],
                                 {"nblk 0": (1, 0), "dim 0": (3, 0), "guard_rows > rows": (6, 5), "guard_rows < 0": (6, -1),
                                  "null guards are allowed": None}),
        "ln_guard": (L.vh_op_ln_guard, [pin, 4, pout, None], {}),
        "head_f32": (L.vh_op_head_f32, [pin, pin, pin, pout, 4, 8, 64, None], {"batch 0": (4, 0), "classes % 4": (5, 6), "classes 0": (5, 0),
                                                                             "dim % 16": (6, 24), "dim 0": (6, 0)}),
        "fold_ln": (L.vh_op_fold_ln, [pin, pin, pin, pin, 4, 64, 1.0, pout, pout, pout, BF16, None],
                    {"dtype 100": (10, 100), "dtype 7": (10, 7), "dtype e4m3 (its own tap)": (10, FP8), "dim 0": (5, 0)}),
        "fold_ln_f8": (L.vh_op_fold_ln_f8, [pin, pin, pin, pin, 4, 64, 1.0, pout, pout, pout, pout, None], {"dim % 4": (5, 62), "dim 0": (5, 0)}),
        "fake_quant_rows": (L.vh_op_fake_quant_rows, [pin, 4, 64, pout, None], {"cols % 4": (2, 62), "cols 0": (2, 0)}),
    }
    nullable = {"rowstats_guard": (5, 9), "pre_layernorm": (6, 7, 8, 9), "pre_layernorm_guard": (6, 7, 8, 9, 12, 13),
                "finalize_stats_guard": (7, 8)}
    rows_at = {"finalize_stats": 2, "finalize_stats_guard": 2, "ln_guard": 1, "head_f32": None, "fold_ln": 4, "fold_ln_f8": 4,
               "fake_quant_rows": 1, "layernorm_split": 2}
    dim_at = {"layernorm": 2, "layernorm_f32": 2, "layernorm_split": 3, "rowstats_cast": 2, "rowstats_split": 2, "rowstats_guard": 2,
              "pre_layernorm": 2, "pre_layernorm_guard": 2}
    calls = []
    for name, (fn, good, spoil) in taps.items():
        muts = {k: v for k, v in spoil.items() if v is not None}
        for i, a in enumerate(good[:-1]):
            if a in (pin, pout) and isinstance(a, int) and i not in nullable.get(name, ()):
                muts[f"null pointer (argument {i})"] = (i, None)
        r = rows_at.get(name, 1)
        if r is not None:
            muts["rows 0"] = (r, 0)
        if name in dim_at:
            muts["dim % 4"] = (dim_at[name], 62)
            muts["dim > 2048"] = (dim_at[name], 2052)
            muts["dim 0"] = (dim_at[name], 0)
        if name in ("pre_layernorm", "pre_layernorm_guard"):
            both = list(good)
            both[6] = both[7] = both[8] = None
            calls.append((f"{name}: neither y32 nor hi", lambda fn=fn, a=both: fn(*a)))
        for label, (i, v) in muts.items():
            a = list(good)
            a[i] = v
            if label == "dim > 2048" and name in ("layernorm", "layernorm_f32", "layernorm_split"):
                a[i + 1] = 2052    # (the row stride follows the dim: it is the dim that is refused)
            calls.append((f"{name}: {label}", lambda fn=fn, a=a: fn(*a)))
    return calls
