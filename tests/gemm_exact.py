"""Exactly predictable GEMM inputs, their reference, a numpy emulation of the epilogues and layouts, and the per-element
assertions of test_gemm_exact.py (CPU) and test_gpu_gemm_exact.py (GPU).  No GPU, no oracle.

Operands.  A is sparse: in every K-tile (64 columns; 128 for e4m3 operands) a row holds one or two non-zeros from {+-1, +-2} at
seeded columns that differ from row to row.  W is dense, integers in [-3, 3].  Every product and every partial sum is a small
integer, so the accumulator is the same exact integer in any summation order, and a dropped or repeated K-tile, a wrong row,
a wrong column or a wrong k pairing changes it.  e4m3 operands carry a per-channel weight scale from {1, 1/2} (exact).

Epilogue inputs are chosen so that every claimed-exact result is exact: integer bias / c / d / position embedding / residual,
mean[m] integers in [-3, 3] that vary inside a 16-row block, rstd[m] from {1/2, 1, 2}; every 16-bit result has at most 8
significant bits (exact in bf16 and fp16).  The split residual's incoming planes hold an integer plus a fixed fraction, 1/32
(bf16) or 1/256 (fp16): below the hi plane's rounding step from |x| = 8 on, and exactly 1.0 after the lo plane's scale, so the
expected planes are unambiguous and hi + lo reproduces x exactly.  The only inexact quantities are the activations (bounded
as tests/test_gpu_clip.py bounds them: half a unit in the last place plus max(the erf fit's documented error, a quarter unit)) and
the split residual's sum of squares (bounded by the fp32 noise of its 64 additions of positive terms, 64 * 2^-24 relative).

Activations: erf GELU, QuickGELU and tanh GELU (float64 references and tables keyed per activation).  The bound separates every pair
with 16-bit results.  With e4m3 results it does NOT separate the erf from the tanh form on the designs' grid (act_separated: no grid
point fails; QuickGELU fails at 30 against either): the e4m3 forms check the layout, the pre-activation and the rounding of those two
codes, not which of the two functions ran.  test_gemm_exact.py asserts exactly this set of pairs.

The patch forms take `lead` rows in front of an image's patch rows (Case(lead=...), Case.with_lead): GEMM row img * np + p lands on
output row img * (np + lead) + lead + p and adds position row 1 + p whatever the lead; lead rows, and the partial sums of lead rows
and padding rows, keep their canaries.  lead_rows_expected is the reference of the kernel that writes those lead rows afterwards.

Buffers are kept in their LOGICAL form here -- out [R][N], out16 [R][N], partials [N / 64][R][2], R = M (the patch forms: token
rows) -- and the layouts (tiled, head-major) are conversions of `out`.
"""
import copy
import math

import numpy as np

import vithip

BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16", FP8: "e4m3"}
E = {n[4:]: getattr(vithip, n) for n in dir(vithip) if n.startswith("EPI_")}   # "BIAS" -> vithip.EPI_BIAS, ...
ENAME = {v: k for k, v in E.items()}
ACT = (E["BIAS_GELU"], E["LNFOLD_GELU"], E["BIAS_QGELU"], E["LNFOLD_QGELU"], E["BIAS_TGELU"], E["LNFOLD_TGELU"])
QACT = (E["BIAS_QGELU"], E["LNFOLD_QGELU"])
TACT = (E["BIAS_TGELU"], E["LNFOLD_TGELU"])
FOLD = (E["LNFOLD"], E["LNFOLD_GELU"], E["LNFOLD_QGELU"], E["LNFOLD_TGELU"])
SPLIT = (E["RESID_SPLIT"], E["PATCH_SPLIT"])
PATCHES = (E["PATCH"], E["PATCH_SPLIT"])
NEED_N256 = (E["RESID_LN"], E["RESID_SPLIT"], E["PATCH_SPLIT"])
EPI_16BIT_OPERANDS = sorted(E.values())
EPI_E4M3_OPERANDS = [E[k] for k in ("BIAS", "BIAS_GELU", "BIAS_QGELU", "BIAS_TGELU", "BIAS_RESID", "BIAS_F32", "LNFOLD", "LNFOLD_GELU",
                                    "LNFOLD_QGELU", "LNFOLD_TGELU", "RESID_LN", "RESID_SPLIT")]
# tests/test_gpu_clip.py (the activation sweeps): the erf fit's documented absolute error per result type, mantissa bits, smallest
# normal exponent
ERF_ABS = {FP16: 7.7e-6, BF16: 3.4e-5, FP8: 5.7e-4}
MANT = {FP16: 10, BF16: 7, FP8: 3}
MIN_EXP = {FP16: -14, BF16: -126, FP8: -6}
SQ_REL = 64 * 2.0 ** -24          # sum of squares of 64 positive terms in fp32, any order: derived, not measured
CANARY16, CANARY8 = 0x7B7B, 0x7B
CANARY32 = np.array([0x7B7B7B7B], dtype=np.uint32).view(np.float32)[0]
CANARY_P = np.float32(-7.0)
TILE = 256
LO_FRAC = {BF16: 1.0 / 32.0, FP16: 1.0 / 256.0, FP8: 0.0}


def ktile(f8):
    return 128 if f8 else 64


def patches_per_image(M):
    """Patch count of the patch-embedding forms: below the 128-row wave tile where M allows (image boundaries inside it)."""
    for d in (100, 64, 50, 32, 16):
        if M % d == 0:
            return d
    raise ValueError(M)


class Case:
    """Operands and epilogue inputs of one shape.  a [M][K], w [N][K] fp32 integers; ws [N] the weight scale (ones for 16-bit
    operands); acc = ws * (a w^T), exact; contrib(j) = K-tile j's share of it.

    The patch forms: np_img patches per image (patches_per_image(M) unless given), `lead` rows in front of an image's patch rows
    (class token + register tokens; 0 = none), so GEMM row img * np_img + p lands on output row img * (np_img + lead) + lead + p.
    The position row it adds is 1 + p of a table of np_img + 1 rows WHATEVER the lead: that is what the launch is handed (a context
    without a class token passes its [np_img][N] table one row early).  pad_rows: rows of `partials` beyond the last token row."""

    def __init__(self, M, N, K, f8, seed=0, lead=1, np_img=None, pad_rows=0):
        kw = ktile(f8)
        assert K % kw == 0 and lead >= 0 and pad_rows >= 0
        self.M, self.N, self.K, self.f8, self.nk = M, N, K, f8, K // kw
        self.lead, self.pad_rows = lead, pad_rows
        r = np.random.default_rng([seed, M, N, K, int(f8)])
        a = np.zeros((M, K), dtype=np.float32)
        rows = np.arange(M)
        for kt in range(self.nk):
            c1 = r.integers(0, kw, size=M)
            c2 = (c1 + r.integers(1, kw, size=M)) % kw
            v = r.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), size=(M, 2))
            second = r.random(M) < 0.5
            a[rows, kt * kw + c1] = v[:, 0]
            a[rows[second], kt * kw + c2[second]] = v[second, 1]
        self.a = a
        self.w = r.integers(-3, 4, size=(N, K)).astype(np.float32)
        n, m = np.arange(N), np.arange(M)
        self.ws = np.where(n % 3 == 1, 0.5, 1.0).astype(np.float32) if f8 else np.ones(N, dtype=np.float32)
        self.bias = ((n * 7) % 33 - 16).astype(np.float32)            # also d_n of the LN-fold forms
        self.c = ((n * 3) % 9 - 4).astype(np.float32)
        self.mean = ((m * 5) % 7 - 3).astype(np.float32)
        self.rstd = np.array([0.5, 1.0, 2.0], dtype=np.float32)[(m + m // 3) % 3]
        self.stats = np.ascontiguousarray(np.stack([self.mean, self.rstd], axis=1))
        self.acc = (a @ self.w.T) * self.ws[None, :]                 # fp32 sgemm of small integers: exact
        self._seed, self._x0 = seed, None
        try:
            self.np_img = np_img or patches_per_image(M)
        except ValueError:
            self.np_img = 0
        if self.np_img:
            assert M % self.np_img == 0
            self.pos = r.integers(-50, 51, size=(self.np_img + 1, N)).astype(np.float32)
        for arr in (self.a, self.w, self.acc):
            arr.setflags(write=False)

    @property
    def x0(self):
        """The integer residual the RESID_* epilogues update, [M][N] in [-100, 100] (generated on first use)."""
        if self._x0 is None:
            r = np.random.default_rng([self._seed, self.M, self.N, 77])
            self._x0 = r.integers(-100, 101, size=(self.M, self.N)).astype(np.float32)
            self._x0.setflags(write=False)
        return self._x0

    @property
    def tiles_m(self):
        return (self.M + TILE - 1) // TILE

    @property
    def tiles_n(self):
        return (self.N + TILE - 1) // TILE

    @property
    def ntiles(self):
        return self.tiles_m * self.tiles_n

    def contrib(self, j):
        kw = ktile(self.f8)
        return (self.a[:, j * kw:(j + 1) * kw] @ self.w[:, j * kw:(j + 1) * kw].T) * self.ws[None, :]

    def operand_bits(self, dt):
        """A and W as the kernel takes them (uint16, or e4m3 bytes)."""
        if self.f8:
            return to_e4m3(self.a), to_e4m3(self.w)
        return vithip.to16(self.a, dt), vithip.to16(self.w, dt)

    # ---- the patch forms' row map --------------------------------------------------------------------------------------
    def with_lead(self, lead, pad_rows=0):
        """The same operands (shared, not copied) with another count of lead rows."""
        c = copy.copy(self)
        c.lead, c.pad_rows = lead, pad_rows
        return c

    @property
    def tokens(self):
        return self.np_img + self.lead

    def out_rows(self, epi):
        return self.M // self.np_img * self.tokens if epi in PATCHES else self.M

    def partial_rows(self, epi):
        """Row stride of `partials` (PATCH_SPLIT: the launch's prow)."""
        return self.out_rows(epi) + (self.pad_rows if epi == E["PATCH_SPLIT"] else 0)

    def row_map(self, epi):
        m = np.arange(self.M)
        return m + (m // self.np_img + 1) * self.lead if epi in PATCHES else m

    def pos_rows(self):
        """The position row of every GEMM row: 1 + p, not the output row's index inside its image (the two agree at lead 1 only)."""
        return 1 + np.arange(self.M) % self.np_img

    def tile_mask(self, tiles):
        """[M][N] bool: the elements of the launched tiles (None = all), tile t = (t / tiles_n, t % tiles_n)."""
        if tiles is None:
            return np.ones((self.M, self.N), dtype=bool)
        hit = np.zeros(self.ntiles, dtype=bool)
        hit[np.asarray(list(tiles), dtype=np.int64)] = True
        t = (np.arange(self.M)[:, None] // TILE) * self.tiles_n + np.arange(self.N)[None, :] // TILE
        return hit[t]


def out_kind(epi, dt, f8):
    """Element types of (out, out16): 'f32', dt (16-bit), FP8 (bytes) or None."""
    if epi in (E["BIAS_RESID"], E["BIAS_F32"], E["PATCH"]):
        return "f32", None
    if epi == E["RESID_LN"]:
        return "f32", (FP8 if f8 else dt)
    if epi in SPLIT:
        return (FP8, BF16) if f8 else (dt, "lo8")
    if epi in ACT:
        return (FP8 if f8 else dt), None
    return (BF16 if f8 else dt), None          # BIAS, LNFOLD


def np_dtype(kind):
    return np.float32 if kind == "f32" else (np.uint8 if kind in (FP8, "lo8") else np.uint16)


def canary(kind):
    return CANARY32 if kind == "f32" else (CANARY8 if kind in (FP8, "lo8") else CANARY16)


def to_e4m3(x):
    """vithip.to_e4m3 (round to nearest even, saturating at +-448) by integer arithmetic on the fp32 bits: the many-tile shape
    converts 4e7 elements.  test_gemm_exact.py checks the two against each other."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sign = (x.view(np.uint32) >> np.uint32(24)) & np.uint32(0x80)
    a = np.minimum(np.abs(x), np.float32(448.0))
    u = a.view(np.uint32)
    r = ((u + np.uint32(0x7FFFF) + ((u >> np.uint32(20)) & np.uint32(1))) >> np.uint32(20)).astype(np.int32)   # exponent | 3 mantissa bits, RNE
    code = r - ((127 - 7) << 3)
    sub = np.rint(a * np.float32(512.0)).astype(np.int32)        # below 2^-6: multiples of 2^-9 (8 of them reach the first normal code)
    code = np.where(a < np.float32(2.0 ** -6), sub, code)
    return (code.astype(np.uint32) | sign).astype(np.uint8)


def to_lo8(residue, dt):
    return to_e4m3(np.asarray(residue, dtype=np.float32) * np.float32(vithip.LO8_SCALE[dt]))


def encode(v, kind):
    if kind == "f32":
        return np.asarray(v, dtype=np.float32)
    return to_e4m3(v) if kind == FP8 else vithip.to16(np.asarray(v, dtype=np.float32), kind)


def decode(b, kind):
    if kind == "f32":
        return np.asarray(b, dtype=np.float32)
    return vithip.from_e4m3(b) if kind == FP8 else vithip.from16(b, kind)


def split_planes(x, dt, f8):
    """x -> (hi, lo) as RESID_SPLIT stores them: 16-bit hi + scaled e4m3 byte, or (e4m3 operands) e4m3 hi + bf16 lo."""
    x = np.asarray(x, dtype=np.float32)
    if f8:
        hi = to_e4m3(x)
        return hi, vithip.to16(x - vithip.from_e4m3(hi), BF16)
    hi = vithip.to16(x, dt)
    return hi, to_lo8(x - vithip.from16(hi, dt), dt)


def join_planes(hi, lo, dt, f8):
    if f8:
        return vithip.from_e4m3(hi) + vithip.from16(lo, BF16)
    return vithip.from16(hi, dt) + vithip.from_lo8(lo, dt)


def initial(case, epi, dt):
    """The buffers before the launch: canaries, or the residual the epilogue updates.  {'out', 'out16', 'partials'} (those it has)."""
    ko, k16 = out_kind(epi, dt, case.f8)
    R, N = case.out_rows(epi), case.N
    b = {}
    if epi in (E["BIAS_RESID"], E["RESID_LN"]):
        b["out"] = case.x0.copy()
    elif epi == E["RESID_SPLIT"]:
        b["out"], b["out16"] = split_planes(case.x0 + np.float32(LO_FRAC[FP8 if case.f8 else dt]), dt, case.f8)
    else:
        b["out"] = np.full((R, N), canary(ko), dtype=np_dtype(ko))
    if k16 is not None and "out16" not in b:
        b["out16"] = np.full((R, N), canary(k16), dtype=np_dtype(k16))
    if epi in NEED_N256:
        b["partials"] = np.full((N // 64, case.partial_rows(epi), 2), CANARY_P, dtype=np.float32)
    return b


def pre_value(case, epi, dt, before, ft=np.float64):
    """The value the epilogue rounds, stores or feeds to the activation, [M][N], in `ft` arithmetic (exact in fp32 by design, so
    float32 and float64 agree: test_gemm_exact.py checks that)."""
    acc = case.acc.astype(ft)
    if epi in FOLD:
        return case.rstd.astype(ft)[:, None] * (acc - case.mean.astype(ft)[:, None] * case.c.astype(ft)[None, :]) + case.bias.astype(ft)[None, :]
    v = acc + case.bias.astype(ft)[None, :]
    if epi in (E["BIAS_RESID"], E["RESID_LN"]):
        v += before["out"].astype(ft)
    elif epi == E["RESID_SPLIT"]:
        v += join_planes(before["out"], before["out16"], dt, case.f8).astype(ft)
    elif epi in PATCHES:
        v += case.pos.astype(ft)[case.pos_rows()]
        if epi == E["PATCH_SPLIT"]:
            v += ft(LO_FRAC[dt])          # (the fraction that keeps lo busy rides on the position embedding)
    return v


def pos_table(case, epi, dt):
    """The position embedding the launch is given (PATCH_SPLIT: with the lo plane's fraction added)."""
    return case.pos + np.float32(LO_FRAC[dt]) if epi == E["PATCH_SPLIT"] else case.pos


_ERF_GRID = 8                      # the pre-activations are multiples of 1/4 at most: a table over multiples of 1/8 in [-1024, 1024]
_GELU_TABLE = None


def gelu64(v):
    """0.5 v (1 + erf(v / sqrt 2)) in float64 (math.erf through a table when v lies on the designs' grid)."""
    global _GELU_TABLE
    v = np.asarray(v, dtype=np.float64)
    k = v * _ERF_GRID
    if v.size and np.abs(v).max() <= 1024 and np.array_equal(k, np.rint(k)):
        if _GELU_TABLE is None:
            x = np.arange(-1024 * _ERF_GRID, 1024 * _ERF_GRID + 1) / _ERF_GRID
            _GELU_TABLE = 0.5 * x * (1.0 + np.array([math.erf(t / math.sqrt(2.0)) for t in x]))
        return _GELU_TABLE[k.astype(np.int64) + 1024 * _ERF_GRID]
    u, inv = np.unique(v, return_inverse=True)
    return (0.5 * u * (1.0 + np.array([math.erf(x / math.sqrt(2.0)) for x in u])))[inv.reshape(v.shape)]


def qgelu64(v):
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-1.702 * v))


def tgelu64(v):
    """0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))) in float64 (gelu_pytorch_tanh; vithip.h VH_EPI_BIAS_TGELU)."""
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)))


ACT64 = {"gelu": gelu64, "qgelu": qgelu64, "tgelu": tgelu64}      # keyed per activation, as the tables of act_on_grid are


def act_of(epi):
    return "qgelu" if epi in QACT else ("tgelu" if epi in TACT else "gelu")


def act64(v, epi, act=None):
    """The activation of epilogue `epi` (or the named one: the wrong_activation mutants) in float64."""
    return ACT64[act or act_of(epi)](np.asarray(v, dtype=np.float64))


def act_tolerance(ref, kind):
    """test_gpu_clip._sweep_check: |stored - f64| - ulp / 2 <= max(ERF_ABS, ulp / 4) * 1.0001, as one bound on |stored - f64|."""
    u = ulp_at(ref, kind)
    return 0.5 * u + np.maximum(ERF_ABS[kind], 0.25 * u) * 1.0001


_ACT_TABLES = {}


def act_on_grid(pre, epi, kind, want=(0, 1, 2), act=None):
    """(float64 activation, tolerance, stored bits of the rounded activation) of exact pre-activations, [M][N] each.  The designs'
    pre-activations are multiples of 1/8 below 1024: a table over that grid then serves the 4e7 elements of the many-tile shape;
    anything else is computed directly (same formulas)."""
    pre = np.asarray(pre)
    k = pre * pre.dtype.type(_ERF_GRID)
    if pre.size and np.abs(pre).max() <= 1024 and np.array_equal(k, np.rint(k)):
        key = (act or act_of(epi), kind)
        if key not in _ACT_TABLES:
            x = np.arange(-1024 * _ERF_GRID, 1024 * _ERF_GRID + 1) / _ERF_GRID
            ref = act64(x, epi, act)
            _ACT_TABLES[key] = (ref, act_tolerance(ref, kind), encode(ref.astype(np.float32), kind))
        idx = k.astype(np.int32) + 1024 * _ERF_GRID
        return tuple(t[idx] if i in want else None for i, t in enumerate(_ACT_TABLES[key]))
    ref = act64(pre, epi, act)
    return ref, act_tolerance(ref, kind), encode(ref.astype(np.float32), kind)


def act_separated(act, other, kind, step=1.0 / _ERF_GRID, below=448.0):
    """The grid points (multiples of `step`, |v| < below: no e4m3 result saturates) at which `other`, rounded to `kind`, misses the
    bound that assert_activation puts around `act`.  Empty: the suite cannot tell the two functions apart in that result type on
    that grid (e4m3 results: erf and tanh GELU, whose difference stays below the type's rounding step there)."""
    n = int(math.ceil(below / step)) - 1
    x = np.arange(-n, n + 1) * step
    ref = ACT64[act](x)
    got = decode(encode(ACT64[other](x).astype(np.float32), kind), kind).astype(np.float64)
    return x[np.abs(got - ref) > act_tolerance(ref, kind)]


def expected(case, epi, dt, before, tiles=None, ft=np.float64):
    """The buffers after the launch of `tiles` (None = all).  Activation epilogues: 'out' is absent and 'pre' holds the exact
    pre-activation [M][N] instead (assert_activation); RESID_SPLIT / PATCH_SPLIT: 'sumsq_exact' says whether partials[..., 1] is."""
    ko, k16 = out_kind(epi, dt, case.f8)
    v = pre_value(case, epi, dt, before, ft)
    mask = case.tile_mask(tiles)
    rows = case.row_map(epi)
    res = {k: a.copy() for k, a in before.items()}
    if epi in ACT:
        res.pop("out")
        res["pre"], res["mask"] = v, mask
        return res

    def put(name, vals):
        cur = res[name][rows]
        cur[mask] = vals[mask]
        res[name][rows] = cur

    if epi in SPLIT:
        hi, lo = split_planes(v, dt, case.f8)
        put("out", hi)
        put("out16", lo)
    else:
        put("out", encode(v, ko))
        if k16 is not None:
            put("out16", encode(v, k16))
    if "partials" in res:
        v64 = v.astype(np.float64).reshape(case.M, case.N // 64, 64)
        s = np.stack([v64.sum(2), (v64 * v64).sum(2)], axis=2).transpose(1, 0, 2)      # [N/64][M][2]
        bm = mask[:, ::64].T
        cur = res["partials"][:, rows]
        cur[bm] = s.astype(np.float32)[bm]
        res["partials"][:, rows] = cur
        full = np.full(res["partials"].shape[:2], np.nan)          # float64 sums of squares of the rows the launch covers
        cur = full[:, rows]
        cur[bm] = s[:, :, 1][bm]
        full[:, rows] = cur
        res["sumsq64"] = full
        # exact when every partial sum of the squares is a multiple of the grid g^2 below 2^24 grid steps
        g = min(LO_FRAC[FP8 if case.f8 else dt] or 1.0, 0.5 if case.f8 else 1.0) if epi in SPLIT else (0.5 if case.f8 else 1.0)
        res["sumsq_exact"] = bool(s[:, :, 1].max() / (g * g) < 2.0 ** 24)
    return res


# ---- the shapes of test_gpu_gemm_exact.py (K doubles with e4m3 operands: a K-tile is 128 of them) -------------------------------
def shape(name, f8=False, epi=None, four_tile_columns=False):
    """S0 one tile, the least the tiled and LDS-constant forms accept; S1 2 x 3 tiles, 7 K-tiles; S1r ragged M and N (N falls back
    to 768 -- or 1024 where the tile-range tests want 3 x 4 tiles -- for the epilogues that need whole column tiles); S2 92 x 7
    tiles = 2.5 per CU of 256, super-columns of 4 with a last one of 3."""
    whole = epi in NEED_N256 or (f8 and epi in ACT and epi in FOLD)
    M, N, K = {"S0": (256, 256, 256), "S1": (512, 768, 448), "S2": (92 * 256, 1792, 256),
               "S1r": (600, (1024 if four_tile_columns else 768) if whole else 772, 448)}[name]
    return M, N, K * (2 if f8 else 1)


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def chunk_of(kind):
    return 16 if kind in (FP8, "lo8") else 8


def to_layout(out, layout, kind):
    """Logical [M][N] -> what the launch stores: 'row', 'tiled' (16-row blocks) or 'hm' (head-major [N / 64][M][64])."""
    if layout == "row":
        return out
    if layout == "tiled":
        return vithip.pack_tiled(out, chunk_of(kind))
    M, N = out.shape
    if N % 192 == 0:       # q|k|v: the attention tap's own packer, [3][heads][M][64] = [N / 64][M][64]
        return vithip.pack_head_major(out, N // 192, M).reshape(N // 64, M, 64)
    return np.ascontiguousarray(out.reshape(M, N // 64, 64).transpose(1, 0, 2))


def from_layout(buf, layout, kind, M, N):
    if layout == "row":
        return np.asarray(buf).reshape(M, N)
    if layout == "tiled":
        return vithip.unpack_tiled(buf, M, N, chunk_of(kind))
    return np.ascontiguousarray(np.asarray(buf).reshape(N // 64, M, 64).transpose(1, 0, 2).reshape(M, N))


# ---- numpy emulation of the kernel: fp32 arithmetic, K-tile by K-tile, stores by the kernels' address formulas -----------------
ACT_MUTANTS = tuple("wrong_activation:" + a for a in ACT64)      # the emulation applies the named function whatever the epilogue's is
LEAD_MUTANTS = ("lead_off_by_one", "pos_by_output_row", "lead_row_written", "image_stride_np_plus_1")
MUTANTS = ("ktile_dropped", "ktile_twice", "neighbour_stats", "c_d_swapped", "swizzle_kept", "block_off_by_one", "hm_stride",
           "resid_twice", "resid_skipped") + ACT_MUTANTS + LEAD_MUTANTS


def mutant_applies(mutant, epi, layout, case=None, dt=None):
    """Does the mutant change what this (epilogue, layout) computes?  Where it cannot, the emulation must return the same bits.
    `case` and `dt` (the lead count, the result type) matter to the activation and lead-row mutants only."""
    if mutant in ACT_MUTANTS:
        # another function than the epilogue's own; with e4m3 results, only where the grid of the designs separates the two at all
        # (act_separated: erf and tanh GELU are NOT -- the suite's blind spot, stated by test_designs_hold_what_they_promise)
        other = mutant.split(":")[1]
        if epi not in ACT or other == act_of(epi):
            return False
        kind = out_kind(epi, dt, case.f8)[0]
        return kind != FP8 or bool(len(act_separated(act_of(epi), other, FP8)))
    if mutant in LEAD_MUTANTS:
        if epi not in PATCHES:
            return False
        # at lead 1 "pos row of the output row" IS pos row 1 + p and the image stride IS np + 1: why lead 1 alone was blind to both
        return case.lead != 1 if mutant in ("pos_by_output_row", "image_stride_np_plus_1") else True
    if mutant in ("neighbour_stats", "c_d_swapped"):
        return epi in FOLD
    if mutant == "swizzle_kept":
        return layout != "tiled"          # the tiled store leaves the registers without staging
    if mutant == "block_off_by_one":
        return layout == "tiled"
    if mutant == "hm_stride":
        return layout == "hm"
    if mutant == "resid_twice":           # an epilogue that does not read its output is idempotent
        return epi in (E["BIAS_RESID"], E["RESID_LN"], E["RESID_SPLIT"])
    return True


def _unswizzle_missing(v, elem_bytes, key_shift=0):
    """The 16-byte chunks of every 64-column group left in the staging order: chunk c of row r holds chunk c ^ key(r)."""
    M, N = v.shape
    per = 16 // elem_bytes
    nch = 64 // per
    g = v.reshape(M, N // 64, nch, per)
    key = (np.arange(M) >> key_shift) & (nch - 1)
    src = np.arange(nch)[None, :] ^ key[:, None]
    return np.take_along_axis(g, src[:, None, :, None], axis=2).reshape(M, N)


def emulate(case, epi, dt, before, tiles=None, layout="row", mutant=None):
    """-> {'out': the stored buffer in `layout` (flat for tiled / hm), 'out16', 'partials'} after launching `tiles`."""
    f32 = np.float32
    ko, k16 = out_kind(epi, dt, case.f8)
    M, N = case.M, case.N
    # the accumulator: a sum of K-tile shares, each an exact small integer (so is every partial sum: the order is immaterial)
    acc = case.acc.copy()
    j = case.nk // 2
    if mutant == "ktile_dropped":
        acc -= case.contrib(j)
    elif mutant == "ktile_twice":
        acc += case.contrib(j - 1) - case.contrib(j)      # the stage still held the previous K-tile
    st = case.stats
    if mutant == "neighbour_stats":
        st = st[np.minimum(np.arange(M) ^ 1, M - 1)]
    cvec, dvec = (case.bias, case.c) if mutant == "c_d_swapped" else (case.c, case.bias)
    mask = case.tile_mask(tiles)
    tl = list(range(case.ntiles)) if tiles is None else list(tiles)
    victim = case.tile_mask([tl[len(tl) // 2]])
    if mutant == "resid_skipped":
        mask = mask & ~victim
    rows = case.row_map(epi)
    pos_rows = case.pos_rows() if epi in PATCHES else None
    keep = slice(None)                                             # the GEMM rows whose output row lies inside the buffer: all of them
    if epi in PATCHES:
        img, p = np.arange(M) // case.np_img, np.arange(M) % case.np_img
        if mutant == "lead_off_by_one":
            rows = rows - 1
        elif mutant == "image_stride_np_plus_1":
            rows = img * (case.np_img + 1) + case.lead + p
        elif mutant == "pos_by_output_row":
            pos_rows = (case.lead + p) % (case.np_img + 1)        # (folded into the table: a row beyond it is no row at all)
        inside = (rows >= 0) & (rows < case.out_rows(epi))         # a mutant's store outside the buffer is dropped (the guard slabs' business)
        if not inside.all():
            keep = np.flatnonzero(inside)
            mask = mask & inside[:, None]
            rows = np.clip(rows, 0, case.out_rows(epi) - 1)
    wrong_act = mutant.split(":")[1] if mutant in ACT_MUTANTS else None
    state = {k: a.copy() for k, a in before.items()}
    res = {}

    def value(cur):
        if epi in FOLD:
            mr = st[:, 0] * st[:, 1]
            return st[:, 1:2] * acc + (dvec[None, :] - mr[:, None] * cvec[None, :]).astype(f32)
        v = acc + case.bias[None, :]
        if epi in (E["BIAS_RESID"], E["RESID_LN"]):
            v = v + cur["out"]
        elif epi == E["RESID_SPLIT"]:
            v = v + join_planes(cur["out"], cur["out16"], dt, case.f8).astype(f32)
        elif epi in PATCHES:
            v = v + pos_table(case, epi, dt)[pos_rows]
        return v.astype(f32)

    def apply(msk):
        v = value({k: a[rows] for k, a in state.items() if k != "partials"})
        vs = v
        if mutant == "swizzle_kept" and layout != "tiled":
            nf = N // TILE * TILE                          # whole column tiles are staged, a ragged last one stores directly
            vs = v.copy()
            if ko == "f32" or epi in SPLIT:
                vs[:, :nf] = _unswizzle_missing(v[:, :nf], 4)       # fp32 staging: 16 chunks of 4 floats, chunk ^ (r & 15)
            elif ko == FP8:
                vs[:, :nf] = _unswizzle_missing(v[:, :nf], 1, 1)    # e4m3 staging: 4 chunks of 16 bytes, chunk ^ ((r >> 1) & 3)
            else:
                vs[:, :nf] = _unswizzle_missing(v[:, :nf], 2)       # 16-bit staging: 8 chunks of 8 values, chunk ^ (r & 7)
        if epi in ACT:
            o = act_on_grid(vs, epi, ko, want=(2,), act=wrong_act)[2]
            o16 = None
        elif epi in SPLIT:
            o, o16 = split_planes(vs, dt, case.f8)
        else:
            o = encode(vs, ko)
            o16 = encode(vs, k16) if k16 is not None else None
        for name, vals in (("out", o), ("out16", o16)):
            if vals is None:
                continue
            cur = state[name][rows[keep]]
            cur[msk[keep]] = vals[keep][msk[keep]]
            state[name][rows[keep]] = cur
        if "partials" in state:
            g = vs.reshape(M, N // 64, 64)
            s = np.stack([g.sum(2, dtype=f32), (g * g).sum(2, dtype=f32)], axis=2).transpose(1, 0, 2)
            bm = msk[:, ::64].T
            cur = state["partials"][:, rows[keep]]
            cur[bm[:, keep]] = s[:, keep][bm[:, keep]]
            state["partials"][:, rows[keep]] = cur

    apply(mask)
    if mutant == "resid_twice":
        apply(victim & mask)
    if mutant == "lead_row_written" and epi in PATCHES:
        # an image's first patch row is stored once more on the row in front of it: its last lead row (at lead 0, where there is
        # none, the previous image's last patch row)
        first = np.flatnonzero((p == 0) & (rows > 0))
        for name in ("out", "out16"):
            if name in state:
                cur = state[name][rows[first] - 1]
                cur[mask[first]] = state[name][rows[first]][mask[first]]
                state[name][rows[first] - 1] = cur
    # ---- the store of `out` in its layout, by the kernels' address arithmetic (gemm_epilogue.h) ----
    out = state["out"]
    if layout == "row":
        res["out"] = out
    else:
        ch = chunk_of(ko)
        m, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
        if layout == "tiled":
            blk = m >> 4
            if mutant == "block_off_by_one":
                blk = (blk + 1) % (M // 16)
            idx = ((blk * (N // ch) + n // ch) * 16 + (m & 15)) * ch + n % ch
        else:
            stride = M - 1 if mutant == "hm_stride" else M
            idx = ((n >> 6) * stride + m) * 64 + (n & 63)
        flat = np.full(M * N, canary(ko), dtype=out.dtype)
        flat[idx.reshape(-1)] = out.reshape(-1)
        res["out"] = flat
    for k in ("out16", "partials"):
        if k in state:
            res[k] = state[k]
    return res


# ---- assertions: a failure names (tile, 16-row block, 8-column chunk, row, column) ------------------------------------------------
def where(r, n, N):
    tn = (N + TILE - 1) // TILE
    return (f"tile {(r // TILE) * tn + n // TILE} = ({r // TILE}, {n // TILE}), 16-row block {r // 16}, 8-column chunk {n // 8}, "
            f"row {r}, column {n}")


def assert_bits(got, want, what=""):
    """Bit equality of two logical [R][N] buffers (uint16, bytes, or fp32 compared as bits)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = g != w
    if bad.any():
        r, n = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} / {bad.size} elements differ in bits; first at {where(r, n, got.shape[1])}: "
                             f"got 0x{int(g[r, n]):x}, want 0x{int(w[r, n]):x}")


def ulp_at(v, kind):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** MIN_EXP[kind])))
    return 2.0 ** (e - MANT[kind])


def assert_activation(got_bits, before_bits, pre, mask, epi, kind, rows=None, what=""):
    """got_bits: logical [R][N] stored results.  Inside `mask` the stored value is the activation of the exact pre-activation
    rounded to the result type: |stored - f64| - ulp / 2 <= max(ERF_ABS, ulp / 4) (test_gpu_clip._sweep_check); outside it the
    buffer keeps its previous bits."""
    got_bits = np.asarray(got_bits)
    N = got_bits.shape[1]
    rows = np.arange(pre.shape[0]) if rows is None else rows
    keep = np.ones(got_bits.shape, dtype=bool)
    km = keep[rows]
    km[mask] = False
    keep[rows] = km
    if (got_bits[keep] != before_bits[keep]).any():
        r, n = (int(i) for i in np.argwhere(keep & (got_bits != before_bits))[0])
        raise AssertionError(f"{what}: an element outside the launched tiles was written, first at {where(r, n, N)}")
    got = decode(got_bits[rows], kind).astype(np.float64)
    ref, tol, _ = act_on_grid(pre, epi, kind, want=(0, 1))
    fin = np.isfinite(got) | ~mask
    if not fin.all():
        r, n = (int(i) for i in np.argwhere(~fin)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~fin)} results not finite, first at {where(r, n, N)}")
    over = np.abs(got - ref) - tol
    over[~mask] = -1.0
    if (over > 0).any():
        r, n = (int(i) for i in np.unravel_index(np.argmax(over), over.shape))
        raise AssertionError(f"{what}: {np.count_nonzero(over > 0)} / {over.size} activations outside the bound; worst at {where(r, n, N)}: "
                             f"pre {pre[r, n]!r}, got {got[r, n]!r}, f64 {ref[r, n]!r}, |d| {abs(got[r, n] - ref[r, n]):.3e} > {tol[r, n]:.3e}")


def assert_partials(got, want, sumsq64, sumsq_exact, what=""):
    """partials [N / 64][R][2]: the sums bit for bit; the sums of squares bit for bit where exact, else within SQ_REL of the float64
    sum sumsq64 [N / 64][R] (NaN = a row the launch does not cover: it keeps its previous bits)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)

    def name(b, r):
        return f"64-column block {b} (tile column {b // 4}), 16-row block {r // 16}, row {r}"

    bad = got[..., 0].view(np.uint32) != want[..., 0].view(np.uint32)
    if bad.any():
        b, r = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} row sums differ; first at {name(b, r)}: got {got[b, r, 0]!r}, want {want[b, r, 0]!r}")
    if sumsq_exact:
        bad = got[..., 1].view(np.uint32) != want[..., 1].view(np.uint32)
    else:
        touched = ~np.isnan(sumsq64)
        ref = np.where(touched, sumsq64, 0.0)
        bad = np.where(touched, ~(np.abs(got[..., 1].astype(np.float64) - ref) <= SQ_REL * ref), got[..., 1].view(np.uint32) != want[..., 1].view(np.uint32))
    if bad.any():
        b, r = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} sums of squares outside the bound; first at {name(b, r)}: got {got[b, r, 1]!r}, "
                             f"want {want[b, r, 1]!r}")


def check(case, epi, dt, before, got, tiles=None, what=""):
    """Every buffer of a launch, in logical form (got['out'] [R][N], ...), against expected()."""
    ko, k16 = out_kind(epi, dt, case.f8)
    exp = expected(case, epi, dt, before, tiles, np.float32 if case.M * case.N > (1 << 22) else np.float64)
    what = f"{what} {ENAME[epi]} {NAME[FP8] + '-operands ' if case.f8 else ''}{NAME[dt]} {case.M}x{case.N}x{case.K}"
    if epi in ACT:
        assert_activation(got["out"], before["out"], exp["pre"], exp["mask"], epi, ko, what=what)
    else:
        assert_bits(got["out"], exp["out"], what + " out")
    if k16 is not None:
        assert_bits(got["out16"], exp["out16"], what + " out16")
    if "partials" in exp:
        assert_partials(got["partials"], exp["partials"], exp["sumsq64"], exp["sumsq_exact"], what + " partials")


# ---- the other half of the assembly: vh_op_lead_rows on the buffers a PATCH / PATCH_SPLIT launch left -------------------------------
def lead_rows_inputs(dim, lead, no_cls, dt, split, seed=0):
    """cls [dim], pos0 [dim] (position row 0), reg [lead - 1][dim] (no_cls: cls and pos0 None, reg [lead][dim]; None without a
    register row): integers, cls and reg carrying the split form's fraction LO_FRAC[dt] so that the lo plane is busy.  Every row
    x = cls + pos0 or reg[r] is exact in fp32 and in the pair of planes, |x| < 256."""
    r = np.random.default_rng([seed, dim, lead, int(no_cls), 91])
    frac = np.float32(LO_FRAC[dt] if split else 0.0)
    regs = lead - (0 if no_cls else 1)
    return {"cls": None if no_cls else r.integers(-120, 121, size=dim).astype(np.float32) + frac,
            "pos0": None if no_cls else r.integers(-100, 101, size=dim).astype(np.float32),
            "reg": r.integers(-200, 201, size=(regs, dim)).astype(np.float32) + frac if regs else None}


def lead_rows_values(inp, ft=np.float32):
    """x [lead][dim]: row 0 = cls + pos[0], row 1 + r = reg[r]; without a class token row r = reg[r]."""
    rows = [] if inp["cls"] is None else [(inp["cls"].astype(ft) + inp["pos0"].astype(ft))[None, :]]
    if inp["reg"] is not None:
        rows.append(inp["reg"].astype(ft))
    return np.concatenate(rows, axis=0)


def lead_rows_expected(before, inp, batch, tokens, dt, split, ft=np.float64):
    """The buffers {'out' [batch * tokens][dim], and in the split form 'out16', 'partials' [dim / 64][prow][2]} after the lead-row
    kernel ran on `before`: the lead rows of every image written, every other element as it was.  Split form: also 'sumsq64' and
    'sumsq_exact', as expected() gives them."""
    x = lead_rows_values(inp, ft)
    lead, dim = x.shape
    res = {k: a.copy() for k, a in before.items()}
    at = (np.arange(batch)[:, None] * tokens + np.arange(lead)[None, :]).reshape(-1)       # image-major, as x tiles
    x32 = np.tile(x.astype(np.float32), (batch, 1))
    if not split:
        res["out"][at] = x32
        return res
    res["out"][at], res["out16"][at] = split_planes(x32, dt, False)
    g = np.tile(x.astype(np.float64), (batch, 1)).reshape(batch * lead, dim // 64, 64)
    s = np.stack([g.sum(2), (g * g).sum(2)], axis=2).transpose(1, 0, 2)                    # [dim / 64][batch * lead][2]
    res["partials"][:, at] = s.astype(np.float32)
    res["sumsq64"] = np.full(res["partials"].shape[:2], np.nan)
    res["sumsq64"][:, at] = s[:, :, 1]
    res["sumsq_exact"] = bool(s[:, :, 1].max() / LO_FRAC[dt] ** 2 < 2.0 ** 24)
    return res


def check_lead_rows(before, got, inp, batch, tokens, dt, split, what=""):
    exp = lead_rows_expected(before, inp, batch, tokens, dt, split)
    assert_bits(got["out"], exp["out"], what + " out")
    if split:
        assert_bits(got["out16"], exp["out16"], what + " out16")
        assert_partials(got["partials"], exp["partials"], exp["sumsq64"], exp["sumsq_exact"], what + " partials")
