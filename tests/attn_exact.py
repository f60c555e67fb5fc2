"""Exactly predictable attention inputs, their float64 reference, a numpy emulation of the kernels' arithmetic and the
per-element assertions of test_attention_exact.py (CPU) and test_gpu_attention_exact.py (GPU).  No GPU, no oracle.

The attention kernels work in the exp2 domain on a q that arrives already scaled, so a test controls the log2-domain scores
q.k directly.  With small-integer q and k every score is an exact integer (in the MFMA's fp32 accumulator, in the class-token
kernel's fmaf chain and here), every probability 2^(s - shift) an exact power of two -- exact in fp16 and bf16 as well -- and
with small-integer V the result is the correctly rounded quotient sum(p v) / sum(p) up to the noise of the fp32 sums.

Layout everywhere: the taps' row-major q|k|v [batch * T][3 * heads * hd] -> out [batch * T][heads * hd].  Every design puts its
active q / k columns at seeded positions among the hd columns that differ per head (the k-step and swizzle mapping matter), and V
differs per (image, head).

  uniform      q = 0, k small integers, V integers in [-8, 8] with V[T-1] = +-8 (and V[0] = -V[T-1]): every p is 1, l = T.
               The pure key-mask test: one key too many or too few moves every column by about 8 / T.
  graded       ten active columns, q in {0, 1}, k = +1 with at most four -1 per key and all-zero on keys 0..31: the tile-0
               shift of every row is 0 and the scores lie in [-4, 10].  Every third 32-row block is capped at 8 ones per query:
               it reaches p = 2^8 under the stale shift WITHOUT a rescale; the other blocks hold queries that reach 9 and 10 and
               force it (kTau = 8).  No p falls below 2^-14 (fp16's smallest normal).  The last key has no -1.
  permutation  13 active columns, k_j = +-4 coding the bits of j, q_i = +-4 coding the bits of pi(i) for a seeded permutation pi
               per (image, head): score = 16 * (13 - 2 * hamming), every improvement is a step of 32 > kTau (each one
               rescales), the match ends with p = 1 exactly and every other key below 2^-32.  V = values already rounded to
               the storage type, magnitudes in [1/4, 8): the result is V[pi(i)] BIT FOR BIT.
"""
import numpy as np

import vithip

BF16, FP16, FP8 = vithip.DTYPE_BF16, vithip.DTYPE_FP16, vithip.DTYPE_FP8
NAME = {BF16: "bf16", FP16: "fp16", FP8: "e4m3"}
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}   # test_gpu_ops.ULP: the relative rounding step of a 16-bit result
K_TAU = 8.0                                 # kernels_attn*.hip kTau
VMAX = 8.0                                  # max |V| of every design
# fp32 noise allowance, relative to max |V|: 512 roundings at 2^-24 relative to sum |p v| / l <= max |V| (a 4097-key row performs
# fewer than 300: 129 tile sums, 129 PV accumulations, the rescales, rcp and the product).  Derived, not measured.
EXTRA_REL = 2.0 ** -17
DESIGNS = ("uniform", "graded", "permutation")


def _rng(seed, *key):
    return np.random.default_rng([int(seed)] + [int(k) for k in key])


def _round_dt(a, dt):
    return vithip.from16(vithip.to16(np.asarray(a, dtype=np.float32), dt), dt)


class Case:
    """One generated problem: qkv (fp32 values that are exact in bf16 and fp16), its shape, and for the permutation design
    the target key of every query, pi [batch][heads][T]."""

    def __init__(self, design, qkv, batch, tokens, heads, hd, pi=None):
        self.design, self.qkv, self.batch, self.tokens, self.heads, self.hd, self.pi = design, qkv, batch, tokens, heads, hd, pi

    @property
    def dim(self):
        return self.heads * self.hd

    def v_of(self, b, h):
        D, T = self.dim, self.tokens
        return self.qkv[b * T:(b + 1) * T, 2 * D + h * self.hd:2 * D + (h + 1) * self.hd]

    def expected_permutation(self):
        """V[pi(i)] per (image, head): what the permutation design must return bit for bit, [batch * T][dim] fp32."""
        out = np.empty((self.batch * self.tokens, self.dim), dtype=np.float32)
        for b in range(self.batch):
            for h in range(self.heads):
                out[b * self.tokens:(b + 1) * self.tokens, h * self.hd:(h + 1) * self.hd] = self.v_of(b, h)[self.pi[b, h]]
        return out


def make_case(design, batch, tokens, heads, hd, seed=0, vdtype=FP16):
    """vdtype: the type V of the permutation design is rounded to (BF16, FP16, or FP8 = e4m3-representable values, which are
    bf16 values too); the other designs hold small integers whatever the type."""
    assert design in DESIGNS and hd >= 16 and tokens >= 1
    T, D = tokens, heads * hd
    qkv = np.zeros((batch * T, 3 * D), dtype=np.float32)
    pi = np.zeros((batch, heads, T), dtype=np.int64) if design == "permutation" else None
    nact = {"uniform": hd, "graded": 10, "permutation": 13}[design]
    for h in range(heads):
        cols = np.sort(_rng(seed, 1, h, hd).permutation(hd)[:nact])   # per head, shared by the images
        for b in range(batch):
            r = _rng(seed, 2, b, h, T, hd)
            q = np.zeros((T, hd), dtype=np.float32)
            k = np.zeros((T, hd), dtype=np.float32)
            if design == "uniform":
                k = r.integers(-3, 4, size=(T, hd)).astype(np.float32)
            elif design == "graded":
                cap = np.where((np.arange(T) // 32) % 3 == 0, 8, 10)
                ones = r.integers(0, cap + 1)                     # ones per query: 0..8 in the capped blocks, 0..10 elsewhere
                order = np.argsort(r.random((T, 10)), axis=1)
                qa = (np.argsort(order, axis=1) < ones[:, None]).astype(np.float32)
                flips = r.integers(0, 5, size=T)
                flips[T - 1] = 0
                order = np.argsort(r.random((T, 10)), axis=1)
                ka = np.where(np.argsort(order, axis=1) < flips[:, None], -1.0, 1.0).astype(np.float32)
                ka[:32] = 0.0
                q[:, cols], k[:, cols] = qa, ka
            else:
                p = r.permutation(T)
                pi[b, h] = p
                bits = np.arange(13)
                k[:, cols] = np.where((np.arange(T)[:, None] >> bits) & 1, 4.0, -4.0)
                q[:, cols] = np.where((p[:, None] >> bits) & 1, 4.0, -4.0)
            if design == "permutation":
                if vdtype == FP8:   # (1 + m / 8) * 2^e, e in -2..2: e4m3 and bf16 values
                    v = (1.0 + r.integers(0, 8, size=(T, hd)) / 8.0) * 2.0 ** r.integers(-2, 3, size=(T, hd))
                else:
                    v = _round_dt(r.uniform(0.25, 7.9, size=(T, hd)), vdtype)
                v = (v * r.choice([-1.0, 1.0], size=(T, hd))).astype(np.float32)
            else:
                v = r.integers(-8, 9, size=(T, hd)).astype(np.float32)
                v[T - 1] = r.choice([-8.0, 8.0], size=hd)
                if T > 1:
                    v[0] = -v[T - 1]
            rows = slice(b * T, (b + 1) * T)
            qkv[rows, h * hd:(h + 1) * hd] = q
            qkv[rows, D + h * hd:D + (h + 1) * hd] = k
            qkv[rows, 2 * D + h * hd:2 * D + (h + 1) * hd] = v
    return Case(design, qkv, batch, T, heads, hd, pi)


def reference(case, rows=None):
    """float64, log2 domain: P = 2^(S - rowmax), out = P V / sum P per (image, head).  rows: None = every query, or a list of
    query indices per image (the class-token tap: [0]) -> [batch * len(rows)][dim]."""
    B, T, H, hd, D = case.batch, case.tokens, case.heads, case.hd, case.dim
    qi = np.arange(T) if rows is None else np.asarray(rows)
    out = np.empty((B * len(qi), D), dtype=np.float64)
    x = case.qkv.astype(np.float64)
    for b in range(B):
        img = x[b * T:(b + 1) * T]
        for h in range(H):
            q, k, v = (img[:, i * D + h * hd:i * D + (h + 1) * hd] for i in range(3))
            for c0 in range(0, len(qi), 1024):
                sel = qi[c0:c0 + 1024]
                s = q[sel] @ k.T
                p = np.exp2(s - s.max(axis=1, keepdims=True))
                out[b * len(qi) + c0:b * len(qi) + c0 + len(sel), h * hd:(h + 1) * hd] = (p @ v) / p.sum(axis=1, keepdims=True)
    return out


def emulate(case, dt, mutant=None):
    """The ring / streaming / head-dim kernels' arithmetic in numpy: fp32 scores that start at -shift, the shift = the row's
    tile-0 maximum, re-centred for a whole 32-row wave when any of its rows exceeds it by more than 2^kTau, P rounded to the
    16-bit operand type, fp32 sums, fp32 division in place of rcp, the result rounded to `dt` (FP8: bf16 operands, e4m3 out).
    mutant: None, "extra_key" (key T, a replica of row T-1, is not masked), "drop_last" (key T-1 is masked), "swap_heads" (V is
    read from head h ^ 1).  Returns (out fp32 [batch * T][dim], {"rescales": wave-tile rescale events, "blocks": per (image,
    head) the set of 32-row blocks that rescaled, "pmax": the largest probability a P operand held})."""
    B, T, H, hd, D = case.batch, case.tokens, case.heads, case.hd, case.dim
    opdt = BF16 if dt == FP8 else dt
    valid = T + (mutant == "extra_key") - (mutant == "drop_last")
    ntiles = max(1, (valid + 31) // 32)
    nblk = (T + 31) // 32
    out = np.empty((B * T, D), dtype=np.float32)
    stats = {"rescales": 0, "blocks": {}, "pmax": 0.0}
    f32 = np.float32
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            img = case.qkv[b * T:(b + 1) * T]
            for h in range(H):
                hv = h ^ 1 if mutant == "swap_heads" and (h ^ 1) < H else h
                q = img[np.minimum(np.arange(nblk * 32), T - 1), h * hd:(h + 1) * hd]   # rows >= T run the clamped last row
                k = img[:, D + h * hd:D + (h + 1) * hd]
                v = img[:, 2 * D + hv * hd:2 * D + (hv + 1) * hd]
                o = np.zeros((nblk * 32, hd), dtype=f32)
                l = np.zeros(nblk * 32, dtype=f32)
                negm = np.zeros(nblk * 32, dtype=f32)
                hit = set()
                for kt in range(ntiles):
                    keys = np.arange(kt * 32, kt * 32 + 32)
                    src = np.minimum(keys, T - 1)                                       # rows >= T replicate the last row
                    s = (negm[:, None] + q @ k[src].T).astype(f32)
                    s[:, keys >= valid] = -np.inf
                    mx = s.max(axis=1)
                    if kt == 0:
                        negm = -mx
                        s = s - mx[:, None]
                    else:
                        wave = (mx.reshape(nblk, 32) > K_TAU).any(axis=1)
                        if wave.any():
                            stats["rescales"] += int(wave.sum())
                            hit.update(np.nonzero(wave)[0].tolist())
                            rowsel = np.repeat(wave, 32)
                            delta = np.where(rowsel, np.maximum(mx, f32(0)), f32(0)).astype(f32)
                            alpha = np.exp2(-delta).astype(f32)
                            negm = negm - delta
                            l = l * alpha
                            o = o * alpha[:, None]
                            s = s - delta[:, None]
                    p = np.exp2(s).astype(f32)
                    l = l + p.sum(axis=1, dtype=f32)
                    p16 = _round_dt(p, opdt)
                    fin = p16[np.isfinite(p16)]
                    if fin.size:
                        stats["pmax"] = max(stats["pmax"], float(fin.max()))
                    o = o + (p16 @ v[src]).astype(f32)
                stats["blocks"][(b, h)] = hit
                res = (o / l[:, None]).astype(f32)[:T]
                out[b * T:(b + 1) * T, h * hd:(h + 1) * hd] = round_out(res, dt)
    return out, stats


def round_out(a, dt):
    """fp32 -> the kernel's output type and back (NaN stays NaN for the 16-bit types; e4m3 saturates like pack4_e4m3)."""
    a = np.asarray(a, dtype=np.float32)
    if dt == FP8:
        r = vithip.from_e4m3(vithip.to_e4m3(np.nan_to_num(a, nan=0.0)))
        return np.where(np.isnan(a), np.float32(np.nan), r).astype(np.float32)
    return _round_dt(a, dt)


# ---- assertions ---------------------------------------------------------------------------------------------------------
def _where(idx, tokens, heads, hd, rows_per_image):
    r, c = int(idx[0]), int(idx[1])
    return f"image {r // rows_per_image} head {c // hd} row {r % rows_per_image} column {c % hd} (T = {tokens}, heads = {heads}, hd = {hd})"


def tolerance(ref, dt, vmax=VMAX):
    """Per-element bound.  16-bit results: test_gpu_ops.assert_close16's 1.01 * ULP * |ref| + extra with extra = 2^-17 * max|V|.
    e4m3 results: half an e4m3 step (2^-4 relative) plus the subnormal step 2^-10, plus the same extra."""
    extra = EXTRA_REL * vmax
    if dt == FP8:
        return 1.01 * 2.0 ** -4 * np.abs(ref) + 2.0 ** -10 + extra
    return 1.01 * ULP[dt] * np.abs(ref) + extra


def excess(got, ref, dt, vmax=VMAX):
    """Worst (|d| - ULP * |ref|) / max|V| (what `extra` has to cover, recorded in profiles/attn_exact_gpu_tests.txt)."""
    step = 2.0 ** -4 if dt == FP8 else ULP[dt]
    sub = 2.0 ** -10 if dt == FP8 else 0.0
    return float(np.max(np.abs(got.astype(np.float64) - ref) - step * np.abs(ref) - sub) / vmax)


def assert_elements(got, ref, dt, case, what="", rows_per_image=None, vmax=VMAX):
    """Every element finite and inside tolerance(); a failure names image, head, row, column and T of the worst element."""
    rpi = rows_per_image or case.tokens
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(got)
    if not fin.all():
        idx = np.argwhere(~fin)[0]
        raise AssertionError(f"{what} {case.design} {NAME[dt]}: {np.count_nonzero(~fin)} / {got.size} elements not finite "
                             f"(unwritten or NaN), first at {_where(idx, case.tokens, case.heads, case.hd, rpi)}")
    d = np.abs(got - ref)
    bad = d > tolerance(ref, dt, vmax)
    if bad.any():
        idx = np.unravel_index(np.argmax(np.where(bad, d - tolerance(ref, dt, vmax), -1.0)), d.shape)
        raise AssertionError(f"{what} {case.design} {NAME[dt]}: {np.count_nonzero(bad)} / {bad.size} elements outside the bound; "
                             f"worst at {_where(idx, case.tokens, case.heads, case.hd, rpi)}: got {got[idx]!r}, ref {ref[idx]!r}, "
                             f"|d| {d[idx]:.3e} > {tolerance(ref, dt, vmax)[idx]:.3e}")


def assert_bits(got_bits, want_bits, case, dt, what="", rows_per_image=None):
    """Bit equality of stored results (uint16 or e4m3 bytes); a failure names the first differing element."""
    rpi = rows_per_image or case.tokens
    got_bits, want_bits = np.asarray(got_bits), np.asarray(want_bits)
    assert got_bits.shape == want_bits.shape and got_bits.dtype == want_bits.dtype, (got_bits.shape, want_bits.shape)
    bad = got_bits != want_bits
    if bad.any():
        idx = np.argwhere(bad)[0]
        raise AssertionError(f"{what} {case.design} {NAME[dt]}: {np.count_nonzero(bad)} / {bad.size} elements differ in bits; first at "
                             f"{_where(idx, case.tokens, case.heads, case.hd, rpi)}: got 0x{int(got_bits[tuple(idx)]):x}, "
                             f"want 0x{int(want_bits[tuple(idx)]):x}")


def to_bits(a, dt):
    """fp32 values that are exact in `dt` -> their stored form (uint16, or e4m3 bytes for FP8)."""
    return vithip.to_e4m3(a) if dt == FP8 else vithip.to16(a, dt)
