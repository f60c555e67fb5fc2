"""GPU, per element: every GEMM launch form against exactly predictable inputs (tests/gemm_exact.py).

The operator tests of test_gpu_ops / test_gpu_fp8 / test_gpu_clip compare the GEMM with the oracle on random data at 1 ulp plus an
absolute extra, through taps that cannot ask for the tiled hidden activation, the head-major q|k|v, tiled A / W operands or a tile
range: the forms the forward runs by default were reached through whole forwards only.  Here the accumulators are exact small
integers, so every epilogue but the activations is compared BIT FOR BIT, per element, in every layout (taps vh_op_gemm_layout,
vh_op_gemm_fp8_layout, vh_op_tile_rows), and a failure names tile, 16-row block, 8-column chunk, row and column.
test_gemm_exact.py proves on the CPU that these assertions fail for a dropped or repeated K-tile, a neighbouring row's statistics,
swapped c / d, a kept staging swizzle, an off-by-one row block, a wrong head-major stride, a residual tile applied twice or not
at all, another activation than the epilogue's, and the four ways a lead-row remap goes wrong.

The three activations (erf, QuickGELU and tanh GELU; codes EPI_*_GELU / _QGELU / _TGELU) run through every form: row-major at every
variant, the tiled hidden activation with 16-bit and e4m3 results, a tile range.  Their bound is the activation sweeps' (gemm_exact
.act_tolerance).  What that bound cannot see: with e4m3 RESULTS the erf and the tanh GELU round alike at every pre-activation of
the designs, so a kernel that ran one for the other would pass the e4m3 forms (test_gemm_exact.py asserts that this is so, and that
every other pair, and every pair with 16-bit results, separates); the 16-bit forms of the same code paths catch it.

The patch-embedding epilogues run through vh_op_gemm_lead with 0, 1, 5 and 17 rows in front of an image's patch rows -- registers,
no-class-token models, SigLIP, DINOv3 -- with several column tiles, image boundaries inside every 128-row wave tile, a ragged last
row tile, every variant: the patch rows, the untouched lead rows and the partial sums (a padded row stride) bit for bit.  At lead 1
"pos row 1 + p" and "pos row of the output row" are one row; only the other leads tell them apart.  vh_op_lead_rows then completes
the assembly on the same buffers and is compared with cls + pos[0] and reg[r] themselves, not with another run of the kernel.

Every buffer a launch may write is exactly sized, pre-filled (canaries, or the residual it updates) and has a guard slab of 0xA5
bytes in front of and behind it that must survive.

Shapes (gemm_exact.shape): S0 one tile; S1 2 x 3 tiles and 7 K-tiles (an odd count >= 4: the LDS-prefetched LN-fold constants, both
stage rings wrapped an odd number of times); S1r ragged; S2 644 tiles (2.5 per CU: persistent workgroups walk two and three
tiles in super-columns of 4 + 3), one epilogue per layout family.
"""
import numpy as np
import pytest

import gemm_exact as X
from vh_testlib import _release_buffers, dev

pytestmark = pytest.mark.gpu

vithip = pytest.importorskip("vithip")
E, BF16, FP16, FP8 = X.E, X.BF16, X.FP16, X.FP8
DT = [BF16, FP16]
GUARD = 0xA5
_CASES = {}


def case_of(M, N, K, f8):
    """Generated once per shape and shared, unchanged, by the tests."""
    key = (M, N, K, f8)
    if key not in _CASES:
        if M * N > 1 << 22 or len(_CASES) > 12:
            _CASES.clear()
        _CASES[key] = X.Case(M, N, K, f8)
    return _CASES[key]


class Launch:
    """The device side of one (case, epilogue, type): operands, epilogue inputs and guarded output buffers holding `before`."""

    def __init__(self, case, epi, dt, before, layout="row", ab_tiled=False, w_tiled_ptr=None, lead_tap=False):
        self.case, self.epi, self.dt, self.layout, self.ab_tiled, self.lead_tap = case, epi, dt, layout, ab_tiled, lead_tap
        assert lead_tap or (case.lead == 1 and not case.pad_rows), "every other tap keeps lead = 1 and prow = the token rows"
        self.ko, self.k16 = X.out_kind(epi, dt, case.f8)
        a, w = case.operand_bits(dt)
        chunk = 16 if case.f8 else 8
        self.a = dev(vithip.pack_tiled(a, chunk) if ab_tiled else a)
        self.w_ptr = w_tiled_ptr if w_tiled_ptr else dev(vithip.pack_tiled(w, chunk) if ab_tiled else w).ptr
        self.bias, self.ws = dev(case.bias), dev(case.ws)
        self.c = dev(case.c) if epi in X.FOLD else None
        self.stats = dev(case.stats) if epi in X.FOLD else None
        self.pos = dev(X.pos_table(case, epi, dt)) if epi in X.PATCHES else None
        self.shapes, self.bufs, self.guards = {}, {}, {}
        for name, arr in before.items():
            payload = X.to_layout(arr, layout, self.ko) if name == "out" else arr
            raw = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
            g = (max(arr.shape[-1] * arr.itemsize * (16 if layout != "row" else 1), 256) + 255) // 256 * 256
            self.shapes[name], self.guards[name] = arr, g
            self.bufs[name] = dev(np.concatenate([np.full(g, GUARD, np.uint8), raw, np.full(g, GUARD, np.uint8)]))

    def ptr(self, name):
        return self.bufs[name].ptr + self.guards[name] if name in self.bufs else None

    def launch(self, variant, tiles=None):
        c, epi = self.case, self.epi
        tb, tc = (tiles[0], len(tiles)) if tiles is not None else (0, 0)
        extras = dict(out_tiled=self.layout != "row", ab_tiled=self.ab_tiled, tile_begin=tb, tile_count=tc)
        plain = not (extras["out_tiled"] or self.ab_tiled or tc)      # then the taps the layout taps extend
        if self.lead_tap:      # the patch forms with case.lead rows in front of an image's patch rows; prow as the case pads it
            vithip.op_gemm_lead(self.a.ptr, self.w_ptr, self.bias.ptr, self.ptr("out"), c.M, c.N, c.K, epi, self.dt, self.pos.ptr if self.pos else None,
                                c.np_img, c.lead, out16_ptr=self.ptr("out16"), partials_ptr=self.ptr("partials"),
                                prow=c.partial_rows(epi) if c.pad_rows else 0, variant=variant)
        elif c.f8:
            args = (self.a.ptr, self.w_ptr, self.ws.ptr, self.bias.ptr, self.ptr("out"), c.M, c.N, c.K, epi)
            kw = dict(c_ptr=self.c.ptr if self.c else None, stats_ptr=self.stats.ptr if self.stats else None, out16_ptr=self.ptr("out16"),
                      partials_ptr=self.ptr("partials"), variant=variant)
            if not plain:
                vithip.op_gemm_fp8_layout(*args, **kw, **extras)
            elif epi in X.FOLD or epi in (E["RESID_LN"], E["RESID_SPLIT"]):
                vithip.op_gemm_fp8_ex(*args, **kw)
            else:
                vithip.op_gemm_fp8(*args, variant)
        else:
            aux = self.c.ptr if self.c else (self.pos.ptr if self.pos else None)
            args = (self.a.ptr, self.w_ptr, self.bias.ptr, self.ptr("out"), c.M, c.N, c.K, epi, self.dt)
            kw = dict(aux_ptr=aux, aux_i=c.np_img if epi in X.PATCHES else 0, stats_ptr=self.stats.ptr if self.stats else None,
                      out16_ptr=self.ptr("out16"), partials_ptr=self.ptr("partials"), variant=variant)
            (vithip.op_gemm_ex if plain else vithip.op_gemm_layout)(*args, **kw, **({} if plain else extras))

    def read(self, what="", stored=False):
        """The buffers back in logical form, after checking the guard slabs.  stored: also 'out_stored', the buffer as it lies in memory."""
        res = {}
        for name, b in self.bufs.items():
            arr, g = self.shapes[name], self.guards[name]
            raw = b.to_numpy(np.uint8, (2 * g + arr.nbytes,))
            assert np.all(raw[:g] == GUARD) and np.all(raw[-g:] == GUARD), f"{what}: a guard slab around `{name}` was written"
            body = np.ascontiguousarray(raw[g:-g]).view(arr.dtype)
            if name == "out":
                if stored:
                    res["out_stored"] = body
                res[name] = X.from_layout(body, self.layout, self.ko, arr.shape[0], arr.shape[1])
            else:
                res[name] = body.reshape(arr.shape)
        return res


def run_and_check(case, epi, dt, variant, layout="row", ab_tiled=False, w_tiled_ptr=None, tiles=None, stored=False, lead_tap=False, keep=None):
    before = X.initial(case, epi, dt)
    L = Launch(case, epi, dt, before, layout, ab_tiled, w_tiled_ptr, lead_tap)
    L.launch(variant, tiles)
    what = f"variant {variant} {layout}{' ab_tiled' if ab_tiled else ''}{'' if tiles is None else f' tiles {tiles[0]}..{tiles[-1]}'}"
    if lead_tap:
        what += f" lead {case.lead}, {case.np_img} patches per image"
    got = L.read(what, stored)
    X.check(case, epi, dt, before, got, tiles, what)
    if keep is not None:
        keep.append(L)         # the device side, for a caller that goes on with the buffers
    return before, got


def same_bits(a, b, what):
    for k in a:
        if k != "out_stored":
            X.assert_bits(a[k].reshape(a[k].shape[0], -1) if a[k].ndim != 2 else a[k], b[k].reshape(b[k].shape[0], -1) if b[k].ndim != 2 else b[k],
                          f"{what} `{k}`")


# ---- 1. row-major: every epilogue x every variant ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("epi", X.EPI_16BIT_OPERANDS, ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", ["S1", "S1r"])
def test_row_major_16bit_operands(name, epi, dt):
    for variant in (1, 2, 5, 6, 7):
        M, N, K = X.shape(name, False, epi)
        if variant == 6 and N % 256:
            N = 768        # ragged N would only send the persistent variant to variant 5's code
        run_and_check(case_of(M, N, K, False), epi, dt, variant)


@pytest.mark.parametrize("epi", X.EPI_E4M3_OPERANDS, ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", ["S1", "S1r"])
def test_row_major_e4m3_operands(name, epi):
    for variant in (5, 6, 7):
        M, N, K = X.shape(name, True, epi)
        if variant == 6 and N % 256:
            N = 768
        run_and_check(case_of(M, N, K, True), epi, BF16, variant)


# ---- 2. the tiled and head-major layouts (variant 6) ---------------------------------------------------------------------------
LAYOUT_SHAPES = ["S0", "S1"]


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("epi", X.ACT, ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", LAYOUT_SHAPES)
def test_tiled_hidden_activation(name, epi, dt):
    case = case_of(*X.shape(name, False, epi), False)
    _, tiled = run_and_check(case, epi, dt, 6, layout="tiled")
    _, row = run_and_check(case, epi, dt, 6)
    same_bits(tiled, row, "tiled vs row-major")


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("epi", [E["LNFOLD"], E["BIAS"]], ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", LAYOUT_SHAPES)
def test_head_major_result(name, epi, dt):
    case = case_of(*X.shape(name, False, epi), False)
    before, got = run_and_check(case, epi, dt, 6, layout="hm", stored=True)
    want = X.expected(case, epi, dt, before)["out"]
    hm = X.to_layout(want, "hm", dt)       # vithip.pack_head_major where N is q|k|v-shaped
    X.assert_bits(got["out_stored"].reshape(case.N // 64 * case.M // 16, 16 * 64), hm.reshape(case.N // 64 * case.M // 16, 16 * 64), "head-major buffer")


def tiled_w_on_device(case, dt):
    """W through vh_op_tile_rows; must equal pack_tiled of the rounded matrix bit for bit.  Returns the device pointer."""
    _, w = case.operand_bits(dt)
    if case.f8:
        src, chunk = dev(w), 16
    else:
        src, chunk = dev(case.w), 8
    out = dev(np.full(w.nbytes + 512, GUARD, np.uint8))
    vithip.op_tile_rows(src.ptr, case.N, case.K, out.ptr + 256, FP8 if case.f8 else dt)
    raw = out.to_numpy(np.uint8, (w.nbytes + 512,))
    assert np.all(raw[:256] == GUARD) and np.all(raw[-256:] == GUARD)
    got = np.ascontiguousarray(raw[256:-256]).view(w.dtype)
    X.assert_bits(got.reshape(case.N // 16, -1), vithip.pack_tiled(w, chunk).reshape(case.N // 16, -1), "vh_op_tile_rows(W): rows are 16-row blocks")
    return out.ptr + 256


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("epi", [E["RESID_SPLIT"], E["BIAS"]], ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", LAYOUT_SHAPES)
def test_tiled_operands(name, epi, dt):
    case = case_of(*X.shape(name, False, epi), False)
    _, host = run_and_check(case, epi, dt, 6, ab_tiled=True)                                   # A and W packed on the host
    _, devw = run_and_check(case, epi, dt, 6, ab_tiled=True, w_tiled_ptr=tiled_w_on_device(case, dt))
    same_bits(host, devw, "W tiled on the device vs on the host")


@pytest.mark.parametrize("form", ["tiled_LNFOLD_GELU", "tiled_BIAS_GELU", "tiled_LNFOLD_QGELU", "tiled_BIAS_QGELU", "tiled_LNFOLD_TGELU", "tiled_BIAS_TGELU",
                                  "hm_LNFOLD", "ab_RESID_SPLIT"])
@pytest.mark.parametrize("name", LAYOUT_SHAPES)
def test_e4m3_operand_layouts(name, form):
    kind, ename = form.split("_", 1)
    epi = E[ename]
    case = case_of(*X.shape(name, True, epi), True)
    if kind == "tiled":        # the e4m3 hidden activation, [M / 16][N / 16][16][16 B]
        _, tiled = run_and_check(case, epi, BF16, 6, layout="tiled")
        _, row = run_and_check(case, epi, BF16, 6)
        same_bits(tiled, row, "tiled vs row-major")
    elif kind == "hm":         # bf16 q|k|v head-major
        before, got = run_and_check(case, epi, BF16, 6, layout="hm", stored=True)
        hm = X.to_layout(X.expected(case, epi, BF16, before)["out"], "hm", BF16)
        X.assert_bits(got["out_stored"].reshape(-1, 1024), hm.reshape(-1, 1024), "head-major buffer")
    else:                      # tiled e4m3 A / W into the split residual
        _, host = run_and_check(case, epi, BF16, 6, ab_tiled=True)
        _, devw = run_and_check(case, epi, BF16, 6, ab_tiled=True, w_tiled_ptr=tiled_w_on_device(case, BF16))
        same_bits(host, devw, "W tiled on the device vs on the host")


@pytest.mark.parametrize("form", ["tiled", "hm", "ab", "tiled_e4m3"])
def test_layouts_where_workgroups_walk_several_tiles(form):
    # S2: 644 tiles on 256 CUs, 7 column tiles in super-columns of 4 + 3; one epilogue per layout family, bf16
    f8 = form == "tiled_e4m3"
    epi = {"tiled": E["LNFOLD_GELU"], "hm": E["LNFOLD"], "ab": E["BIAS"], "tiled_e4m3": E["LNFOLD_GELU"]}[form]
    case = case_of(*X.shape("S2", f8, epi), f8)
    if form == "ab":
        run_and_check(case, epi, BF16, 6, ab_tiled=True, w_tiled_ptr=tiled_w_on_device(case, BF16))
    else:
        run_and_check(case, epi, BF16, 6, layout="hm" if form == "hm" else "tiled")


# ---- 3. vh_op_tile_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, FP16, FP8], ids=lambda d: X.NAME[d])
def test_tile_rows(dt):
    r = np.random.default_rng(17)
    chunk = 16 if dt == FP8 else 8
    for rows, cols in ((16, chunk), (48, 208 if dt == FP8 else 200), (768, 896 if dt == FP8 else 448)):
        if dt == FP8:
            src = r.integers(0, 256, size=(rows, cols)).astype(np.uint8)
            want = vithip.pack_tiled(src, 16)
        else:
            src = (r.standard_normal((rows, cols)) * 3).astype(np.float32)      # rounds on the way: round to nearest even
            want = vithip.pack_tiled(vithip.to16(src, dt), 8)
        out = dev(np.full(want.nbytes + 512, GUARD, np.uint8))
        vithip.op_tile_rows(dev(src).ptr, rows, cols, out.ptr + 256, dt)
        raw = out.to_numpy(np.uint8, (want.nbytes + 512,))
        assert np.all(raw[:256] == GUARD) and np.all(raw[-256:] == GUARD), (rows, cols)
        got = np.ascontiguousarray(raw[256:-256]).view(want.dtype).reshape(want.shape)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{rows} x {cols} {X.NAME[dt]}: {len(bad)} elements differ, first at (16-row block, chunk, row, element) {tuple(bad[0])}"
    b = dev(np.full(4096, GUARD, np.uint8))
    for args in ((b.ptr, 8, chunk, b.ptr, dt), (b.ptr, 16, chunk - 4, b.ptr, dt), (b.ptr, 0, chunk, b.ptr, dt), (None, 16, chunk, b.ptr, dt),
                 (b.ptr, 16, chunk, None, dt), (b.ptr, 16, 16, b.ptr, 7)):
        with pytest.raises(vithip.VhError) as e:
            vithip.op_tile_rows(*args)
        assert e.value.code == 1 and str(e.value), args
    assert np.all(b.to_numpy(np.uint8, (4096,)) == GUARD)


# ---- 4. tile ranges (variants 5 and 7) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [5, 7])
@pytest.mark.parametrize("epi", [E["BIAS"], E["RESID_LN"], E["RESID_SPLIT"]], ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("ops", ["bf16", "fp16", "e4m3"])
def test_tile_ranges(ops, epi, variant):
    tile_ranges(ops, epi, variant)


@pytest.mark.parametrize("variant", [5, 7])
@pytest.mark.parametrize("ops", ["bf16", "fp16"])
def test_tile_ranges_tanh_gelu(ops, variant):
    # an activation epilogue in a tile range: the tiles outside it keep their canaries, the two ranges give the one launch's bits
    tile_ranges(ops, E["BIAS_TGELU"], variant)


def tile_ranges(ops, epi, variant):
    f8 = ops == "e4m3"
    dt = FP16 if ops == "fp16" else BF16
    M, N, K = X.shape("S1r", f8, epi, four_tile_columns=True)
    N = N if N % 256 == 0 else 1024 - 252
    case = case_of(M, N, K, f8)
    assert (case.tiles_m, case.tiles_n) == (3, 4)
    before = X.initial(case, epi, dt)
    L = Launch(case, epi, dt, before)
    L.launch(variant, range(0, 5))
    first = L.read("tiles 0..4")
    X.check(case, epi, dt, before, first, range(0, 5), f"variant {variant} tiles 0..4")      # tiles 5..11 keep their bits
    L.launch(variant, range(5, 12))
    both = L.read("tiles 0..4 then 5..11")
    full = Launch(case, epi, dt, before)
    full.launch(variant)
    whole = full.read("all tiles")
    X.check(case, epi, dt, before, whole, None, f"variant {variant} all tiles")
    same_bits(both, whole, f"variant {variant}: [0, 5) + [5, 12) vs one launch")               # every residual tile applied once
    run_and_check(case, epi, dt, variant, tiles=range(8, 12))                                  # the ragged last tile row alone


# ---- 5. the patch forms with lead rows (vh_op_gemm_lead) and the lead-row kernels (vh_op_lead_rows) --------------------------------
LEAD_VARIANTS = (0, 1, 2, 5, 6, 7)                 # what gemm_check accepts for EPI_PATCH / EPI_PATCH_SPLIT: everything but ...
LEAD_REFUSED = {3: "variants 3/4 (BK=32 pipeline) were removed", 4: "variants 3/4 (BK=32 pipeline) were removed", 8: "gemm: variant", -1: "gemm: variant"}


LEAD_FORMS = {"lead1": (False, 1), "lead5": (False, 5), "lead16": (False, 16), "no_cls4": (True, 4)}      # (no class token, lead rows)


def refused(call, text):
    with pytest.raises(vithip.VhError) as e:
        call()
    assert e.value.code == 1 and text in str(e.value), (text, str(e.value))


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("lead", [0, 1, 5, 17])
@pytest.mark.parametrize("epi", X.PATCHES, ids=lambda e: X.ENAME[e])
@pytest.mark.parametrize("name", ["S1", "S1r"])
def test_patch_epilogues_with_lead_rows(name, epi, lead, dt):
    # bit for bit per element: the patch rows on output row img * (np + lead) + lead + p with pos row 1 + p; the lead rows of out and
    # out16, the partial sums of the lead rows and of the 5 padding rows of `partials` keep their canaries; the guard slabs survive
    M, N, K = X.shape(name, False, epi)
    keep = []
    for variant in LEAD_VARIANTS:
        n = 768 if variant == 6 and N % 256 else N      # (test_row_major_16bit_operands' rule)
        case = case_of(M, n, K, False).with_lead(lead, pad_rows=5)
        assert case.np_img < 128 and case.out_rows(epi) == M // case.np_img * (case.np_img + lead)
        before, got = run_and_check(case, epi, dt, variant, lead_tap=True, keep=keep)
    L = keep[-1]
    for variant, text in LEAD_REFUSED.items():
        refused(lambda: L.launch(variant), text)

    def tap(epi=epi, patches=case.np_img, lead=lead, prow=0):      # the last launch's own operands and buffers, one argument changed
        return lambda: vithip.op_gemm_lead(L.a.ptr, L.w_ptr, L.bias.ptr, L.ptr("out"), M, n, K, epi, dt, L.pos.ptr, patches, lead,
                                           out16_ptr=L.ptr("out16"), partials_ptr=L.ptr("partials"), prow=prow, variant=5)

    refused(tap(lead=-1), "gemm: EPI_PATCH* lead rows outside 0..17")
    refused(tap(lead=18), "gemm: EPI_PATCH* lead rows outside 0..17")
    refused(tap(epi=E["BIAS_F32"]), "gemm_lead: epilogue must be VH_EPI_PATCH or VH_EPI_PATCH_SPLIT")
    refused(tap(patches=case.np_img - 1), "gemm_lead: M must be a whole number of images")
    if epi == E["PATCH_SPLIT"]:
        refused(tap(prow=case.out_rows(epi) - 1), "gemm_lead: prow is below images x (aux_i + lead)")
    same_bits(L.read("after the refused calls"), got, "a refused call wrote to its output:")


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("batch", [3, 20])
@pytest.mark.parametrize("form", list(LEAD_FORMS))
def test_lead_rows_kernel_exact(form, batch, dim):
    # the whole assembly once: the patch GEMM through vh_op_gemm_lead (16 patches per image), then vh_op_lead_rows on the buffers it
    # left.  fp32 form (EPI_PATCH): row 0 = cls + pos[0], row 1 + r = reg[r] bit for bit, every patch row untouched.  Split form
    # (EPI_PATCH_SPLIT): planes by split_planes, sums exact, sums of squares within SQ_REL, no patch row's plane or partial sum and
    # nothing beyond batch * tokens rows of `partials` touched.  no_cls4: cls and pos NULL, the 4 lead rows are all registers
    no_cls, lead = LEAD_FORMS[form]
    case = X.Case(batch * 16, dim, 128, False, lead=lead, np_img=16, pad_rows=3)
    T = case.tokens
    for dt in DT:
        for epi in X.PATCHES:
            split = epi == E["PATCH_SPLIT"]
            keep = []
            _, mid = run_and_check(case, epi, dt, 0, lead_tap=True, keep=keep)
            L = keep[0]
            inp = X.lead_rows_inputs(dim, lead, no_cls, dt, split)
            ptr = {k: (dev(v).ptr if v is not None else None) for k, v in inp.items()}
            extra = dict(lo_ptr=L.ptr("out16"), partials_ptr=L.ptr("partials"), prow=case.partial_rows(epi), dtype=dt) if split else {}
            what = f"lead_rows {form} batch {batch} dim {dim} {X.NAME[dt]} {'split' if split else 'fp32'}"
            vithip.op_lead_rows(L.ptr("out"), ptr["cls"], ptr["pos0"], ptr["reg"], lead, batch, T, dim, **extra)
            got = L.read(what)
            X.check_lead_rows(mid, got, inp, batch, T, dt, split, what)
            # the tap's refusals, with the outputs untouched afterwards
            text = "lead_rows: bad argument"
            refused(lambda: vithip.op_lead_rows(L.ptr("out"), ptr["cls"], ptr["pos0"], ptr["reg"], lead, batch, T, dim - 32, **extra), text)     # dim % 64
            refused(lambda: vithip.op_lead_rows(L.ptr("out"), ptr["cls"], ptr["pos0"], ptr["reg"], lead, batch, lead, dim, **extra), text)       # lead >= tokens
            if split:
                small = dict(extra, prow=batch * T - 1)
                refused(lambda: vithip.op_lead_rows(L.ptr("out"), ptr["cls"], ptr["pos0"], ptr["reg"], lead, batch, T, dim, **small),
                        "lead_rows: the split form needs partials, a 16-bit dtype and prow >= batch x tokens")
            same_bits(L.read(what + " after the refused calls"), got, what + ": a refused call wrote to its output:")


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_layout_taps_refuse_what_the_launchers_refuse():
    # (one text since gemm_check states both: the taps print its reason, launch_gemm asks it first, so every caller is refused alike)
    size = 1 << 20
    b = dev(np.full(size, GUARD, np.uint8))
    p = b.ptr

    def g16(M, N, K, epi, variant, ot=0, ab=0, tb=0, tc=0, dt=BF16):
        return lambda: vithip.op_gemm_layout(p, p, p, p, M, N, K, epi, dt, aux_ptr=p, aux_i=64, stats_ptr=p, out16_ptr=p, partials_ptr=p,
                                             variant=variant, out_tiled=ot, ab_tiled=ab, tile_begin=tb, tile_count=tc)

    def g8(M, N, K, epi, variant, ot=0, ab=0, tb=0, tc=0):
        return lambda: vithip.op_gemm_fp8_layout(p, p, p, p, p, M, N, K, epi, c_ptr=p, stats_ptr=p, out16_ptr=p, partials_ptr=p,
                                                 variant=variant, out_tiled=ot, ab_tiled=ab, tile_begin=tb, tile_count=tc)

    bad = [
        g16(256, 256, 256, E["LNFOLD_GELU"], 5, ot=1), g16(256, 256, 256, E["LNFOLD_GELU"], 0, ot=1),      # tiled flags: variant 6 only
        g16(256, 256, 256, E["BIAS"], 7, ab=1),
        g16(264, 256, 256, E["BIAS_GELU"], 6, ot=1), g16(256, 260, 256, E["BIAS_GELU"], 6, ot=1),          # M, N multiples of 256
        g16(256, 256, 64, E["BIAS_GELU"], 6, ot=1), g16(256, 256, 192, E["LNFOLD_GELU"], 6, ot=1),         # K-tiles: 2, LN-fold 4
        g16(256, 256, 192, E["LNFOLD"], 6, ot=1), g16(256, 256, 64, E["RESID_SPLIT"], 6, ab=1),
        g16(256, 256, 256, E["BIAS"], 6, ot=1, ab=1),                                                       # not both
        g16(256, 256, 256, E["BIAS_RESID"], 6, ot=1), g16(256, 256, 256, E["RESID_LN"], 6, ot=1),          # out_tiled: act, LNFOLD, BIAS
        g16(256, 256, 256, E["RESID_SPLIT"], 6, ot=1), g16(256, 256, 256, E["BIAS_F32"], 6, ot=1),
        g16(256, 256, 256, E["LNFOLD"], 6, ab=1), g16(256, 256, 256, E["BIAS_GELU"], 6, ab=1),             # ab_tiled: RESID_SPLIT, BIAS
        g16(256, 256, 256, E["RESID_LN"], 6, ab=1),
        g16(600, 1024, 128, E["BIAS"], 6, tc=5), g16(600, 1024, 128, E["BIAS"], 1, tc=5),                  # ranges: variants 5 and 7
        g16(600, 1024, 128, E["BIAS"], 2, tc=5), g16(600, 1024, 128, E["BIAS"], 0, tc=5),
        g16(600, 1024, 128, E["BIAS"], 5, tb=-1, tc=3), g16(600, 1024, 128, E["BIAS"], 5, tb=8, tc=5),     # begin >= 0, end <= tiles
        g16(600, 1024, 128, E["BIAS"], 7, tb=0, tc=13), g16(600, 1024, 128, E["BIAS"], 5, tb=3, tc=0),     # begin != 0 needs a count
        g16(600, 1024, 128, E["BIAS"], 5, tb=0, tc=-2),
        g16(256, 256, 256, E["BIAS"], 6, ot=1, tc=1),                                                       # a range excludes the layouts
        g16(256, 256, 96, E["BIAS"], 5), g16(256, 258, 128, E["BIAS"], 5), g16(256, 256, 128, 12, 5),      # what vh_op_gemm_ex refuses
        g8(256, 256, 512, E["LNFOLD_GELU"], 5, ot=1), g8(256, 256, 512, E["LNFOLD_GELU"], 0, ot=1),
        g8(256, 256, 512, E["BIAS"], 6, ot=1), g8(256, 256, 512, E["BIAS"], 6, ab=1),                       # e4m3 BIAS has neither layout
        g8(256, 256, 384, E["LNFOLD"], 6, ot=1), g8(256, 256, 128, E["BIAS_GELU"], 6, ot=1),               # K-tiles: LNFOLD 4, others 2
        g8(256, 256, 128, E["RESID_SPLIT"], 6, ab=1), g8(256, 256, 512, E["RESID_LN"], 6, ab=1),
        g8(256, 256, 512, E["LNFOLD"], 6, ab=1), g8(256, 256, 512, E["RESID_SPLIT"], 6, ot=1),
        g8(512, 256, 512, E["LNFOLD_GELU"], 6, ot=1, ab=1), g8(300, 256, 512, E["LNFOLD_GELU"], 6, ot=1),
        # the tanh-GELU codes, wherever an activation code stands above for a tiled flag
        g16(256, 256, 256, E["LNFOLD_TGELU"], 5, ot=1), g16(256, 256, 256, E["LNFOLD_TGELU"], 0, ot=1), g16(256, 256, 256, E["BIAS_TGELU"], 7, ot=1),
        g16(264, 256, 256, E["BIAS_TGELU"], 6, ot=1), g16(256, 260, 256, E["BIAS_TGELU"], 6, ot=1),
        g16(256, 256, 64, E["BIAS_TGELU"], 6, ot=1), g16(256, 256, 192, E["LNFOLD_TGELU"], 6, ot=1),
        g16(256, 256, 256, E["BIAS_TGELU"], 6, ab=1), g16(256, 256, 256, E["LNFOLD_TGELU"], 6, ab=1), g16(256, 256, 256, E["BIAS_TGELU"], 6, ot=1, ab=1),
        g16(256, 256, 256, E["BIAS_TGELU"], 6, ot=1, tc=1),
        g8(256, 256, 512, E["LNFOLD_TGELU"], 5, ot=1), g8(256, 256, 512, E["LNFOLD_TGELU"], 0, ot=1), g8(256, 256, 128, E["BIAS_TGELU"], 6, ot=1),
        g8(256, 256, 128, E["LNFOLD_TGELU"], 6, ot=1), g8(256, 256, 512, E["BIAS_TGELU"], 6, ab=1),
        g8(512, 256, 512, E["LNFOLD_TGELU"], 6, ot=1, ab=1), g8(300, 256, 512, E["LNFOLD_TGELU"], 6, ot=1),
        g8(600, 1024, 256, E["BIAS"], 6, tc=5), g8(600, 1024, 256, E["BIAS"], 0, tc=5), g8(600, 1024, 256, E["BIAS"], 5, tb=8, tc=5),
        g8(600, 1024, 256, E["BIAS"], 7, tb=2, tc=0), g8(600, 1024, 256, E["BIAS"], 5, tb=-1, tc=2),
        g8(256, 256, 192, E["BIAS"], 5), g8(256, 256, 256, E["PATCH"], 5), g8(256, 256, 256, E["BIAS"], 2),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(vithip.VhError) as e:
            call()
        assert e.value.code in (1, 4) and str(e.value), i      # VH_ERR_INVALID (an epilogue the e4m3 form lacks: VH_ERR_UNSUPPORTED), with a message
        assert e.value.code == 1 or i == len(bad) - 2, i
    for call in (lambda: vithip.op_gemm_layout(None, p, p, p, 256, 256, 256, E["BIAS"], BF16, variant=6, ab_tiled=1),
                 lambda: vithip.op_gemm_fp8_layout(p, p, None, p, p, 256, 256, 512, E["BIAS"], variant=5, tile_count=1)):
        with pytest.raises(vithip.VhError) as e:
            call()
        assert e.value.code == 1 and str(e.value)
    assert np.all(b.to_numpy(np.uint8, (size,)) == GUARD), "a refused call wrote to its output"
