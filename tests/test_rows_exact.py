"""CPU self-test of tests/rows_exact.py: the proof that the assertions of test_gpu_rows_exact.py can fail, and the guard of the
generators.  The numpy emulation of the row kernels (fp32, in the kernels' chunk and butterfly order) passes every check at
every shape the GPU file runs -- the sweeps are the same functions -- which also proves that the closed forms of the designs
(mean = m, rstd = 1 / a, y = +-gamma + beta, ...) are what fp32 arithmetic in that order gives.  Every named mutant of the
emulation fails the checks it is meant for.

Which (mutant, shape) pairs can fail is decided by the mathematics, not by what the emulation happens to give; where a mutant is
the identity, the test asserts identical bits instead:
  * ch_small and gamma_by_lane at dim <= 256 (one chunk per lane: there is no smaller class, and lane = lane + 64 i);
  * no_eps on rows without a constant row (eps = 2^-40 is absorbed by a^2 anyway); eps_on_sigma in the LayerNorm's RESULT on
    tiny-eps rows (1 / (a + 2^-40) = 1 / a, and a constant row is beta under any rstd) -- the statistics and the big-eps rows pin it;
  * lo_scale_other on the e4m3 form (its lo plane is bf16, no scale); in layernorm_split the mixed planes pin the scale (form a
    stays two-level under any power-of-two lo scale);
  * guard_miss_last when the maximal row stands first; garbage_blocks at nblk = 16 and 32 (no missing block);
  * head_no_batch_clamp everywhere (an image column of the MFMA never reaches another image's logits: the clamp only keeps the
    loads inside the buffer), head_image_wrap up to 16 images, head_drop_class_tail at classes % 64 == 0;
  * c_unrounded on the integer rows (nothing is rounded).
"""
import numpy as np
import pytest

import rows_exact as X
import vithip

EMU = X.Emulation()
MUT_DIMS = [60, 260, 772, 1284, 2048]
MUT_ROWS = [3, 7]


def fails(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def identical(mutant, fn, *args, **kw):
    """The mutant passes and returns the bits of the emulation as written."""
    a, b = X.Recorder(EMU), X.Recorder(X.Emulation(mutant))
    fn(a, *args, **kw)
    fn(b, *args, **kw)
    assert a.log and a.same_as(b), (mutant, fn.__name__, args)


# ---- the emulation passes every check at every shape of the GPU file -------------------------------------------------------
@pytest.mark.parametrize("dim", X.DIMS)
def test_emulation_passes_layernorm(dim):
    X.sweep_layernorm(EMU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_emulation_passes_rowstats(dim):
    X.sweep_rowstats(EMU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_emulation_passes_pre_layernorm(dim):
    for dt, c, res in X.sweep_pre_ln(EMU, dim):
        # what the GPU file asserts between two kernels holds between the two emulations
        again = EMU.rowstats(X.from_bits(res["y32"], X.F32), c.eps, dt, True)
        X.assert_bits(X.to_bits(res["stats"], X.F32), X.to_bits(again["stats"], X.F32), "pre_layernorm stats = rowstats(y32)", dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_emulation_passes_layernorm_split(dim):
    X.sweep_ln_split(EMU, dim)


@pytest.mark.parametrize("nblk", X.NBLK)
def test_emulation_passes_finalize_stats(nblk):
    X.sweep_finalize(EMU, nblk)


def test_emulation_passes_ln_guard():
    X.sweep_ln_guard(EMU)


@pytest.mark.parametrize("dim", X.HEAD_DIMS)
def test_emulation_passes_head(dim):
    X.sweep_head(EMU, dim)


@pytest.mark.parametrize("dim", X.DIMS)
def test_emulation_passes_fold(dim):
    X.sweep_fold(EMU, dim)


def test_designs_cover_what_they_claim():
    assert [X.ch_class(d) for d in (256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 1284, 2048)] == [1, 2, 2, 3, 3, 4, 4, 5, 5, 8, 8]
    c = X.two_level(7, 260, 0)
    assert abs(c.m[0]) == 4096 and c.a[0] == 0.25 and (c.a == 0).any() and np.all(c.sign.reshape(7, -1, 4).sum(2) == 0)
    assert len({(g, b) for g, b in zip(c.gamma, c.beta)}) == 16
    for dt in (X.BF16, X.FP16, X.FP8, X.F32):   # +-gamma + beta is exact in every result type
        assert np.array_equal(X.from_bits(X.to_bits(c.y, dt), dt), c.y)
    for dt in (X.BF16, X.FP16):
        r = X.residue_rows(3, 64, dt, 0)
        assert not np.any(np.log2(np.abs(vithip.from16(r.hi, dt)[1:])) % 1 == 0)     # h is no power of two
        s = 2.0 ** (-9 if dt == X.BF16 else -12)      # the fold design's edges round as its comments say
        edges = np.array([1 + s, 1 + 2 * s, -(1 + 3 * s), -(1 + 6 * s)], dtype=np.float32)
        assert list(X.from_bits(X.to_bits(edges, dt), dt)) == [1.0, 1.0, -(1 + 4 * s), -(1 + 8 * s)]
        f = X.fold_case(5, 772, dt, 0, True)
        assert np.all(f.c_unrounded - f.c.astype(np.float64) > 100 * 2.0 ** (-9 if dt == X.BF16 else -12))
    p = X.partials_rows(17, 65, 0, "last")
    assert np.sqrt(p.part[:, p.p, 1].max()) % 1 == 0 and len(set(p.part[:, 3, 0])) > 1
    assert X.PRESETS[1] < X.word_of(1.0) < X.PRESETS[2] < X.INF_BITS < X.PRESETS[3]


def test_refusals_need_no_device():
    """Every refusal of the row taps is decided on the host: VH_ERR_INVALID with pointers that are never followed."""
    calls = X.refusal_calls(0x10000, 0x20000)
    assert len(calls) > 120
    for label, call in calls:
        assert call() == 1, label


# ---- the mutants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", MUT_DIMS)
def test_register_kernel_mutants(dim):
    for rows in MUT_ROWS:
        for dt in X.ALL_DT:
            for m in ("one_pass", "drop_last_chunk"):
                fails(X.check_layernorm, X.Emulation(m), rows, dim, dt)
            for m in ("ch_small", "gamma_by_lane"):
                if dim > 256:
                    fails(X.check_layernorm, X.Emulation(m), rows, dim, dt)
                    fails(X.check_layernorm, X.Emulation(m), rows, dim, dt, "bigeps")
                else:
                    identical(m, X.check_layernorm, rows, dim, dt)
            fails(X.check_layernorm, X.Emulation("no_eps"), rows, dim, dt)            # rows >= 3 hold a constant row: NaN
            identical("no_eps", X.check_layernorm, 2, dim, dt)
            for m in ("no_eps", "eps_on_sigma"):
                fails(X.check_layernorm, X.Emulation(m), rows, dim, dt, "bigeps")
            identical("eps_on_sigma", X.check_layernorm, rows, dim, dt)
        for dt in X.PLANE_DT:
            for m in ("one_pass", "drop_last_chunk", "no_eps", "eps_on_sigma") + (("ch_small",) if dim > 256 else ()):
                for split in (False, True):
                    fails(X.check_rowstats, X.Emulation(m), rows, dim, dt, split)
                fails(X.check_pre_ln_uniform, X.Emulation(m), rows, dim, dt, "ratio")
                if m != "eps_on_sigma":
                    fails(X.check_pre_ln_coded, X.Emulation(m), rows, dim, dt, ("y32", "hi", "lo", "stats"))
            fails(X.check_pre_ln_coded, X.Emulation("eps_on_sigma"), rows, dim, dt, ("y32",), "bigeps")
            if dim > 256:
                fails(X.check_pre_ln_coded, X.Emulation("gamma_by_lane"), rows, dim, dt, ("y32", "hi", "lo", "stats"))
            else:
                identical("ch_small", X.check_rowstats, rows, dim, dt, True)
                identical("gamma_by_lane", X.check_pre_ln_coded, rows, dim, dt, ("y32", "hi", "lo", "stats"))
            for form in "abc":
                fails(X.check_ln_split, X.Emulation("drop_last_chunk"), rows, dim, dt, form)


@pytest.mark.parametrize("dim", MUT_DIMS)
def test_lo_scale_mutant(dim):
    for rows in MUT_ROWS:
        for dt in (X.BF16, X.FP16):
            m = X.Emulation("lo_scale_other")
            fails(X.check_rowstats_residue, m, rows, dim, dt)
            fails(X.check_rowstats, m, rows, dim, dt, True)
            fails(X.check_ln_split, m, rows, dim, dt, "c")     # (form a is two-level under any lo scale: LayerNorm is scale-free)
        identical("lo_scale_other", X.check_rowstats, rows, dim, X.FP8, True)
        identical("lo_scale_other", X.check_ln_split, rows, dim, X.FP8, "a")
        identical("lo_scale_other", X.check_pre_ln_coded, rows, dim, X.FP8, ("y32", "hi", "lo", "stats"))


@pytest.mark.parametrize("dim", [60, 1284])
def test_guard_mutants_in_the_row_kernels(dim):
    for rows in (4, 7):
        for m in ("guard_incl_pad", "guard_store"):
            for split in (False, True):
                fails(X.check_rowstats, X.Emulation(m), rows, dim, X.FP8, split)
            for dt in X.PLANE_DT:
                for design in ("ratio", "ratio_pad"):
                    fails(X.check_pre_ln_uniform, X.Emulation(m), rows, dim, dt, design)
            for design in ("amax", "amax_pad"):
                fails(X.check_pre_ln_uniform, X.Emulation(m), rows, dim, X.FP8, design)
        fails(X.check_rowstats, X.Emulation("guard_miss_last"), rows, dim, X.FP8, True, "last")
        identical("guard_miss_last", X.check_rowstats, rows, dim, X.FP8, True, "first")
        for dt in X.PLANE_DT:
            fails(X.check_pre_ln_uniform, X.Emulation("guard_miss_last"), rows, dim, dt, "ratio", "last")
            identical("guard_miss_last", X.check_pre_ln_uniform, rows, dim, dt, "ratio", "first")
            fails(X.check_pre_ln_nan_row, X.Emulation("guard_miss_last"), rows, dim, dt, "last")
        fails(X.check_pre_ln_uniform, X.Emulation("guard_miss_last"), rows, dim, X.FP8, "amax", "last")
        # 16-bit forms carry no |x| word: the three guard mutants are the identity there
        identical("guard_incl_pad", X.check_rowstats, rows, dim, X.BF16, True)


@pytest.mark.parametrize("nblk", X.NBLK)
def test_finalize_and_ln_guard_mutants(nblk):
    for rows in (1, 65, 257):
        for m in ("guard_incl_pad", "guard_store"):
            fails(X.check_finalize, X.Emulation(m), nblk, rows)
        fails(X.check_finalize, X.Emulation("guard_miss_last"), nblk, rows, "last")
        if rows > 1:
            identical("guard_miss_last", X.check_finalize, nblk, rows, "first")
        if nblk % 16:
            fails(X.check_finalize, X.Emulation("garbage_blocks"), nblk, rows)
        else:
            identical("garbage_blocks", X.check_finalize, nblk, rows)
        for m in ("guard_incl_pad", "guard_store"):
            fails(X.check_ln_guard, X.Emulation(m), rows)
        fails(X.check_ln_guard, X.Emulation("guard_miss_last"), rows, "last")
        if rows > 1:
            identical("guard_miss_last", X.check_ln_guard, rows, "first")


@pytest.mark.parametrize("dim", [16, 192])
def test_head_mutants(dim):
    for batch in X.HEAD_BATCH:
        for classes in X.HEAD_CLASSES:
            identical("head_no_batch_clamp", X.check_head, batch, classes, dim)
            if batch > 16:
                fails(X.check_head, X.Emulation("head_image_wrap"), batch, classes, dim)
                fails(X.check_head_random, X.Emulation("head_image_wrap"), batch, classes, dim)
            else:
                identical("head_image_wrap", X.check_head, batch, classes, dim)
            if classes % 64:
                fails(X.check_head, X.Emulation("head_drop_class_tail"), batch, classes, dim)
                fails(X.check_head_random, X.Emulation("head_drop_class_tail"), batch, classes, dim)
            else:
                identical("head_drop_class_tail", X.check_head, batch, classes, dim)


@pytest.mark.parametrize("dim", [60, 772, 2048])
def test_fold_mutant(dim):
    for rows in (1, 5, 70):
        for dt in (X.BF16, X.FP16):
            fails(X.check_fold, X.Emulation("c_unrounded"), rows, dim, dt, True)
            identical("c_unrounded", X.check_fold, rows, dim, dt, False)
        if rows > 1:
            fails(X.check_f8, X.Emulation("c_unrounded"), rows, dim)


def test_every_named_mutant_is_exercised():
    src = open(__file__).read()
    for m in X.MUTANTS:
        assert f'"{m}"' in src, m
