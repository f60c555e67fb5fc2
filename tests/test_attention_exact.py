"""CPU self-test of tests/attn_exact.py: the proof that the assertions of test_gpu_attention_exact.py can fail, and the guard of
the generators.  A numpy emulation of the kernels' arithmetic (fp32, P rounded to 16 bit, the wave-wide deferred rescale) passes
every design; three mutants of it -- one key too many, one too few, V read from the neighbouring head -- fail the same
assertions.

Which (mutant, design) pairs can fail is decided by the mathematics, not by what the emulation happens to give:
  * extra_key at T = 1 is the identity in every design (softmax over two copies of the only key), so it is asserted to be
    bit-identical there instead;
  * extra_key in the permutation design is the identity as well (the replica of key T-1 either shares the matched V row or
    stays below 2^-32): masks are pinned by the uniform and graded designs, the permutation design pins the rescale;
  * every other pair must fail at every shape.
"""
import numpy as np
import pytest

import attn_exact as X
import vithip

TOKENS = [1, 31, 32, 33, 197, 1025]
HEAD_DIMS = [32, 64, 80, 128]
DT = [X.BF16, X.FP16]
MUTANTS = ["extra_key", "drop_last", "swap_heads"]


def _shape(tokens):
    return (1, 2) if tokens > 640 else (2, 2)   # (batch, heads): two heads so that swap_heads has a neighbour


_CASES = {}


def case_and_ref(design, tokens, hd, dt):
    """Generated once per shape and shared, unchanged, by the tests (the integer designs do not depend on the type)."""
    key = (design, tokens, hd, dt if design == "permutation" else None)
    if key not in _CASES:
        batch, heads = _shape(tokens)
        case = X.make_case(design, batch, tokens, heads, hd, seed=7, vdtype=dt)
        _CASES[key] = (case, X.reference(case))
        _CASES[key][0].qkv.setflags(write=False)
        _CASES[key][1].setflags(write=False)
    return _CASES[key]


def check(case, ref, got, dt):
    if case.design == "permutation":
        X.assert_bits(X.to_bits(got, dt), X.to_bits(case.expected_permutation(), dt), case, dt, "emulation")
    X.assert_elements(got, ref, dt, case, "emulation", vmax=X.VMAX)


@pytest.mark.parametrize("dt", DT, ids=lambda d: X.NAME[d])
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("tokens", TOKENS)
def test_emulation_passes_every_design_and_every_mutant_fails(tokens, hd, dt):
    for design in X.DESIGNS:
        case, ref = case_and_ref(design, tokens, hd, dt)
        got, stats = X.emulate(case, dt)
        check(case, ref, got, dt)
        nblk = (tokens + 31) // 32
        if design == "graded":
            assert stats["pmax"] <= 2.0 ** 8
            if tokens >= 197:
                assert stats["rescales"] >= 1 and stats["pmax"] == 2.0 ** 8, stats["rescales"]
                # the capped blocks (every third) never rescale: they carry p = 2^8 under the stale shift to the end
                assert all(not any(blk % 3 == 0 for blk in hit) for hit in stats["blocks"].values())
        if design == "permutation" and tokens >= 197:
            for bh, hit in stats["blocks"].items():   # a rescale in EVERY 32-row block of every (image, head)
                assert hit == set(range(nblk)), (bh, sorted(set(range(nblk)) - hit))
        for mutant in MUTANTS:
            mut, _ = X.emulate(case, dt, mutant)
            if mutant == "extra_key" and (tokens == 1 or design == "permutation"):
                assert np.array_equal(mut, got)   # the identity (module docstring)
                continue
            with pytest.raises(AssertionError):
                check(case, ref, mut, dt)


@pytest.mark.parametrize("design", ["graded", "permutation"])
def test_emulation_e4m3_output(design):
    # bf16 operands, e4m3 result: the permutation design returns e4m3-representable V rows byte for byte, the graded design
    # stays inside half an e4m3 step; the mutants fail here too
    case = X.make_case(design, 2, 197, 2, 64, seed=9, vdtype=X.FP8)
    ref = X.reference(case)
    got, _ = X.emulate(case, X.FP8)
    if design == "permutation":
        X.assert_bits(X.to_bits(got, X.FP8), X.to_bits(case.expected_permutation(), X.FP8), case, X.FP8)
    X.assert_elements(got, ref, X.FP8, case)
    for mutant in ("drop_last", "swap_heads"):
        mut, _ = X.emulate(case, X.FP8, mutant)
        with pytest.raises(AssertionError):
            if design == "permutation":
                X.assert_bits(X.to_bits(mut, X.FP8), X.to_bits(case.expected_permutation(), X.FP8), case, X.FP8)
            X.assert_elements(mut, ref, X.FP8, case)


def test_generators_hold_what_the_designs_promise():
    for hd in HEAD_DIMS:
        for dt in DT:
            for design in X.DESIGNS:
                case = X.make_case(design, 2, 197, 3, hd, seed=3, vdtype=dt)
                D, T = case.dim, case.tokens
                # exact in both 16-bit types
                for t in DT:
                    if design != "permutation" or t == dt:
                        assert np.array_equal(vithip.from16(vithip.to16(case.qkv, t), t), case.qkv)
                q, k = case.qkv[:, :D].astype(np.float64), case.qkv[:, D:2 * D].astype(np.float64)
                cols = [tuple(np.nonzero(np.abs(k[:, h * hd:(h + 1) * hd]).sum(0))[0]) for h in range(3)]
                if design != "uniform":
                    assert len(set(cols)) == 3, "active columns must differ per head"
                for b in range(2):
                    for h in range(3):
                        s = q[b * T:(b + 1) * T, h * hd:(h + 1) * hd] @ k[b * T:(b + 1) * T, h * hd:(h + 1) * hd].T
                        v = case.v_of(b, h)
                        if design == "uniform":
                            assert not s.any() and np.all(np.abs(v[T - 1]) == 8) and np.array_equal(v[0], -v[T - 1])
                        elif design == "graded":
                            assert not s[:, :32].any() and s.min() >= -4 and s.max() == 10
                            assert np.abs(v).max() <= 8
                        else:
                            assert np.array_equal(s.argmax(1), case.pi[b, h]) and np.all(s.max(1) == 208)
                            part = np.sort(s, axis=1)
                            assert np.all(part[:, -1] - part[:, -2] >= 32)
                            assert sorted(case.pi[b, h]) == list(range(T))
                            assert np.abs(v).min() >= 0.25 and np.abs(v).max() < 8
                if design != "uniform":
                    assert not np.array_equal(case.v_of(0, 0), case.v_of(1, 0)) and not np.array_equal(case.v_of(0, 0), case.v_of(0, 1))


def test_assertion_helpers_name_the_element():
    case = X.make_case("uniform", 2, 33, 2, 64, seed=1)
    ref = X.reference(case)
    got = ref.copy()
    got[33 + 5, 64 + 7] += 0.01
    with pytest.raises(AssertionError, match=r"image 1 head 1 row 5 column 7 \(T = 33"):
        X.assert_elements(got, ref, X.FP16, case)
    got = ref.copy()
    got[2, 3] = np.nan   # an unwritten (0xFF-filled) element
    with pytest.raises(AssertionError, match=r"not finite.*image 0 head 0 row 2 column 3"):
        X.assert_elements(got, ref, X.FP16, case)
    bits = vithip.to16(ref.astype(np.float32), X.FP16)
    other = bits.copy()
    other[40, 100] ^= 1
    with pytest.raises(AssertionError, match=r"image 1 head 1 row 7 column 36"):
        X.assert_bits(other, bits, case, X.FP16)
    # the bound itself: one 16-bit rounding step passes, two do not
    one = np.full((1, 1), 3.0)
    c1 = X.Case("uniform", None, 1, 1, 1, 64)
    X.assert_elements(one * (1 + 2.0 ** -11), one, X.FP16, c1)
    with pytest.raises(AssertionError):
        X.assert_elements(one * (1 + 2.0 ** -10), one, X.FP16, c1)
    X.assert_elements(one * (1 + 2.0 ** -4), one, X.FP8, c1)
    with pytest.raises(AssertionError):
        X.assert_elements(one * (1 + 2.0 ** -3), one, X.FP8, c1)


def test_layout_helpers_round_trip():
    r = np.random.default_rng(5)
    for rows, heads, hm_rows in ((197 * 4, 2, 197 * 4), (200 * 3, 4, 768), (33, 1, 48)):
        D = heads * 64
        qkv = r.integers(0, 65536, size=(rows, 3 * D)).astype(np.uint16)
        hm = vithip.pack_head_major(qkv, heads, hm_rows, fill=0xFFFF)
        assert hm.shape == (3, heads, hm_rows, 64)
        for part in range(3):
            for h in range(heads):
                assert np.array_equal(hm[part, h, :rows], qkv[:, part * D + h * 64:part * D + (h + 1) * 64])
                assert np.all(hm[part, h, rows:] == 0xFFFF)
        # the kernel's address arithmetic (kernels_attn.hip): element (part, h, row, c) at ((part * heads + h) * hm_rows + row) * 64 + c
        flat = hm.reshape(-1)
        assert flat[((2 * heads + heads - 1) * hm_rows + 5) * 64 + 9] == qkv[5, 2 * D + (heads - 1) * 64 + 9]
    for rows, dim, chunk, dtype in ((788, 128, 8, np.uint16), (600, 256, 8, np.uint16), (788, 128, 16, np.uint8), (17, 64, 16, np.uint8)):
        a = r.integers(0, 250, size=(rows, dim)).astype(dtype)
        t = vithip.pack_tiled(a, chunk, fill=0xFF)
        nb = (rows + 15) // 16
        assert t.shape == (nb, dim // chunk, 16, chunk)
        assert np.array_equal(vithip.unpack_tiled(t, rows, dim, chunk), a)
        # the kernel's store address: row m, chunk c at ((m >> 4) * (dim / chunk) + c) * 16 * chunk + (m & 15) * chunk
        flat = t.reshape(-1)
        m, c = rows - 1, dim // chunk - 1
        assert np.array_equal(flat[((m >> 4) * (dim // chunk) + c) * 16 * chunk + (m & 15) * chunk:][:chunk], a[m, c * chunk:(c + 1) * chunk])
        full = vithip.unpack_tiled(t, nb * 16, dim, chunk)
        assert np.all(full[rows:] == 0xFF)   # the padding rows of the last block
