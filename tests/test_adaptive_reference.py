"""tests/adaptive_reference.py itself, on the CPU: the rule against exact rational arithmetic, the quantile against the bisection
the library runs, the fp32 image against the oracle — and, for every case tests/test_adaptive_rule.py runs on the GPU, that the
reference leaves no pixel's sample count open and no err_map float in doubt.  That last part is a condition on the cases, not a
tolerance: a case that fails it gets another seed or size, never an exclusion."""
import math
from fractions import Fraction

import adaptive_cases as ac
import adaptive_reference as ar
import mpmath
import numpy as np
import pytest
from conftest import assert_bit_equal, bits

# ---- the rule against exact arithmetic ----------------------------------------------------------------------------------

def _exact_rule(Y, cps, max_spp, E, L, z):
    """One pixel in rationals: (n, half^2, denominator) at the stopping checkpoint; half^2 is None for the +inf of n == 1."""
    for n in cps:
        S1, S2 = sum(Y[:n]), sum(y * y for y in Y[:n])
        den = max(S1 / n, L)
        if n == 1:
            half2, stop = None, False
        else:
            half2 = z * z * max(Fraction(0), (S2 - S1 * S1 / n) / (n - 1)) / n
            stop = half2 == 0 or half2 <= (E * den) ** 2
        if stop or n == max_spp:
            return n, half2, den
    raise AssertionError("no checkpoint at max_spp")


def _dyadic_pixels():
    """[P, 8] luminance, every value k / 64 with small k: sums, squares and the moments' difference are exact in fp64."""
    rng = np.random.default_rng(11)
    named = [[0.5] * 8,                                            # constant: half == 0, stops at the first n > 1
             [0.0] * 8,                                            # all zero: 0 / 0 without the guard at min_luminance = 0
             [1 / 64, 3 / 64, 1 / 64, 0, 2 / 64, 1 / 64, 0, 1 / 64],  # mean far below a min_luminance of 0.5
             [0, 0, 0, 4.0, 0, 0, 0, 0],                           # one lit sample: runs on
             [1.0, 1.25, 0.75, 1.0, 1.0, 1.0, 1.25, 0.75],         # quiet
             [0, 0, 0, 0, 0, 0, 0, 0.015625]]                      # black until the last sample
    return np.concatenate([np.array(named), rng.integers(0, 512, (40, 8)) / 64.0])


@pytest.mark.parametrize("spp,batch,max_spp", [(4, 4, 8), (2, 2, 4), (2, 6, 8), (1, 3, 4), (1, 1, 2), (1, 0, 1), (8, 0, 8)])
@pytest.mark.parametrize("max_error,min_lum", [(0.25, 0.0), (0.25, 0.5), (1.5, 0.0), (0.01, 0.015625), (3.0, 0.5)])
def test_rule_is_exact_arithmetic(spp, batch, max_spp, max_error, min_lum):
    Y = _dyadic_pixels()
    z = ar.quantile(0.05)
    n, err = ar.rule_luminance(Y, spp, batch, max_spp, max_error, min_lum, z)
    cps = ar.checkpoints(spp, batch, max_spp)
    E, L = Fraction(float(np.float32(max_error))), Fraction(float(np.float32(min_lum)))
    for k in range(Y.shape[0]):
        want_n, half2, den = _exact_rule([Fraction(float(y)) for y in Y[k]], cps, max_spp, E, L, Fraction(z))
        assert n[k] == want_n, (k, n[k], want_n)
        if half2 is None:
            assert err[k] == np.inf, k
        elif half2 == 0:
            assert err[k] == 0.0 and not np.signbit(err[k]), k
        else:
            with mpmath.workdps(50):
                want = mpmath.sqrt(mpmath.mpf(half2.numerator) / half2.denominator) / (mpmath.mpf(den.numerator) / den.denominator)
                assert abs(mpmath.mpf(float(err[k])) - want) <= 4 * np.spacing(float(want)), (k, err[k], want)


def test_rule_stops_where_it_should():
    """The named pixels: a constant and an all-zero pixel stop at the first checkpoint with n > 1 with err == +0; at spp = 1 nobody
    stops at n == 1; a mean below min_luminance is divided by min_luminance."""
    Y = _dyadic_pixels()
    z = ar.quantile(0.0)
    n, err = ar.rule_luminance(Y, 1, 3, 8, 0.25, 0.0, z)
    assert list(n[:2]) == [4, 4] and (err[:2] == 0).all() and not np.signbit(err[:2]).any()
    assert (n > 1).all()
    n4, err4 = ar.rule_luminance(Y, 4, 4, 8, 1e-3, 0.5, z)
    s1 = Y[2].sum()
    var = ((Y[2] ** 2).sum() - s1 * s1 / 8) / 7
    assert n4[2] == 8 and err4[2] == z * math.sqrt(var / 8) / 0.5


def test_luminance_is_left_to_right():
    rng = np.random.default_rng(5)
    s = rng.random((64, 3)).astype(np.float32) * np.float32(7.0)
    Y = ar.luminance(s)
    for k in range(s.shape[0]):
        r, g, b = (Fraction(float(v)) for v in s[k])
        t = float(Fraction(0.2126) * r)                  # float(Fraction) rounds to nearest: one fp64 operation each
        t = float(Fraction(t) + Fraction(float(Fraction(0.7152) * g)))
        t = float(Fraction(t) + Fraction(float(Fraction(0.0722) * b)))
        assert Y[k] == t, k


def test_mean_image_is_the_fp32_sum_in_order():
    s = np.array([[[1e8, 1, 0.1], [1, 1e8, 0.2], [-1e8, 3, 0.3]]], np.float32)
    fb = ar.mean_image(s, np.array([3]))
    a = np.float32(0) + s[0, 0]
    a = a + s[0, 1]
    a = a + s[0, 2]
    assert_bit_equal(fb[0], a * (np.float32(1.0) / np.float32(3.0)), "fp32 sum")
    assert fb[0, 0] == 0.0                               # (1e8 + 1) + -1e8 in fp32: the order shows


def test_checkpoints_and_defaults():
    assert ar.checkpoints(4, 4, 32) == [4, 8, 12, 16, 20, 24, 28, 32]
    assert ar.checkpoints(2, 5, 31) == [2, 7, 12, 17, 22, 27, 31]
    assert ar.checkpoints(1, 0, 0) == list(range(1, 33))
    assert ar.checkpoints(3, 0, 7) == [3, 6, 7]
    assert ar.checkpoints(4, 9, 4) == [4]


def test_plan_passes():
    # 1200 pixels, budget of one sample of the full frame: round 0 runs 4 passes; 300 listed pixels run 4 samples in one
    assert ar.plan_passes(4, 4, 12, [1200, 300, 7], 16 * 1200) == 4 + 1 + 1
    assert ar.plan_passes(4, 4, 12, [1200, 601, 7], 16 * 1200) == 4 + 4 + 1
    assert ar.plan_passes(4, 4, 12, [1200, 600, 400], 16 * 1200) == 4 + 2 + 2      # 2 and 3 samples per pass
    assert ar.plan_passes(4, 7, 30, [10, 10, 10, 10, 10], 16) == 4 + 7 + 7 + 7 + 5


# ---- the quantile ---------------------------------------------------------------------------------------------------------

def _bisected(pv):
    """The library's z: 200 bisection steps of erfc(z / sqrt 2) = p over [0, 64]."""
    lo, hi = 0.0, 64.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > pv:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("p_value", ac.P_VALUES)
def test_quantile_brackets_the_bisection(p_value):
    """Why 1e-12: libm's erfc puts the bisection within a few ulp of the true quantile for p up to 0.9 (7e-14 at 0.999, where erfc
    loses relative precision near 1)."""
    pv = 0.05 if p_value == 0 else float(np.float32(p_value))
    z = ar.quantile(p_value)
    assert abs(_bisected(pv) - z) <= ar.Z_BRACKET * z
    assert abs(math.erfc(z / math.sqrt(2.0)) - pv) <= 1e-13 * pv


def test_quantile_takes_the_float_field():
    assert ar.quantile(0.0) == 1.9599639845400543                    # 1.95996398454005423552...
    assert ar.quantile(0.05) != ar.quantile(0.0)                     # float32(0.05) is not the double 0.05
    assert abs(ar.quantile(0.05) / ar.quantile(0.0) - 1.0) < 1e-8


# ---- the image ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["scene1", "cbox"])
def test_fb_is_the_oracle_at_each_pixels_n(oracle, name):
    frame, rule = ac.Frame(name), ac.RULES[0]
    p, E = ac.reference(oracle, frame, rule)
    values, counts = np.unique(E.n, return_counts=True)
    assert len(values) >= 3
    for n in values[np.argsort(-counts)][:4]:
        q = p.copy()
        q.spp, q.stream_stride = int(n), rule.max_spp
        img, _ = oracle.render(ac.scene(name)[1], q)
        assert_bit_equal(E.fb[E.n == n], img.reshape(-1, 3)[E.n == n], f"{name} n = {n}")


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ac.every_case()))
def test_no_pixel_is_undecided(oracle, name):
    frame, rule = ac.every_case()[name]
    p, E = ac.reference(oracle, frame, rule)
    assert E.n.shape == (p.num_rows() * p.width,)
    assert int((~E.decided).sum()) == 0
    assert int((bits(E.err_lo) != bits(E.err_hi)).sum()) == 0
    cps = ar.checkpoints(rule.spp, rule.batch, rule.max_spp)
    assert np.isin(E.n, cps).all() and E.list_sizes[0] == E.n.size and len(E.list_sizes) == E.rounds


@pytest.mark.parametrize("scene", ac.SCENES)
@pytest.mark.parametrize("i", range(len(ac.RULES)))
def test_the_matrix_reaches_several_counts(oracle, scene, i):
    _, E = ac.reference(oracle, ac.Frame(scene), ac.RULES[i])
    assert len(np.unique(E.n)) >= 4, np.unique(E.n)


def test_the_black_scene_has_black_and_half_black_pixels(oracle):
    for frame, rule in ac.BLACK:
        lit = (ac.frame_samples(oracle, frame, rule.max_spp) != 0).any(axis=2)
        black = (~lit).all(axis=1)
        assert int(black.sum()) >= 100
        assert int((lit.any(axis=1) & ~lit.all(axis=1)).sum()) >= 100
        _, E = ac.reference(oracle, frame, rule)
        first = [c for c in ar.checkpoints(rule.spp, rule.batch, rule.max_spp) if c > 1][0]
        assert (E.n[black] == first).all() and (bits(E.err_lo[black]) == 0).all()


def test_the_edge_cases_are_edges(oracle):
    _, E = ac.reference(oracle, *ac.ALL_STOP)
    assert E.rounds == 1 and (E.n == ac.ALL_STOP[1].spp).all()
    frame, rule = ac.NONE_STOP
    _, E = ac.reference(oracle, frame, rule)
    s = ac.frame_samples(oracle, frame, rule.max_spp)
    flat = (ar.luminance(s)[:, :rule.spp] == ar.luminance(s)[:, :1]).all(axis=1)
    assert (E.n[flat] == rule.spp).all()
    # only a variance that comes out as exactly zero stops a pixel (a nearly constant one's can, at a later checkpoint too)
    assert ((E.n < rule.max_spp) == (E.err == 0)).all()
    assert 50 <= (E.n < rule.max_spp).sum() <= E.n.size - 50
    assert ((E.err_lo > np.float32(rule.max_error)) == (E.n == rule.max_spp)).all()


@pytest.mark.parametrize("k", ac.LIST_SIZES)
def test_list_size_cases_continue_exactly_k(oracle, k):
    rule = ac.list_case(oracle, k)
    assert rule is not None, "the ranks tie: another scene, size or seed"
    _, E = ac.reference(oracle, ac.LIST_FRAME, rule)
    assert int((~E.decided).sum()) == 0 and int((bits(E.err_lo) != bits(E.err_hi)).sum()) == 0
    assert int((E.n > rule.spp).sum()) == k
    assert (E.list_sizes[1] if k else E.rounds) == (k if k else 1)


def test_pass_plans_differ_by_round(oracle):
    frame, rule = ac.PASSES
    npix = frame.w * frame.h
    _, E = ac.reference(oracle, frame, rule, scratch_bytes=16 * npix)
    assert E.rounds >= 3 and E.passes > E.rounds                       # round 0 runs sample by sample
    assert E.passes < rule.max_spp                                     # later rounds run more per pass as the list shrinks
    _, E1 = ac.reference(oracle, frame, rule, scratch_bytes=16)
    assert E1.passes == ar.checkpoints(*rule[:3])[E1.rounds - 1]        # one sample per pass everywhere
