"""tests/observe_truth.py without a GPU: the extended-precision response against 50 digits; the fp64 restatement inside its own
allowance on every hostile case, d_ref taken from another seed (the condition tests/test_gpu_observe_truth.py rests on); and three
deliberately wrong restatements that the judge must reject although each passes the benign case at the existing FLUX_TOL — an erf
difference in the tails, a window of 7.9 sigma, end weights taken as full spacings, and three wrong memberships (lo < x < hi, one
point more and one point less at either end of a window).  The same for the adjoint.  U here is scipy's:
measured on scipy.special.erf / erfc by the procedure the GPU test applies to the device's."""
import functools

import mpmath
import numpy as np
import pytest
from scipy.special import erf, erfc

import observe_adjoint_reference as aref
import observe_reference as oref
import observe_tangent_reference as tref
import observe_truth as OT
from observe_reference import FLUX_TOL

OTHER_SEED = 1


@functools.lru_cache(maxsize=None)
def scipy_U():
    p = OT.ulp_arguments()[0]
    worst, where = OT.ulp_figure(p, erfc(p), erf(p))
    print(f"scipy erf / erfc: worst {worst:.2f} x 2^-53 |value| at {where}; U = {OT.chosen_U(worst)}")
    return OT.chosen_U(worst)


@functools.lru_cache(maxsize=None)
def restated(name, seed=0):
    lam, f, g, edges, sigma, D = OT.hostile(name, seed)
    return oref.observe(lam, f, edges, sigma, D, reference=g)


@functools.lru_cache(maxsize=None)
def d_ref(name, seed=0):
    t = OT.case_truth(name, seed)
    return float(np.max(OT.distance(restated(name, seed), t.out, t.A)))


# ---- 1: the truth's response against 50 digits ---------------------------------------------------------------------------------------------
def response_points():
    """observe_tangent_reference.response_grad_points() extended to widths 1e-6 and 1e4 and to tails of +-8.5"""
    a, b = tref.response_grad_points()
    t = np.r_[np.linspace(-8.0, 8.0, 65), -8.5, -8.25, 8.25, 8.5]
    more_a, more_b = [], []
    for width in (1e-6, 1e-4, 1.0, 1e4):
        more_a += [t, t - width]
        more_b += [t + width, t]
    return np.r_[a, np.concatenate(more_a)], np.r_[b, np.concatenate(more_b)]


def test_extended_response_against_50_digits():
    a, b = response_points()
    worst = 0.0
    with mpmath.workdps(50):
        for x, y in zip(a, b):
            exact = tref.mp_response(x, y)[0]
            got = OT.mp_response(x, y, 0.0, 1.0)[0]
            assert exact > 0
            worst = max(worst, float(abs(mpmath.mpf(got) - exact) / exact))
    print(f"{a.size} points: worst relative distance of the {OT.DPS}-digit response from 50 digits {worst:.3e}")
    assert a.size > 1400 and worst <= 1e-17


def test_the_procedure_that_measures_U_sees_a_wrong_function():
    p = OT.ulp_arguments()[0]
    assert p[0] == 0.0 and p[-1] == 8.5 and p.size == 545 and np.all(np.diff(p) > 0)
    honest = OT.ulp_figure(p, erfc(p), erf(p))[0]
    off = OT.ulp_figure(p, erfc(p) * (1 + 100 * OT.EPS), erf(p))[0]
    print(f"scipy {honest:.2f}, erfc off by 100 units {off:.2f}")
    assert honest < 64 and 60 < off < 200 and OT.chosen_U(3.2) == 5 and OT.chosen_U(4.0) == 5


# ---- 2: the restatement inside its own allowance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OT.CASES)
def test_restatement_meets_its_own_allowance(name):
    t = OT.case_truth(name)
    assert t.n_window.min() >= 1 and len(t.out) == OT.PER_CLASS and np.all(np.isfinite(t.ratio)) and np.all(t.ratio > 0)
    OT.judge(name, "out", restated(name), t.out, t.A, t.ratio, t.T, restated(name), scipy_U(), label="restatement", record=None, d_ref=d_ref(name, OTHER_SEED))


def test_the_classes_are_what_they_say():
    lam, f, _, edges, sigma, D = OT.hostile("spacing")
    assert np.array_equal(oref.window_lengths(lam, edges, sigma, D), OT.SPACING_COUNTS)
    assert set(OT.case_truth("spacing").rows.lanes.tolist()) == {8, 64}
    lam, f, _, edges, sigma, D = OT.hostile("spacing_ends")
    lo, hi = edges[:-1] - 8 * sigma, edges[1:] + 8 * sigma
    assert lo.min() == lam[0] and hi.max() == lam[-1]  # a window reaches either end of the grid
    for name, ratio in (("narrow_1e-6", 1e-6), ("wide_1e4", 1e4)):
        _, _, _, edges, sigma, _ = OT.hostile(name)
        assert np.isclose(np.diff(edges).min() / sigma[0] if ratio < 1 else np.diff(edges).max() / sigma[0], ratio, rtol=1e-3)
    up, down = OT.hostile("range_up+ref"), OT.hostile("range_down+ref")
    assert np.abs(up[1]).min() > 1e149 and np.abs(down[1]).max() < 1e-149 and up[2].max() < 1e-149
    for name in ("far_912_blue30000", "far_1e5_red30000"):
        lam, _, _, edges, _, D = OT.hostile(name)
        assert abs(D - oref.doppler_factor(-30000.0 if "blue" in name else 30000.0)) == 0 and abs(edges[8] / (912.0 if "912" in name else 1e5) - 1) < 1e-3


# ---- 3: mutants ----------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("erf difference in the tails", "window of 7.9 sigma", "end weights as full spacings", "membership lo < x < hi", "window one point wider",
           "window one point narrower")


def mutant_rows(kind, lam, edges, sigma, D):
    """observe_adjoint_reference.pixel_rows with one thing wrong -> [(j, slice, w)]"""
    x = lam * D
    h = oref.trapezoid_weights(x)
    if kind == MUTANTS[2]:
        h[0], h[-1] = x[1] - x[0], x[-1] - x[-2]
    reach = 7.9 if kind == MUTANTS[1] else 8
    out = []
    for j in range(sigma.size):
        strict = kind == MUTANTS[3]
        i0 = int(np.searchsorted(x, edges[j] - reach * sigma[j], "right" if strict else "left"))
        i1 = int(np.searchsorted(x, edges[j + 1] + reach * sigma[j], "left" if strict else "right"))
        grow = {MUTANTS[4]: 1, MUTANTS[5]: -1}.get(kind, 0)
        sl = slice(max(i0 - grow, 0), min(i1 + grow, x.size))
        if kind == MUTANTS[0]:
            s2 = sigma[j] * np.sqrt(2.0)
            r = 0.5 * (erf((edges[j + 1] - x[sl]) / s2) - erf((edges[j] - x[sl]) / s2))
        else:
            r = oref.response(edges[j], edges[j + 1], x[sl], sigma[j])
        out.append((j, sl, r * h[sl]))
    return out


def mutant_observe(kind, name, seed=0):
    lam, f, g, edges, sigma, D = OT.hostile(name, seed)
    out = np.empty(sigma.size)
    for j, sl, w in mutant_rows(kind, lam, edges, sigma, D):
        out[j] = (w * f[sl]).sum() / (w.sum() if g is None else (w * g[sl]).sum())
    return out


def mutant_adjoint(kind, name, c_kind, seed=0):
    """observe_adjoint_reference.adjoint over the mutant's rows -> (w_flux, w_ref or None)"""
    lam, f, g, edges, sigma, D = OT.hostile(name, seed)
    c = OT.pixel_vector(name, c_kind, seed)
    w_flux, w_ref = np.zeros(lam.size), None if g is None else np.zeros(lam.size)
    for j, sl, w in mutant_rows(kind, lam, edges, sigma, D):
        den = w.sum() if g is None else (w * g[sl]).sum()
        w_flux[sl] += w * (c[j] / den)
        if g is not None:
            w_ref[sl] += w * (-((w * f[sl]).sum() / den) * (c[j] / den))
    return w_flux, w_ref


REJECTED_IN = {MUTANTS[0]: ("tail_spike", "tail_spike+ref", "deep_core", "deep_core+ref"), MUTANTS[1]: ("tail_spike", "tail_spike+ref"),
               MUTANTS[2]: ("spacing_ends", "spacing_ends+ref"), MUTANTS[3]: ("on_edge", "on_edge+ref"), MUTANTS[4]: ("on_edge", "on_edge+ref"),
               MUTANTS[5]: ("on_edge", "on_edge+ref")}


@pytest.mark.parametrize("kind", MUTANTS)
def test_the_judge_rejects_a_wrong_restatement(kind):
    for name in ("benign", "benign+ref"):  # the present suite's spectrum and tolerance would not have seen it
        got, ref = mutant_observe(kind, name), restated(name)
        err = float(np.max(np.abs(got - ref) / np.abs(ref)))
        print(f"{kind}, {name}: max |mutant - restatement| / |restatement| = {err:.3e} (FLUX_TOL {FLUX_TOL:g})")
        assert err <= FLUX_TOL
    for name in REJECTED_IN[kind]:
        t = OT.case_truth(name)
        d = OT.distance(mutant_observe(kind, name), t.out, t.A)
        allow = OT.allowance(d_ref(name), t.ratio, t.T, scipy_U())
        print(f"{kind}, {name}: worst mutant distance / allowance {float(np.max(d / allow)):.3e}; the restatement's {d_ref(name) / float(allow.min()):.3e}")
        assert not OT.within(mutant_observe(kind, name), t.out, t.A, t.ratio, t.T, d_ref(name), scipy_U())
        assert OT.within(restated(name), t.out, t.A, t.ratio, t.T, d_ref(name), scipy_U())


# ---- 4: the adjoint ------------------------------------------------------------------------------------------------------------------------
ADJOINT_CASES = [(b + "+ref", OT.adjoint_kind(b + "+ref"), bool(i % 2)) for i, b in enumerate(OT.BASES)] + [
    ("benign", "signed", True), ("tail_spike", "far_tail", False), ("narrow_1e-4_spike", "range", False), ("spacing_ends", "far_tail", True)]


def adjoint_quantities(t):
    q = [("w_flux", t.w_flux, t.scale, t.ratio, t.T)]
    return q + ([("w_reference", t.w_ref, t.scale_ref, t.ratio_ref, t.T_ref)] if hasattr(t, "w_ref") else [])


def test_adjoint_truth_against_50_digits():
    lam, f, g, edges, sigma, D = OT.hostile("tail_spike+ref")
    c = OT.pixel_vector("tail_spike+ref", "range")
    t = OT.case_adjoint_truth("tail_spike+ref", "range", True)
    old = OT.M.dps
    OT.M.dps = 50
    try:
        fine = OT.adjoint_truth(lam, c, edges, sigma, D, flux=f, reference=g, nus=OT.nus_of(lam))
        for (name, w, scale, _, _), (_, w50, scale50, _, _) in zip(adjoint_quantities(t), adjoint_quantities(fine)):
            d = OT.distance([float(0)] * lam.size, [a - b for a, b in zip(w, w50)], scale50)
            print(f"{name}: {OT.DPS} digits against 50: worst distance {d.max():.3e} of the absolute terms")
            assert np.array_equal(scale == 0, scale50 == 0) and (scale > 0).sum() > 100 and d.max() <= 1e-17
    finally:
        OT.M.dps = old
    # the truth's own sums of absolute terms are observe_adjoint_reference's
    _, _, s, s_ref = aref.adjoint(lam, c, edges, sigma, D, flux=f, reference=g, nus=OT.nus_of(lam))
    assert np.allclose(s, t.scale, rtol=1e-9, atol=0) and np.allclose(s_ref, t.scale_ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,c_kind,with_nus", ADJOINT_CASES)
def test_adjoint_restatement_meets_its_own_allowance(name, c_kind, with_nus):
    t, other = OT.case_adjoint_truth(name, c_kind, with_nus), OT.case_adjoint_truth(name, c_kind, with_nus, OTHER_SEED)
    got, got_other = OT.restated_adjoint(name, c_kind, with_nus), OT.restated_adjoint(name, c_kind, with_nus, OTHER_SEED)
    for k, ((quantity, w, scale, ratio, T), (_, w_o, scale_o, _, _)) in enumerate(zip(adjoint_quantities(t), adjoint_quantities(other))):
        assert (scale > 0).sum() > 10
        d_other = float(np.max(OT.distance(got_other[k], w_o, scale_o)))
        OT.judge(f"{name}, c {c_kind}{', nus' if with_nus else ''}", quantity, got[k], w, scale, ratio, T, got[k], scipy_U(), label="restatement", record=None, d_ref=d_other)


@pytest.mark.parametrize("kind", MUTANTS)
def test_the_judge_rejects_a_wrong_adjoint(kind):
    """(No claim here that the present suite would have missed the mutant: tests/test_gpu_observe_adjoint.py takes its tolerance per point
    against the point's own terms, and a point beyond the detector's ends has terms from far tails alone.)  A window of 7.9 sigma moves a point's
    weight by more than 1e-15 of its terms only where every term is a far tail: the pixel vector `far_tail`, under which the spike 7.95
    sigma above the first pixel has that pixel's term alone.  `far_tail` in turn has no term at the ends of the spacing_ends grid, which
    the widest window reaches, not the first or last pixel's: the end weights are asked of the other two vectors."""
    for c_kind in {MUTANTS[0]: OT.C_KINDS, MUTANTS[1]: OT.C_KINDS[2:], MUTANTS[2]: OT.C_KINDS[:2]}.get(kind, ("even",)):  # (membership: on_edge's own vector)
        for name in (n for n in REJECTED_IN[kind] if n.endswith("+ref")):
            t = OT.case_adjoint_truth(name, c_kind)
            got, ref = mutant_adjoint(kind, name, c_kind), OT.restated_adjoint(name, c_kind)
            for k, (quantity, w, scale, ratio, T) in enumerate(adjoint_quantities(t)):
                own = float(np.max(OT.distance(ref[k], w, scale)))
                d = OT.distance(got[k], w, scale)
                allow = OT.allowance(own, ratio, T, scipy_U())
                print(f"{kind}, {name}, c {c_kind}, {quantity}: worst mutant distance / allowance {float(np.max(d / allow)):.3e}")
                assert not OT.within(got[k], w, scale, ratio, T, own, scipy_U()) and OT.within(ref[k], w, scale, ratio, T, own, scipy_U())
