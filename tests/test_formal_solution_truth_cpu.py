"""The conditions tests/test_gpu_formal_solution_truth.py rests on, checked on the reference alone (no GPU): at every shape of that
file the double-precision oracle (oracle/stardis_oracle.c, the reference's operations in the reference's order) is run against the
80-bit evaluation of the same formulas (tests/formal_solution_truth.py) on the hostile columns.  The oracle has the truth's NaN
pattern and no infinity, transparent columns are exactly zero, and in the classes whose weights do not cancel it stays within 1e-13
of the truth (measured: 1.5e-14 at most, flux and intensities) — so a kernel held to four times the oracle's distance is held to something.

Largest oracle-to-truth distance of the flux per class, per_class = 16, seed 100 n_depth + n_theta (the GPU figures beside them are in
profiles/formal_truth_classes.json):

    depth/theta  thin     straddle_small  moderate  everything  ramp     tiny     underflow
    2/3          2.8e-15  1.3e-7          3.7e-11   2.0e-7      8.4e-12  2.1e-14  4.7e-1
    9/20         1.1e-14  5.6e-9          5.0e-13   5.7e-10     1.1e-8   5.4e-14  1.2e-2
    56/20        6.5e-14  1.0e-10         1.3e-13   9.0e-11     1.4e-11  4.7e-14  7.4e-5
    57/64        1.3e-7   5.6e-11         2.4e-14   2.3e-10     1.3e-11  1.7e-14  2.4e-4

(in `underflow` w2 is subnormal: the double-precision reference is itself meaningless there, and no bound is put on it)."""
import numpy as np
import pytest

import contribution_reference as cref
import formal_solution_truth as T

pytestmark = pytest.mark.skipif(not T.EXTENDED, reason="no extended-precision long double on this host")

PLANE = [(2, 3), (3, 7), (9, 20), (55, 1), (56, 20), (57, 64)]
SPHERICAL = [(9, 20), (56, 20), (40, 7)]
STABLE = ("thick", "straddle_50", "huge", "overflow", "spike")  # no cancellation in the weights: the oracle is as good as its arithmetic


def conditions(c):
    ref = c.reference()
    Ft, It, Fo, Io = ref["Ft"], ref["It"], ref["Fo"], ref["Io"]
    assert Fo.shape == Ft.shape == (c.n_depth, c.n_nu) and Io.shape == It.shape == (c.n_depth, c.n_nu, c.n_theta)
    assert np.array_equal(np.isnan(Fo), np.isnan(Ft)) and np.array_equal(np.isnan(Io), np.isnan(It))
    assert not np.isinf(Fo).any() and not np.isinf(Io).any()
    assert not np.isinf(Ft).any() and not np.isinf(It).any()
    if "transparent" in c.classes:
        cols = c.columns("transparent")
        assert not Fo[:, cols].any() and not Io[:, cols].any() and not Ft[:, cols].any()
    if "leading_transparent" in c.classes and not c.spherical:  # (the inward sweep of spherical geometry arrives with an intensity)
        for j in np.flatnonzero(c.columns("leading_transparent")):
            first_opaque = int(np.flatnonzero(c.alphas[:, j])[0])  # rows 0 .. first_opaque - 1 are zero: gaps 0 .. first_opaque - 1 transparent
            assert not Fo[:first_opaque + 1, j].any() and not Ft[:first_opaque + 1, j].any()
            assert Fo[first_opaque + 1:, j].all()
    if not c.spherical:
        assert not Fo[0].any() and not Ft[0].any()
    flux = T.per_class(c, Fo, Ft, Fo)
    intensity = T.per_class(c, Io, It, Io, reduce_angles=True)
    for name in STABLE:
        if name in c.classes:
            assert flux[name][0] <= 1e-13 and intensity[name][0] <= 1e-13, (name, flux[name], intensity[name])
    return flux


@pytest.mark.parametrize("order", ["grouped", "interleaved"])
@pytest.mark.parametrize("n_depth,n_theta", PLANE)
def test_oracle_meets_the_conditions_plane_parallel(n_depth, n_theta, order):
    c = T.case(n_depth, n_theta, 16, order)
    flux = conditions(c)
    # the NaN-producing classes do produce NaN where the geometry allows it (two opaque gaps below the transparent one)
    Fo = c.reference()["Fo"]
    if n_depth >= 9:
        assert np.isnan(Fo[-1, c.columns("surface_transparent")]).all()
        assert np.isnan(Fo[-1, c.columns("interior_transparent")]).any()
    assert np.isfinite(Fo[:, ~(c.columns("surface_transparent") | c.columns("interior_transparent"))]).all()
    assert np.isfinite(flux["underflow"][0])  # (meaningless, but finite)


def test_orders_hold_the_same_columns():
    g, i = T.case(9, 20, 16, "grouped"), T.case(9, 20, 16, "interleaved")
    assert g.cls[:16].tolist() == ["thin"] * 16 and i.cls[:16].tolist() == list(T.CLASSES)
    for name in T.CLASSES:
        assert np.array_equal(g.alphas[:, g.columns(name)], i.alphas[:, i.columns(name)])
    again = T.Case(9, 20, 16, "grouped")
    assert np.array_equal(again.alphas, g.alphas) and np.array_equal(again.dist, g.dist)


def test_classes_reach_the_regimes_they_are_named_for():
    c = T.case(56, 20)
    with np.errstate(all="ignore"):
        tau = (np.sqrt(c.alphas[1:]) * np.sqrt(c.alphas[:-1]))[:, :, None] * c.ray[:, None, :]
        den = tau[:-1] * tau[1:] * (tau[:-1] + tau[1:])
    of = lambda a, name: a[:, c.columns(name)]  # noqa: E731
    tiny = np.finfo(np.float64).tiny
    assert (of(tau, "thin")[:, :, :1] < T.TAU_SMALL).all()  # (the steepest of 20 angles may cross 5e-4)
    assert (of(tau, "straddle_small") < T.TAU_SMALL).any() and (of(tau, "straddle_small") > T.TAU_SMALL).any()
    assert (of(tau, "straddle_50") < T.TAU_BIG).any() and (of(tau, "straddle_50") > T.TAU_BIG).any()
    assert (of(tau, "thick") >= T.TAU_BIG).all()
    assert (of(den, "tiny") >= tiny).all() and (of(den, "tiny") < 1e-250).all()
    assert (of(den, "underflow") < tiny).all()
    assert np.isfinite(of(den, "huge")).all() and (of(den, "huge") > 1e250).all()
    assert np.isinf(of(den, "overflow")).all()
    assert not of(tau, "transparent").any()


def test_pure_regime_inputs():
    """130 columns of one class: whole launches in one regime of the weights"""
    for shape in [(55, 1), (56, 20)]:
        for name in ("thin", "thick"):
            c = T.case(*shape, 130, "grouped", (name,))
            assert c.n_nu == 130
            conditions(c)  # (thick: within 1e-13; thin: the steepest of 20 angles may cross 5e-4)
            assert np.isfinite(c.reference()["Fo"]).all()


def test_oracle_meets_the_conditions_deep_model():
    conditions(T.case(985, 20, 2))


@pytest.mark.parametrize("n_depth,n_theta", SPHERICAL)
def test_oracle_meets_the_conditions_spherical(n_depth, n_theta):
    c = T.case(n_depth, n_theta, 16, "grouped", T.CLASSES, True)
    assert (c.ray == 0).any() == (n_depth >= 40)  # grazing rays miss the inner shells of the deeper models
    conditions(c)


@pytest.mark.parametrize("n_depth,n_theta", [(175, 20), (302, 20)])
def test_oracle_meets_the_conditions_other_depths(n_depth, n_theta):
    conditions(T.case(n_depth, n_theta, 16 if n_depth < 200 else 4))


@pytest.mark.parametrize("n_depth,n_theta,per", [(9, 20, 16), (56, 20, 16), (302, 20, 4)])
def test_contribution_truth(n_depth, n_theta, per):
    """the longdouble contribution function adds up to the longdouble emergent flux, and the numpy restatement of the definition
    (tests/contribution_reference.py, the judge's counterpart for C) has its NaN pattern"""
    c = T.case(n_depth, n_theta, per)
    Ft, _, Ct = c.truth(contribution=True)
    assert np.array_equal(Ft, c.reference()["Ft"], equal_nan=True)
    Co = cref.contribution_function(c.nus, c.temps, c.ray, c.weights, c.alphas)
    assert np.array_equal(np.isnan(Co), np.isnan(Ct)) and not np.isinf(Co).any()
    assert np.array_equal(np.isnan(Ct).any(axis=0), np.isnan(Ft[-1]))  # a column is undefined in C exactly where the flux is
    ok = ~np.isnan(Ft[-1])
    total = Ct[:, ok].sum(axis=0)
    assert np.max(np.abs(total - Ft[-1, ok]) / np.maximum(np.abs(Ft[-1, ok]), 1e-300)) < 1e-17 * n_depth
    assert not Ct[0].any() and not Ct[:, c.columns("transparent")].any()
    finite = np.isfinite(Co)
    d = T.distance(Co, Ct, finite)
    for name in STABLE:
        assert d[c.columns(name)].max() <= 1e-13, name


def test_source_plane():
    """the Planck function handed over as a plane gives the Planck run (rounded to double first: to 1e-15)"""
    c = T.case(9, 20)
    S = cref.planck(c.nus, c.temps)
    F, I = T.truth(c.nus, c.temps, c.dist, c.thetas, c.weights, c.alphas, source=S)
    ref = c.reference()
    assert np.array_equal(np.isnan(F), np.isnan(ref["Ft"]))
    keep = ~c.columns("underflow")
    assert T.distance(F, ref["Ft"], np.isfinite(ref["Fo"]))[keep].max() < 1e-11
    twice, _ = T.truth(c.nus, c.temps, c.dist, c.thetas, c.weights, c.alphas, source=2.0 * S)
    assert T.distance(twice, 2 * F, np.isfinite(ref["Fo"])).max() < 1e-18


def test_distance_and_bound():
    ref = np.array([[1.0, 0.0, np.nan], [4.0, 0.0, 2.0]])
    a = np.array([[1.5, 0.0, 7.0], [4.0, 0.0, 2.0]])
    assert T.distance(a, ref, np.isfinite(ref)).tolist() == [0.125, 0.0, 0.0]
    assert np.isinf(T.distance(np.array([[np.inf], [1.0]]), np.ones((2, 1)), np.ones((2, 1), dtype=bool))[0])
    assert T.bound(1e-9, 56) == 4e-9 + 55 * 4e-15
    near = T.near_threshold(np.array([[5e-10, 1e-3], [5e-10, 1e-3]]), np.array([[1e6]]))
    assert near.tolist() == [True, False]
