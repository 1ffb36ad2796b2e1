"""Continuum scattering on the device (sdx_mean_intensity_dev, sdx_scatter_source_dev and their host-buffer twins, ops.mean_intensity,
ops.scatter_source, radiation_field_solvers.scattering_source, SpectralSynthesizer(scattering=True)).

One application of the operator is judged as every kernel of the formal solution is (tests/test_gpu_formal_solution_truth.py): on the
hostile columns of formal_solution_truth, per class, the distance of J and of the diagonal L from the 80-bit restatement of the
definition (tests/scattering_reference.py) is at most formal_solution_truth.bound(the fp64 restatement's own distance, N_d) — four
times that distance plus 4e-15 per gap; `underflow` carries no bound there and carries none here.  Sixteen columns per class, as there, whatever the number of columns a shape
launches: the launch of the shape's own n_nu is the leading columns of the judged launch, bit for bit.
The iteration is judged at the iteration count the device REPORTS for each column — both restatements are run for exactly that many
updates, so stopping one iteration apart is no error — by the same bound, on grids where the iteration contracts: the spectral
radius of its error propagation is derived again here with the restatement, and a column counts for the iterate and the count checks only
below 0.95 (the 57-point grid at albedo 0.999 has 0.953 and is left to the status and fixed-point checks, which do not rest on the rate).
The fp64 restatement forms exp(-tau) as the definition's step does — the kernels' exp_neg, the device library's sequence, restated operation for
operation (scattering_reference.exp_neg64) — not with libm: in a gap just above tau = 5e-4 the weights amplify the last bit of exp by 1 / tau^3,
the two exponentials differ in that bit for one argument in thirteen, and a restatement with libm's measures libm's luck.  Seen before the
restatement had it: `everything`, J, at (57, 20), a column whose downward sweep crosses tau = 1.13e-3 above tau = 1.2e-8 with a second-order
coefficient of -18 — kernel 3.04e-10, a libm restatement 1.18e-11, an exp one ulp away in all 20 angles 4.0e-9; with the step's own exp the
restatement gives 3.04077e-10 against the kernel's 3.04080e-10, and the sixteen columns of the class agree to four digits.
Shapes: the smallest at which the kernel takes another path — two points (both sweeps are only the last-gap form), three, one angle and
several, one wave's frequencies exactly, four waves' and one more (a block's tail, idle lanes), the benchmark's depth and angles over
many blocks, 64 angles.  Every test prints its figures before it asserts; the distances go to scattering_reference.RECORD
(scripts/scattering_truth_table.py -> profiles/scattering_truth_classes.json)."""
import contextlib
import functools
import types

import numpy as np
import pytest

import formal_solution_truth as T
import scattering_reference as R
from stardis_amd import constants as K
from stardis_amd import ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

L = T.L
SHAPES = [(2, 1, 1), (3, 1, 5), (3, 3, 5), (9, 7, 9), (9, 7, 37), (57, 20, 200), (40, 64, 3)]  # (N_d, n_theta, n_nu)
GRIDS = [(3, 1, 0.3, 3.0), (3, 3, 0.3, 3.0), (9, 7, 0.03, 30.0), (17, 3, 1e-3, 100.0), (33, 7, 1e-4, 1e3), (57, 20, 1e-4, 1e3)]  # (points, n_theta, tau range)
ALBEDOS = (0.0, 0.5, 0.9, 0.999)
RADIUS_BELOW = 0.95
# columns per class, the judge's own default (formal_solution_truth.case): a class's figure is the largest over its columns on either side.
# In the classes that sit on the weights' threshold tau = 5e-4 a column's distance is one rounding error of exp amplified by 1 / tau^3 —
# anything between nothing and 1e-8 of the column for the same formulas, by the luck of that one rounding (a single `thin` column at 64
# angles: the restatement 3.9e-11, an exp one ulp away 3.7e-8) — and only the largest of several columns measures an evaluation.
PER_CLASS = 16
TOL, MAX_ITER = 1e-12, 2000


@pytest.fixture(autouse=True)
def extended_precision():
    if not T.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


@contextlib.contextmanager
def profiled(ctx):
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        yield
    finally:
        ctx.call("sdx_profile_enable", 0)


# ---- 1. one application ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def application(n_depth, n_theta, per_class, source_seed):
    """the hostile columns of a shape, the source plane, and J and L of both restatements: computed once, left unchanged"""
    c = T.case(n_depth, n_theta, per_class, "interleaved")
    m = ops.mean_weights(c.thetas, c.weights)
    source = None
    if source_seed is not None:
        source = R.planck(c.nus, c.temps, np.float64) * np.random.default_rng(source_seed).uniform(0.25, 4.0, (n_depth, c.n_nu))
    out = types.SimpleNamespace(case=c, m=m, source=source)
    for tag, dt in (("80", L), ("64", np.float64)):
        S = R.planck(c.nus, c.temps, dt) if source is None else source.astype(dt)
        J, Ld = R.mean_intensity(c.alphas, c.ray, m, S, dt)
        for a in (J, Ld):
            a.setflags(write=False)
        setattr(out, "J" + tag, J)
        setattr(out, "L" + tag, Ld)
    return out


def judge(c, quantity, a, truth, restated, label):
    finite = np.isfinite(restated)
    d_gpu, d_ref = T.distance(a, truth, finite), T.distance(restated, truth, finite)
    missed = []
    for name in c.classes:
        cols = c.columns(name) & finite.any(axis=0)
        if not cols.any():
            continue
        g, o = float(d_gpu[cols].max()), float(d_ref[cols].max())
        R.RECORD.append((label, quantity, c.n_depth, c.n_theta, name, g, o))
        print(f"{label} {quantity} {c.n_depth}/{c.n_theta} {name}: kernel {g:.2e} restatement {o:.2e} bound {T.bound(o, c.n_depth):.2e}")
        if name != "underflow" and not g <= T.bound(o, c.n_depth):
            missed.append((name, g, o))
    assert not missed, (label, quantity, c.n_depth, c.n_theta, missed)


@pytest.mark.parametrize("source_seed", [None, 5], ids=["planck", "source plane"])
@pytest.mark.parametrize("n_depth,n_theta,n_nu", SHAPES)
def test_one_application_against_truth(ctx, n_depth, n_theta, n_nu, source_seed):
    a = application(n_depth, n_theta, PER_CLASS, source_seed)
    c = a.case
    assert c.n_nu == 16 * PER_CLASS >= n_nu
    label = "k_lambda<false>" + ("" if source_seed is None else " source plane")
    with profiled(ctx):
        J, Ld = ops.mean_intensity(c.nus, c.temps, c.ray, a.m, c.alphas, ctx=ctx, source=a.source)
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda<false>"
    judge(c, "J", J, a.J80, a.J64, label)
    judge(c, "L", Ld, a.L80, a.L64, label)
    # a transparent column: nothing is absorbed or emitted — every upward ray carries S[0], no downward ray carries anything
    tr = c.columns("transparent")
    assert np.array_equal(Ld[1:, tr], np.zeros((n_depth - 1, int(tr.sum())))) and np.array_equal(J[:, tr], np.broadcast_to(J[0, tr], (n_depth, int(tr.sum()))))
    # the table's own number of columns: the leading columns alone, bit for bit (a column does not depend on n_nu or on its wave's other columns)
    src = None if a.source is None else np.ascontiguousarray(a.source[:, :n_nu])
    Jn, Ln = ops.mean_intensity(c.nus[:n_nu], c.temps, c.ray, a.m, np.ascontiguousarray(c.alphas[:, :n_nu]), ctx=ctx, source=src)
    assert np.array_equal(Jn, J[:, :n_nu], equal_nan=True) and np.array_equal(Ln, Ld[:, :n_nu], equal_nan=True)
    # either output alone
    only_J, none = ops.mean_intensity(c.nus, c.temps, c.ray, a.m, c.alphas, ctx=ctx, source=a.source, want_L=False)
    assert none is None and np.array_equal(only_J, J, equal_nan=True)
    none, only_L = ops.mean_intensity(c.nus, c.temps, c.ray, a.m, c.alphas, ctx=ctx, source=a.source, want_J=False)
    assert none is None and np.array_equal(only_L, Ld, equal_nan=True)


# ---- 2, 3. the iterate and the fixed point -------------------------------------------------------------------------------------------
def grid_problem(n, n_theta, lo, hi, albedos=ALBEDOS, graded=True):
    """n points log-spaced over [lo, hi] in vertical optical depth, alpha = 1 (the gaps' lengths ARE their optical depths): one column
    per constant albedo with B = 1, then the graded one, albedo = 0.999 / (1 + tau / 3) with B = 1 + tau"""
    tau, dtau = R.log_grid(n, lo, hi)
    thetas, weights = synth.thetas_and_weights(n_theta)
    w = np.repeat(np.asarray(albedos, dtype=np.float64)[None, :], n, axis=0)
    B = np.ones_like(w)
    if graded:
        w = np.concatenate([w, (0.999 / (1.0 + tau / 3.0))[:, None]], axis=1)
        B = np.concatenate([B, (1.0 + tau)[:, None]], axis=1)
    n_nu = w.shape[1]
    return types.SimpleNamespace(n_depth=n, n_theta=n_theta, n_nu=n_nu, tau=tau, thetas=thetas, weights=weights, m=ops.mean_weights(thetas, weights),
                                 ray=dtau.reshape(-1, 1) / np.cos(thetas), alphas=np.ones((n, n_nu)), albedo=np.ascontiguousarray(w),
                                 B=np.ascontiguousarray(B), nus=np.linspace(7.5e14, 3.0e14, n_nu), temps=np.linspace(9500.0, 3900.0, n))


def solve(ctx, p, **kw):
    kw.setdefault("thermal", p.B)
    kw.setdefault("tol", TOL)
    kw.setdefault("max_iter", MAX_ITER)
    return ops.scatter_source(p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, ctx=ctx, **kw)


@pytest.mark.parametrize("n,n_theta,lo,hi", GRIDS)
def test_iterate_and_fixed_point(ctx, n, n_theta, lo, hi):
    p = grid_problem(n, n_theta, lo, hi)
    with profiled(ctx):
        got = solve(ctx, p)
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda<true>"
    op80, op64 = R.operator(p.alphas, p.ray, p.m, L), R.operator(p.alphas, p.ray, p.m, np.float64)
    radius = R.spectral_radius(op64, p.albedo)
    keep = radius < RADIUS_BELOW
    print(f"{n}/{n_theta} [{lo}, {hi}]: radius {np.round(radius, 3)}, iterations {got.iterations}, status {got.status}, change {got.change}")
    assert keep[np.asarray(ALBEDOS + (0.0,)) <= 0.9].all() and keep[-1]  # (the filter may only ever drop albedo 0.999)
    assert (got.status == 0).all() and np.isfinite(got.S).all()
    # the iterate, at the count the device reports
    it80 = R.iterate(op80, p.albedo, p.B, counts=got.iterations)
    it64 = R.iterate(op64, p.albedo, p.B, counts=got.iterations)
    yes = np.ones((n, p.n_nu), dtype=bool)
    d_gpu, d_ref = T.distance(got.S, it80["S"], yes), T.distance(it64["S"], it80["S"], yes)
    own = R.iterate(op64, p.albedo, p.B, tol=TOL, max_iter=MAX_ITER)
    print(f"    S: kernel {d_gpu}, restatement {d_ref}; the restatement's own count {own['iterations']}")
    for i in np.flatnonzero(keep):
        assert d_gpu[i] <= T.bound(d_ref[i], n), (i, d_gpu[i], d_ref[i])
        assert abs(int(got.iterations[i]) - int(own["iterations"][i])) <= 1 and own["status"][i] == 0, (i, got.iterations[i], own["iterations"][i])
    # the fixed point: the 80-bit residual of what the device returned
    S = got.S.astype(L)
    J80, J64 = op80.J(S), op64.J(got.S)
    residual = np.abs(((1 - p.albedo.astype(L)) * p.B.astype(L) + p.albedo.astype(L) * J80) - S).max(axis=0).astype(np.float64)
    d_app = T.distance(J64, J80, yes)
    allowed = TOL * np.abs(got.S).max(axis=0) + np.array([T.bound(d, n) for d in d_app]) * np.abs(J80).max(axis=0).astype(np.float64)
    print(f"    residual {residual}, allowed {allowed}")
    assert (residual <= allowed).all()
    # J is the mean intensity of the returned S: the one-application kernel on it, bit for bit
    J_of_S, _ = ops.mean_intensity(p.nus, p.temps, p.ray, p.m, p.alphas, ctx=ctx, source=got.S, want_L=False)
    assert np.array_equal(got.J, J_of_S)


# ---- 4. no scattering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth,n_theta,n_nu", [(2, 1, 1), (9, 7, 37), (57, 20, 200)])
def test_zero_albedo_is_lte_bit_for_bit(ctx, n_depth, n_theta, n_nu):
    c = T.case(n_depth, n_theta, -(-n_nu // 4), "interleaved", classes=("moderate", "thick", "ramp", "thin"))
    m = ops.mean_weights(c.thetas, c.weights)
    nus, alphas = c.nus[:n_nu], np.ascontiguousarray(c.alphas[:, :n_nu])
    got = ops.scatter_source(nus, c.temps, c.ray, m, alphas, np.zeros(n_depth), ctx=ctx)
    assert (got.iterations == 1).all() and (got.status == 0).all() and (got.change == 0).all()
    lte, _ = ops.raytrace_arrays(nus, c.temps, c.ray, c.weights, alphas, ctx=ctx)
    with_S, _ = ops.raytrace_arrays(nus, c.temps, c.ray, c.weights, alphas, ctx=ctx, source=got.S)
    assert np.array_equal(with_S, lte) and lte[-1].all()
    # S is the Planck plane as the formal-solution kernels stage it (that is what the two fluxes above compare bit for bit): against the
    # reference-order routine it moves by the rounding of the exponent x = h nu / (k T), which exp turns into x ulp, and a few ulp of its own
    planck = ops.blackbody_flux_at_nu(nus, c.temps, ctx=ctx)
    x = (K.H_CGS * nus)[None, :] / (K.K_B_CGS * c.temps[:, None])
    print("S against the reference-order Planck function, in ulp:", float((np.abs(got.S / planck - 1) / np.finfo(np.float64).eps).max()), "largest x", float(x.max()))
    assert (np.abs(got.S / planck - 1) <= (x + 4) * np.finfo(np.float64).eps).all()
    # a caller's plane in place of Planck comes back as it went in, and so does a plane of scattering opacities that are all zero
    plane = planck * np.random.default_rng(n_nu).uniform(0.5, 2.0, planck.shape)
    for scatter in (np.zeros(n_depth), np.zeros((n_depth, n_nu))):
        got = ops.scatter_source(nus, c.temps, c.ray, m, alphas, scatter, ctx=ctx, thermal=plane)
        assert np.array_equal(got.S, plane) and (got.iterations == 1).all() and (got.status == 0).all()


# ---- 5. the ends of the loop ----------------------------------------------------------------------------------------------------------
def test_max_iter_ends_the_loop(ctx):
    p = grid_problem(9, 7, 0.03, 30.0)
    got = solve(ctx, p, tol=0.0, max_iter=7)
    moving = np.asarray(ALBEDOS + (0.5,)) > 0  # (albedo 0 has reached its fixed point after one update: change 0 <= 0)
    print(got.iterations, got.status, got.change)
    assert (got.status[moving] == 1).all() and (got.iterations[moving] == 7).all() and (got.change[moving] > 0).all()
    assert got.status[0] == 0 and got.iterations[0] == 1
    it64 = R.iterate(R.operator(p.alphas, p.ray, p.m, np.float64), p.albedo, p.B, counts=got.iterations)
    assert np.abs(got.S / it64["S"] - 1).max() <= 1e-13  # seven updates of the restatement


def test_a_divergent_column_stops_and_leaves_the_others_alone(ctx):
    """three points over [0.1, 10], one angle, albedo 0.999: the diagonal leaves [0, 1] and the discrete problem has no contraction (the
    restatement's spectral radius there is 7.7).  Its neighbours in the same launch — the same geometry seen through other opacities:
    the contracting three-point grid over [0.3, 3] — converge, bit for bit as they do without it."""
    thetas, weights = synth.thetas_and_weights(1)
    m = ops.mean_weights(thetas, weights)
    _, bad = R.log_grid(3, 0.1, 10.0)
    _, good = R.log_grid(3, 0.3, 3.0)
    ray = bad.reshape(-1, 1) / np.cos(thetas)
    n_nu, at = 70, 33  # (two waves of one-angle columns; the divergent one in the middle of the first)
    alphas = np.repeat(R.alphas_for(good, bad)[:, None], n_nu, axis=1)
    alphas[:, at] = 1.0
    albedo = np.repeat(np.linspace(0.0, 0.999, n_nu)[None, :], 3, axis=0)
    albedo[:, at] = 0.999
    nus, temps, B = np.linspace(7.5e14, 3.0e14, n_nu), np.linspace(9500.0, 3900.0, 3), np.ones((3, n_nu))
    op = R.operator(alphas, ray, m, np.float64)
    radius = R.spectral_radius(op, albedo)
    print("radius of the divergent column", radius[at], "largest of the others", np.delete(radius, at).max(), "its diagonal", op.diagonal()[:, at])
    assert radius[at] > 5 and np.delete(radius, at).max() < RADIUS_BELOW
    got = ops.scatter_source(nus, temps, ray, m, alphas, albedo * alphas, ctx=ctx, thermal=B, tol=TOL, max_iter=300)  # (the call returns)
    print("divergent column: status", got.status[at], "iterations", got.iterations[at], "change", got.change[at])
    assert got.status[at] != 0 and np.isfinite(got.S[:, at]).all()
    others = np.arange(n_nu) != at
    assert (got.status[others] == 0).all()
    without = ops.scatter_source(nus[others], temps, ray, m, np.ascontiguousarray(alphas[:, others]), np.ascontiguousarray((albedo * alphas)[:, others]),
                                 ctx=ctx, thermal=np.ascontiguousarray(B[:, others]), tol=TOL, max_iter=300)
    for name in ("S", "J", "iterations", "status", "change"):
        assert np.array_equal(getattr(got, name)[..., others], getattr(without, name)), name
    # the change that is not finite: a thermal plane whose differences overflow — J is not finite in the first sweep, the update is
    # refused, S stays at S^0 = B; its neighbour converges
    thermal = np.array([[1.0, 1e308], [-1.0, -1e308], [1.0, 1e308]])
    broken = ops.scatter_source(nus[:2], temps, ray, m, np.ones((3, 2)), np.full((3, 2), 0.5), ctx=ctx, thermal=thermal, tol=TOL, max_iter=300)
    print("overflowing column: status", broken.status, "iterations", broken.iterations, "change", broken.change)
    assert broken.status[0] == 0 and np.isfinite(broken.S[:, 0]).all()
    assert broken.status[1] == 2 and broken.iterations[1] == 1 and np.isposinf(broken.change[1]) and np.array_equal(broken.S[:, 1], thermal[:, 1])


# ---- 6. independence and determinism -----------------------------------------------------------------------------------------------
def test_a_column_does_not_depend_on_its_launch(ctx):
    """200 columns on the 57-point grid at 20 angles, albedo 0 .. 0.999 (1 to about 500 iterations in one launch): a column alone, in a
    shard of the grid, in the whole launch, twice in a row and through the host-buffer twin — the same bits"""
    n, n_nu = 57, 200
    tau, dtau = R.log_grid(n, 1e-4, 1e3)
    thetas, weights = synth.thetas_and_weights(20)
    m = ops.mean_weights(thetas, weights)
    ray = dtau.reshape(-1, 1) / np.cos(thetas)
    rng = np.random.default_rng(57)
    albedo = np.repeat(rng.permutation(np.linspace(0.0, 0.999, n_nu))[None, :], n, axis=0)  # (fast and slow columns share every wave)
    alphas, B = np.ones((n, n_nu)), np.repeat((1.0 + tau)[:, None], n_nu, axis=1) * rng.uniform(0.5, 2.0, n_nu)
    nus, temps = np.linspace(7.5e14, 3.0e14, n_nu), np.linspace(9500.0, 3900.0, n)

    def run(cols):
        cut = lambda a: np.ascontiguousarray(a[:, cols])  # noqa: E731
        return ops.scatter_source(nus[cols], temps, ray, m, cut(alphas), cut(albedo * alphas), ctx=ctx, thermal=cut(B), tol=TOL, max_iter=MAX_ITER)

    whole = run(slice(None))
    print("iterations", whole.iterations.min(), "..", whole.iterations.max())
    assert (whole.status == 0).all() and whole.iterations.min() == 1 and whole.iterations.max() > 300
    again = run(slice(None))
    shard = run(slice(60, 137))
    for name in ("S", "J", "iterations", "status", "change"):
        assert np.array_equal(getattr(again, name), getattr(whole, name)), name
        assert np.array_equal(getattr(shard, name), getattr(whole, name)[..., 60:137]), name
    for k in (0, 59, 136, 199, int(np.argmax(whole.iterations))):
        alone = run(slice(k, k + 1))
        for name in ("S", "J", "iterations", "status", "change"):
            assert np.array_equal(getattr(alone, name), getattr(whole, name)[..., k:k + 1]), (name, k)
    # the host-buffer twins
    p = lambda a: a.ctypes.data  # noqa: E731
    h = [np.ascontiguousarray(a, dtype=np.float64) for a in (nus, temps, ray, m, alphas, albedo * alphas, B)]
    S, J, change = np.full((n, n_nu), np.nan), np.full((n, n_nu), np.nan), np.full(n_nu, np.nan)
    iterations, status = np.full(n_nu, -1, dtype=np.int32), np.full(n_nu, -1, dtype=np.int32)
    ctx.call("sdx_scatter_source_f64", n, n_nu, 20, p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[5]), 1, p(h[6]), TOL, MAX_ITER, p(S), p(J), p(iterations),
             p(status), p(change))
    for name, value in (("S", S), ("J", J), ("iterations", iterations), ("status", status), ("change", change)):
        assert np.array_equal(value, getattr(whole, name)), name
    S2 = np.full((n, n_nu), np.nan)
    ctx.call("sdx_scatter_source_f64", n, n_nu, 20, p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[5]), 1, p(h[6]), TOL, MAX_ITER, p(S2), None, None, None, None)
    assert np.array_equal(S2, S)
    Jd, Ld = ops.mean_intensity(nus, temps, ray, m, alphas, ctx=ctx, source=B)
    Jh, Lh = np.full((n, n_nu), np.nan), np.full((n, n_nu), np.nan)
    ctx.call("sdx_mean_intensity_f64", n, n_nu, 20, p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(h[4]), p(h[6]), p(Jh), p(Lh))
    assert np.array_equal(Jh, Jd) and np.array_equal(Lh, Ld)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    p = grid_problem(9, 7, 0.03, 30.0)
    n = p.n_nu
    d = [ctx.upload(a) for a in (p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo, p.B)]
    out = ctx.empty((9, n))

    def iterate(n_depth=9, n_theta=7, n_nu=n, tol=TOL, max_iter=10, S=out.ptr):
        ctx.call("sdx_scatter_source_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, d[5].ptr, n, d[6].ptr, n, tol, max_iter,
                 S, n, None, 0, None, None, None)

    def apply(n_depth=9, n_theta=7, n_nu=n, J=out.ptr):
        ctx.call("sdx_mean_intensity_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, None, 0, J, n, None, 0)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for call in (iterate, apply):
                for n_nu in (n, 0):  # also at set-up time, with an empty grid
                    with pytest.raises(ValueError, match="mixed_precision"):
                        call(n_nu=n_nu)
        finally:
            ctx.set_option("mixed_precision", 0)
        for call in (iterate, apply):
            for n_nu in (n, 0):
                with pytest.raises(ValueError, match="64 angles"):
                    call(n_theta=65, n_nu=n_nu)
                with pytest.raises(ValueError, match="deep"):
                    call(n_depth=1400, n_nu=n_nu)  # (6 n_depth + 28 doubles at seven angles and one frequency per wave: above 64 KB)
        for n_nu in (n, 0):
            for kw in (dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=0)):
                with pytest.raises(ValueError, match="tol >= 0"):
                    iterate(n_nu=n_nu, **kw)
        with pytest.raises(ValueError, match="null pointer"):
            iterate(S=None)
        with pytest.raises(ValueError, match="no output"):
            apply(J=None)
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 0
        iterate()  # and the context still serves
        apply()
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 2


# ---- 7. the engine ----------------------------------------------------------------------------------------------------------------------
def small_model():
    """12 depth points of the solar structure, 300 frequencies around H alpha, 40 lines, 8 angles"""
    sun = synth.solar_atmosphere()
    pick = np.linspace(0, sun["temperatures"].size - 1, 12).astype(int)
    atm = {k: (v[pick] if isinstance(v, np.ndarray) and v.size == sun["temperatures"].size else v) for k, v in sun.items()}
    atm["dist"] = np.diff(atm["r"])
    nus = synth.tracing_grid(6560.0, 6570.0, n_override=300)
    thetas, weights = synth.thetas_and_weights(8)
    return types.SimpleNamespace(atm=atm, nus=nus, lines=synth.synth_lines(nus, atm, 40, seed=17, mix=(0.5, 0.4, 0.1)), thetas=thetas, weights=weights,
                                 cont=synth.synth_continuum_state(atm))


def synthesizer(ctx, m, **kw):
    return SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, m.lines, m.cont, ctx=ctx, track_evaluations=False, **kw)


def outputs(syn):
    return dict(F=np.array(syn.F_nu()), total=np.array(syn.total_alphas()), line=np.array(syn.alpha_line()), C=np.array(syn.contribution.numpy()),
                Fc=np.array(syn.F_nu_continuum))


def test_engine(ctx):
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    m = small_model()
    common = dict(keep_contribution=True, keep_continuum_flux=True)
    plain = synthesizer(ctx, m, **common)
    with profiled(ctx):
        plain.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 0
    lte = outputs(plain)
    assert plain.scattering is None and not hasattr(plain, "d_Ssc")
    with pytest.raises(RuntimeError, match="scattering=True"):
        plain.scattering_flux
    plain.close()
    with pytest.raises(ValueError, match="continuum"):
        SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, m.lines, None, ctx=ctx, scattering=True)

    syn = synthesizer(ctx, m, scattering=True, keep_total=False, **common)
    assert syn.keep_total  # forced
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda<true>"
    for key, value in outputs(syn).items():  # everything else is the twin's, bit for bit: F_nu stays the LTE flux
        assert np.array_equal(value, lte[key]), key
    S, J, F = np.array(syn.scattering_source.numpy()), np.array(syn.scattering_mean_intensity.numpy()), np.array(syn.scattering_flux.numpy())
    iterations, status = syn.scattering_iterations, syn.scattering_status
    print("iterations", iterations.min(), "..", iterations.max(), "| largest albedo",
          float((ops.alpha_electron(1, m.cont["n_e"], ctx=ctx).numpy() / lte["total"].min(axis=1, keepdims=True)).max()),
          "| largest change of the emergent flux", float(np.abs(F / lte["F"][-1] - 1).max()))
    assert S.shape == J.shape == (12, 300) and F.shape == (300,) and iterations.dtype == status.dtype == np.int32
    assert (status == 0).all() and (iterations >= 2).all() and not np.array_equal(F, lte["F"][-1])
    # the ops path on the step's own total_alphas
    ray = m.atm["dist"].reshape(-1, 1) / np.cos(m.thetas)
    thomson = ops.alpha_electron(1, m.cont["n_e"], ctx=ctx).numpy().reshape(-1)
    assert np.array_equal(thomson, ops.alpha_electron(300, m.cont["n_e"], ctx=ctx).numpy()[:, 17])  # the electron term of the total: the same bits
    mw = ops.mean_weights(m.thetas, m.weights)
    got = ops.scatter_source(m.nus, m.atm["temperatures"], ray, mw, lte["total"], thomson, ctx=ctx)
    assert np.array_equal(got.S, S) and np.array_equal(got.J, J) and np.array_equal(got.iterations, iterations) and np.array_equal(got.status, status)
    flux, _ = ops.raytrace_arrays(m.nus, m.atm["temperatures"], ray, m.weights, lte["total"], ctx=ctx, source=S)
    assert np.array_equal(flux[-1], F)
    # the solver-level twin on plain namespaces
    stellar_model = types.SimpleNamespace(spherical=False, temperatures=m.atm["temperatures"], geometry=types.SimpleNamespace(dist_to_next_depth_point=m.atm["dist"]))
    entries = dict(alpha_rayleigh=0, alpha_electron=ops.alpha_electron(300, m.cont["n_e"], ctx=ctx).numpy())
    field = types.SimpleNamespace(thetas=m.thetas, I_nus_weights=m.weights, frequencies=m.nus,
                                  opacities=types.SimpleNamespace(total_alphas=lte["total"], opacities_dict=entries))
    twin = rfs.scattering_source(stellar_model, field)
    assert np.array_equal(twin.S, S) and np.array_equal(twin.iterations, iterations)
    Jm, _ = rfs.mean_intensity(stellar_model, field)
    Jo, _ = ops.mean_intensity(m.nus, m.atm["temperatures"], ray, mw, lte["total"], ctx=ctx)
    assert np.array_equal(Jm, Jo)
    with pytest.raises(NotImplementedError):
        rfs.scattering_source(types.SimpleNamespace(spherical=True), field)
    # recorded and replayed
    syn.capture()
    for a in (syn.scattering_source, syn.scattering_mean_intensity, syn.d_Fsc):
        a.zero()
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.scattering_source.numpy(), S) and np.array_equal(syn.scattering_mean_intensity.numpy(), J)
    assert np.array_equal(syn.scattering_flux.numpy(), F) and np.array_equal(syn.F_nu(), lte["F"]) and np.array_equal(syn.scattering_iterations, iterations)
    syn.close()
    # a frequency shard: its own columns of the whole grid, bit for bit; a looser loop through the option's dictionary
    part = synthesizer(ctx, m, scattering=dict(tol=1e-6, max_iter=50), shard=(100, 120))
    part.step()
    ctx.synchronize()
    loose = ops.scatter_source(m.nus[100:220], m.atm["temperatures"], ray, mw, np.ascontiguousarray(lte["total"][:, 100:220]), thomson, ctx=ctx, tol=1e-6, max_iter=50)
    assert np.array_equal(part.scattering_source.numpy(), loose.S) and np.array_equal(part.scattering_iterations, loose.iterations)
    assert (part.scattering_iterations <= iterations[100:220]).all() and np.array_equal(part.F_nu(), lte["F"][:, 100:220])
    with pytest.raises(ValueError, match="scattering"):
        part.keep_total = False
    part.close()
