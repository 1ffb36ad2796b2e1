"""The scattering adjoint on the device (sdx_mean_intensity_adjoint_dev, sdx_scatter_response_dev and their host-buffer twins,
ops.mean_intensity_adjoint, ops.scatter_response, radiation_field_solvers.scattering_response,
SpectralSynthesizer(scattering=True, keep_response=True)).

Judged as the forward kernels are (tests/test_gpu_scattering.py, whose shapes, grids, albedos and radius filter are imported): one
application on the hostile columns of formal_solution_truth, per judged class (test_scattering_adjoint_cpu.JUDGED), the kernel's
distance from the 80-bit restatement (tests/scattering_adjoint_reference.py) at most formal_solution_truth.bound(the fp64
restatement's own distance, N_d); the solve at the iteration count the device REPORTS; end to end against Richardson quotients of the
device's own scatter_source -> raytrace flux, the gap within twice that of the fp64 restatement put through the same procedure
(scattering_adjoint_reference.restated_gaps: per grid and quantity, the largest over the columns the radius filter keeps).  Every test
prints its figures before it asserts; they go to scattering_adjoint_reference.RECORD (scripts/scattering_adjoint_truth_table.py ->
profiles/scattering_adjoint_truth.json)."""
import types

import numpy as np
import pytest

import formal_solution_truth as T
import scattering_adjoint_reference as A
import scattering_reference as R
import test_gpu_scattering as F
import test_scattering_adjoint_cpu as C
from stardis_amd import ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

L = T.L
TOL, MAX_ITER = F.TOL, F.MAX_ITER
profiled = F.profiled
OUTPUTS = ("y", "R_thermal", "R_absorption", "R_scatter")
EVERYTHING = OUTPUTS + ("iterations", "status", "change")


@pytest.fixture(autouse=True)
def extended_precision():
    if not T.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def judge(c, quantity, a, truth, restated, label):
    finite = np.isfinite(restated)
    d_gpu, d_ref = T.distance(a, truth, finite), T.distance(restated, truth, finite)
    missed = []
    for name in C.JUDGED:
        cols = c.columns(name) & finite.any(axis=0)
        assert cols.sum() >= (1 - C.RT.EXCLUDED_AT_MOST) * c.columns(name).sum(), (quantity, name)
        g, o = float(d_gpu[cols].max()), float(d_ref[cols].max())
        A.RECORD.append((label, quantity, c.n_depth, c.n_theta, name, g, o))
        print(f"{label} {quantity} {c.n_depth}/{c.n_theta} {name}: kernel {g:.2e} restatement {o:.2e} bound {T.bound(o, c.n_depth):.2e}")
        if not g <= T.bound(o, c.n_depth):
            missed.append((name, g, o))
    assert not missed, (label, quantity, c.n_depth, c.n_theta, missed)


# ---- 1. one application ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth,n_theta,n_nu", F.SHAPES)
def test_one_application_against_truth(ctx, n_depth, n_theta, n_nu):
    a = C.one_application(n_depth, n_theta)
    c = a.case
    assert c.n_nu >= n_nu
    args = (c.nus, c.temps, c.ray, a.m, c.alphas, a.z)
    with profiled(ctx):
        Lt, G = ops.mean_intensity_adjoint(*args, ctx=ctx, source=a.source)
        assert ctx.profile("k_lambda_adjoint")[0] == 1 and ctx.profile_variant("k_lambda_adjoint") == "k_lambda_adjoint<false>"
    judge(c, "Lt", Lt, a.Lt80, a.Lt64, "k_lambda_adjoint<false>")
    judge(c, "G", G, a.G80, a.G64, "k_lambda_adjoint<false>")
    # either output alone
    only_Lt, none = ops.mean_intensity_adjoint(*args, ctx=ctx, source=a.source, want_G=False)
    assert none is None and np.array_equal(only_Lt, Lt, equal_nan=True)
    none, only_G = ops.mean_intensity_adjoint(*args, ctx=ctx, source=a.source, want_Lt=False)
    assert none is None and np.array_equal(only_G, G, equal_nan=True)
    # the leading n_nu columns alone
    cut = lambda x: np.ascontiguousarray(x[:, :n_nu])  # noqa: E731
    Ln, Gn = ops.mean_intensity_adjoint(c.nus[:n_nu], c.temps, c.ray, a.m, cut(c.alphas), cut(a.z), ctx=ctx, source=cut(a.source))
    assert np.array_equal(Ln, Lt[:, :n_nu], equal_nan=True) and np.array_equal(Gn, G[:, :n_nu], equal_nan=True)


# ---- 2. the dot identity with the forward kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth,n_theta,n_nu", F.SHAPES)
def test_dot_identity_with_the_forward_kernel(ctx, n_depth, n_theta, n_nu):
    """sum z . J(x) from k_lambda<false> against sum (Lambda^T z) . x, x the seeded source plane, relative to sum |z| |J|; the sums are
    formed in 80-bit arithmetic from the fp64 planes of either side"""
    a = C.one_application(n_depth, n_theta)
    c = a.case
    J, _ = ops.mean_intensity(c.nus, c.temps, c.ray, a.m, c.alphas, ctx=ctx, source=a.source, want_L=False)
    Lt, _ = ops.mean_intensity_adjoint(c.nus, c.temps, c.ray, a.m, c.alphas, a.z, ctx=ctx, want_G=False)

    def identity(Jx, Ltz):
        with np.errstate(all="ignore"):
            lhs, rhs = a.z.astype(L) * np.asarray(Jx).astype(L), np.asarray(Ltz).astype(L) * a.source.astype(L)
            ok = np.isfinite(lhs).all(axis=0) & np.isfinite(rhs).all(axis=0)
            return np.where(ok, np.abs(lhs.sum(axis=0) - rhs.sum(axis=0)) / np.maximum(np.abs(lhs).sum(axis=0), L(1e-300)), np.nan).astype(np.float64), ok

    g_gpu, ok_gpu = identity(J, Lt)
    g_ref, ok_ref = identity(a.J64, a.Lt64)
    missed = []
    for name in C.JUDGED:
        cols = c.columns(name) & ok_ref
        assert cols.any() and ok_gpu[cols].all(), name
        g, o = float(g_gpu[cols].max()), float(g_ref[cols].max())
        A.RECORD.append(("dot identity", "z.J(x) - (Lt z).x", n_depth, n_theta, name, g, o))
        print(f"dot identity {n_depth}/{n_theta} {name}: kernels {g:.2e} restatement {o:.2e} bound {T.bound(o, n_depth):.2e}")
        if not g <= T.bound(o, n_depth):
            missed.append((name, g, o))
    assert not missed, missed


# ---- 3. the solve ------------------------------------------------------------------------------------------------------------------------
def flux_planes(ctx, p, S):
    """the emergent flux's direct part and cotangent at the source plane S: R_alpha and R_source of the LTE response functions"""
    return ops.response(p.nus, p.temps, p.ray, p.weights, p.alphas, ctx=ctx, source=S)


def respond(ctx, p, S, cotangent, direct, **kw):
    kw.setdefault("thermal", p.B)
    kw.setdefault("tol", TOL)
    kw.setdefault("max_iter", MAX_ITER)
    return ops.scatter_response(p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, S, cotangent, ctx=ctx, direct=direct, **kw)


@pytest.mark.parametrize("n,n_theta,lo,hi", F.GRIDS)
def test_solve_and_outputs(ctx, n, n_theta, lo, hi):
    p = F.grid_problem(n, n_theta, lo, hi)
    S = F.solve(ctx, p).S
    direct, cot = flux_planes(ctx, p, S)
    with profiled(ctx):
        got = respond(ctx, p, S, cot, direct)
        assert ctx.profile("k_lambda_adjoint")[0] == 1 and ctx.profile_variant("k_lambda_adjoint") == "k_lambda_adjoint<true>"
    op80, op64 = R.operator(p.alphas, p.ray, p.m, L), R.operator(p.alphas, p.ray, p.m, np.float64)
    radius = R.spectral_radius(op64, p.albedo)
    keep = radius < F.RADIUS_BELOW
    print(f"{n}/{n_theta} [{lo}, {hi}]: radius {np.round(radius, 3)}, iterations {got.iterations}, status {got.status}, change {got.change}")
    assert keep[np.asarray(F.ALBEDOS + (0.0,)) <= 0.9].all() and keep[-1]  # (the filter may only ever drop albedo 0.999)
    assert (got.status == 0).all() and all(np.isfinite(getattr(got, k)).all() for k in OUTPUTS)
    counts = np.where(keep, got.iterations, 0)  # (the restatements run the kept columns only)
    it80, it64 = A.iterate(op80, p.albedo, cot, counts=counts), A.iterate(op64, p.albedo, cot, counts=counts)
    own = A.iterate(R.operator(p.alphas[:, keep], p.ray, p.m, np.float64), p.albedo[:, keep], cot[:, keep], tol=TOL, max_iter=MAX_ITER)
    yes = np.ones((n, p.n_nu), dtype=bool)
    out80, out64 = A.outputs(op80, p.albedo, p.B, S, it80["y"], direct), A.outputs(op64, p.albedo, p.B, S, it64["y"], direct)
    out80["y"], out64["y"] = it80["y"], it64["y"]
    print(f"    the restatement's own count {own['iterations']}")
    kept = np.flatnonzero(keep)
    for j, i in enumerate(kept):
        assert abs(int(got.iterations[i]) - int(own["iterations"][j])) <= 1 and own["status"][j] == 0, (i, got.iterations[i], own["iterations"][j])
    for name in OUTPUTS:
        d_gpu, d_ref = T.distance(getattr(got, name), out80[name], yes), T.distance(out64[name], out80[name], yes)
        print(f"    {name}: kernel {d_gpu[kept]}, restatement {d_ref[kept]}")
        for i in kept:
            A.RECORD.append(("k_lambda_adjoint<true>", name, n, n_theta, int(i), float(d_gpu[i]), float(d_ref[i])))
            assert d_gpu[i] <= T.bound(d_ref[i], n), (name, i, d_gpu[i], d_ref[i])
    # the fixed point: the 80-bit residual of the y the device returned, every column
    y = got.y.astype(L)
    z = p.albedo.astype(L) * y
    Lt80, Lt64 = A.transposed(op80, z), A.transposed(op64, p.albedo * got.y)
    residual = np.abs((cot.astype(L) + Lt80) - y).max(axis=0).astype(np.float64)
    d_app = T.distance(Lt64, Lt80, yes)
    allowed = TOL * np.abs(got.y).max(axis=0) + np.array([T.bound(d, n) for d in d_app]) * np.abs(Lt80).max(axis=0).astype(np.float64)
    print(f"    residual {residual}, allowed {allowed}")
    assert (residual <= allowed).all()
    # every output alone: the same bits
    for name in OUTPUTS[1:]:
        d = [ctx.upload(x) for x in (p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, p.B, S, cot, direct)]
        one = ctx.empty((n, p.n_nu))
        ptrs = {k: (one.ptr if k == name else None) for k in OUTPUTS}
        ctx.call("sdx_scatter_response_dev", n, p.n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, p.n_nu, d[5].ptr, p.n_nu, d[6].ptr, p.n_nu,
                 d[7].ptr, p.n_nu, d[8].ptr, p.n_nu, d[9].ptr, p.n_nu, TOL, MAX_ITER, ptrs["y"], p.n_nu, ptrs["R_thermal"], p.n_nu, ptrs["R_absorption"], p.n_nu,
                 ptrs["R_scatter"], p.n_nu, None, None, None)
        assert np.array_equal(one.numpy(), getattr(got, name)), name


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_theta,lo,hi", F.GRIDS)
def test_end_to_end_against_difference_quotients(ctx, n, n_theta, lo, hi):
    p = F.grid_problem(n, n_theta, lo, hi)
    keep = R.spectral_radius(R.operator(p.alphas, p.ray, p.m, np.float64), p.albedo) < F.RADIUS_BELOW
    assert keep[np.asarray(F.ALBEDOS + (0.0,)) <= 0.9].all() and keep[-1]
    dirs = A.directions(p)

    def flux(total, sc, B):
        S = ops.scatter_source(p.nus, p.temps, p.ray, p.m, total, sc, ctx=ctx, thermal=B, tol=A.TOL_DEVICE, max_iter=MAX_ITER, want_J=False)
        assert (S.status[keep] != 2).all()  # (1: at tol = 1e-13 a column may end at max_iter, on the rounding floor of its updates)
        return ops.raytrace_arrays(p.nus, p.temps, p.ray, p.weights, total, ctx=ctx, source=S.S)[0][-1], S.S

    total, sc, B = A.perturbed(p, "R_thermal", dirs["R_thermal"], 0.0, np.float64)
    Phi, S = flux(total, sc, B)
    direct, cot = flux_planes(ctx, p, S)
    got = respond(ctx, p, S, cot, direct, tol=A.TOL_DEVICE)
    planes = {name: getattr(got, name) for name in A.QUANTITIES}
    yard = A.restated_gaps(p, (n, n_theta, lo, hi), np.float64, A.H_DEVICE, tol=A.TOL_DEVICE)
    missed = []
    for name in A.QUANTITIES:
        quotient = A.richardson(lambda e: flux(*A.perturbed(p, name, dirs[name], e, np.float64))[0], A.H_DEVICE)
        value, scale = A.weighted(name, planes, p, dirs[name])
        gaps = A.gap(value, quotient, scale + np.abs(Phi))
        g, o = float(gaps[keep].max()), float(yard[name][keep].max())
        A.RECORD.append(("end to end", name, n, n_theta, "kept columns", g, o))
        print(f"{n}/{n_theta} {name}: device {gaps}, restatement {yard[name]}; kept {keep}: {g:.2e} against 2 x {o:.2e}")
        if not g <= 2 * o:
            missed.append((name, g, o))
    assert not missed, missed


# ---- 5. no scattering --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth,n_theta,n_nu", [(2, 1, 1), (9, 7, 37), (57, 20, 200)])
def test_zero_albedo(ctx, n_depth, n_theta, n_nu):
    c = T.case(n_depth, n_theta, -(-n_nu // 4), "interleaved", classes=("moderate", "thick", "ramp", "thin"))
    m = ops.mean_weights(c.thetas, c.weights)
    nus, alphas = c.nus[:n_nu], np.ascontiguousarray(c.alphas[:, :n_nu])
    S = ops.scatter_source(nus, c.temps, c.ray, m, alphas, np.zeros(n_depth), ctx=ctx).S
    direct, cot = ops.response(nus, c.temps, c.ray, c.weights, alphas, ctx=ctx, source=S)
    assert np.isfinite(direct).all() and np.isfinite(cot).all() and cot.any()
    for scatter in (np.zeros(n_depth), np.zeros((n_depth, n_nu))):
        got = ops.scatter_response(nus, c.temps, c.ray, m, alphas, scatter, S, cot, ctx=ctx, direct=direct)
        assert np.array_equal(got.y, cot) and np.array_equal(got.R_thermal, cot) and np.array_equal(got.R_absorption, direct)
        assert np.array_equal(got.R_scatter, np.zeros((n_depth, n_nu)))
        assert (got.iterations == 1).all() and (got.status == 0).all() and (got.change == 0).all()
    # no direct part: R_absorption is the opacity derivative of one application at z = 0
    got = ops.scatter_response(nus, c.temps, c.ray, m, alphas, np.zeros(n_depth), S, cot, ctx=ctx)
    assert np.array_equal(got.R_absorption, np.zeros((n_depth, n_nu))) and np.array_equal(got.y, cot)


# ---- 6. the ends of the loop ---------------------------------------------------------------------------------------------------------------
def test_max_iter_ends_the_loop(ctx):
    p = F.grid_problem(9, 7, 0.03, 30.0)
    S = F.solve(ctx, p).S
    direct, cot = flux_planes(ctx, p, S)
    got = respond(ctx, p, S, cot, direct, tol=0.0, max_iter=7)
    moving = np.asarray(F.ALBEDOS + (0.5,)) > 0  # (albedo 0 has reached its fixed point after one update: change 0 <= 0)
    print(got.iterations, got.status, got.change)
    assert (got.status[moving] == 1).all() and (got.iterations[moving] == 7).all() and (got.change[moving] > 0).all()
    assert got.status[0] == 0 and got.iterations[0] == 1
    it64 = A.iterate(R.operator(p.alphas, p.ray, p.m, np.float64), p.albedo, cot, counts=got.iterations)
    assert np.abs(got.y / it64["y"] - 1).max() <= 1e-13  # seven updates of the restatement


def test_a_divergent_column_stops_and_leaves_the_others_alone(ctx):
    """the forward test's construction: three points over [0.1, 10], one angle, albedo 0.999 in one column of 70 (the transposed
    iteration has the forward one's spectral radius, 7.7); its neighbours converge, bit for bit as they do without it"""
    thetas, weights = synth.thetas_and_weights(1)
    m = ops.mean_weights(thetas, weights)
    _, bad = R.log_grid(3, 0.1, 10.0)
    _, good = R.log_grid(3, 0.3, 3.0)
    ray = bad.reshape(-1, 1) / np.cos(thetas)
    n_nu, at = 70, 33
    alphas = np.repeat(R.alphas_for(good, bad)[:, None], n_nu, axis=1)
    alphas[:, at] = 1.0
    albedo = np.repeat(np.linspace(0.0, 0.999, n_nu)[None, :], 3, axis=0)
    albedo[:, at] = 0.999
    nus, temps = np.linspace(7.5e14, 3.0e14, n_nu), np.linspace(9500.0, 3900.0, 3)
    rng = np.random.default_rng(70)
    S, cot, direct, B = (rng.uniform(0.5, 2.0, (3, n_nu)) for _ in range(4))
    radius = R.spectral_radius(R.operator(alphas, ray, m, np.float64), albedo)
    assert radius[at] > 5 and np.delete(radius, at).max() < F.RADIUS_BELOW

    def run(cols, cot=cot):
        cut = lambda a: np.ascontiguousarray(a[:, cols])  # noqa: E731
        return ops.scatter_response(nus[cols], temps, ray, m, cut(alphas), cut(albedo * alphas), cut(S), cut(cot), ctx=ctx, direct=cut(direct), thermal=cut(B),
                                    tol=TOL, max_iter=300)

    got = run(slice(None))  # (the call returns)
    print("divergent column: status", got.status[at], "iterations", got.iterations[at], "change", got.change[at])
    assert got.status[at] in (1, 2) and np.isfinite(got.y[:, at]).all()
    others = np.arange(n_nu) != at
    assert (got.status[others] == 0).all()
    without = run(others)
    for name in EVERYTHING:
        assert np.array_equal(getattr(got, name)[..., others], getattr(without, name)), name
    # a change that is not finite: a cotangent at the top of the double range under albedo 1 — c + Lambda^T (W c) overflows in the first
    # trip, the update is refused, y stays at y^0 = c; its neighbour converges
    big = cot.copy()
    big[:, 1] = 1.7e308
    albedo2 = albedo.copy()
    albedo2[:, 1] = 1.0
    with np.errstate(all="ignore"):
        first = big[:, :2] + A.transposed(R.operator(alphas[:, :2], ray, m, np.float64), albedo2[:, :2] * big[:, :2])
    assert np.isfinite(first[:, 0]).all() and not np.isfinite(first[:, 1]).all()
    broken = ops.scatter_response(nus[:2], temps, ray, m, np.ascontiguousarray(alphas[:, :2]), np.ascontiguousarray((albedo2 * alphas)[:, :2]),
                                  np.ascontiguousarray(S[:, :2]), np.ascontiguousarray(big[:, :2]), ctx=ctx, tol=TOL, max_iter=300)
    print("overflowing column: status", broken.status, "iterations", broken.iterations, "change", broken.change)
    assert broken.status[0] == 0 and np.isfinite(broken.y[:, 0]).all()
    assert broken.status[1] == 2 and broken.iterations[1] == 1 and np.isposinf(broken.change[1]) and np.array_equal(broken.y[:, 1], big[:, 1])


def test_a_column_does_not_depend_on_its_launch(ctx):
    """200 columns on the 57-point grid at 20 angles, albedo 0 .. 0.999 in one launch: a column alone, in a shard of the grid, in the whole
    launch, twice in a row and through the host-buffer twin — the same bits"""
    n, n_nu = 57, 200
    tau, dtau = R.log_grid(n, 1e-4, 1e3)
    thetas, weights = synth.thetas_and_weights(20)
    m = ops.mean_weights(thetas, weights)
    ray = dtau.reshape(-1, 1) / np.cos(thetas)
    rng = np.random.default_rng(57)
    albedo = np.repeat(rng.permutation(np.linspace(0.0, 0.999, n_nu))[None, :], n, axis=0)
    alphas, B = np.ones((n, n_nu)), np.repeat((1.0 + tau)[:, None], n_nu, axis=1) * rng.uniform(0.5, 2.0, n_nu)
    nus, temps = np.linspace(7.5e14, 3.0e14, n_nu), np.linspace(9500.0, 3900.0, n)
    S = ops.scatter_source(nus, temps, ray, m, alphas, albedo * alphas, ctx=ctx, thermal=B, tol=TOL, max_iter=MAX_ITER, want_J=False).S
    direct, cot = ops.response(nus, temps, ray, weights, alphas, ctx=ctx, source=S)

    def run(cols):
        cut = lambda a: np.ascontiguousarray(a[:, cols])  # noqa: E731
        return ops.scatter_response(nus[cols], temps, ray, m, cut(alphas), cut(albedo * alphas), cut(S), cut(cot), ctx=ctx, direct=cut(direct), thermal=cut(B),
                                    tol=TOL, max_iter=MAX_ITER)

    whole = run(slice(None))
    print("iterations", whole.iterations.min(), "..", whole.iterations.max())
    assert (whole.status == 0).all() and whole.iterations.min() == 1 and whole.iterations.max() > 300
    again = run(slice(None))
    shard = run(slice(60, 137))
    for name in EVERYTHING:
        assert np.array_equal(getattr(again, name), getattr(whole, name)), name
        assert np.array_equal(getattr(shard, name), getattr(whole, name)[..., 60:137]), name
    for k in (0, 59, 136, 199, int(np.argmax(whole.iterations))):
        alone = run(slice(k, k + 1))
        for name in EVERYTHING:
            assert np.array_equal(getattr(alone, name), getattr(whole, name)[..., k:k + 1]), (name, k)
    # the host-buffer twins
    ptr = lambda a: a.ctypes.data  # noqa: E731
    h = [np.ascontiguousarray(a, dtype=np.float64) for a in (nus, temps, ray, m, alphas, albedo * alphas, B, S, cot, direct)]
    out = {name: np.full((n, n_nu), np.nan) for name in OUTPUTS}
    out.update(iterations=np.full(n_nu, -1, dtype=np.int32), status=np.full(n_nu, -1, dtype=np.int32), change=np.full(n_nu, np.nan))
    ctx.call("sdx_scatter_response_f64", n, n_nu, 20, *(ptr(a) for a in h[:6]), 1, ptr(h[6]), ptr(h[7]), ptr(h[8]), ptr(h[9]), TOL, MAX_ITER,
             *(ptr(out[name]) for name in EVERYTHING))
    for name in EVERYTHING:
        assert np.array_equal(out[name], getattr(whole, name)), name
    z = rng.uniform(-1.0, 1.0, (n, n_nu))
    Ld, Gd = ops.mean_intensity_adjoint(nus, temps, ray, m, alphas, z, ctx=ctx, source=S)
    Lh, Gh = np.full((n, n_nu), np.nan), np.full((n, n_nu), np.nan)
    ctx.call("sdx_mean_intensity_adjoint_f64", n, n_nu, 20, *(ptr(a) for a in h[:5]), ptr(z), ptr(h[7]), ptr(Lh), ptr(Gh))
    assert np.array_equal(Lh, Ld) and np.array_equal(Gh, Gd)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    p = F.grid_problem(9, 7, 0.03, 30.0)
    n = p.n_nu
    d = [ctx.upload(a) for a in (p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo, p.B)]
    out = ctx.empty((9, n))

    def solve(n_depth=9, n_theta=7, n_nu=n, tol=TOL, max_iter=10, y=out.ptr, S=d[6].ptr):
        ctx.call("sdx_scatter_response_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, d[5].ptr, n, d[6].ptr, n, S, n,
                 d[6].ptr, n, None, 0, tol, max_iter, y, n, None, 0, None, 0, None, 0, None, None, None)

    def apply(n_depth=9, n_theta=7, n_nu=n, Lt=out.ptr, z=d[6].ptr):
        ctx.call("sdx_mean_intensity_adjoint_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, z, n, None, 0, Lt, n, None, 0)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for call in (solve, apply):
                for n_nu in (n, 0):  # also at set-up time, with an empty grid
                    with pytest.raises(ValueError, match="mixed_precision"):
                        call(n_nu=n_nu)
        finally:
            ctx.set_option("mixed_precision", 0)
        for call in (solve, apply):
            for n_nu in (n, 0):
                with pytest.raises(ValueError, match="64 angles"):
                    call(n_theta=65, n_nu=n_nu)
                with pytest.raises(ValueError, match="deep"):
                    call(n_depth=500, n_nu=n_nu)  # (17 n_depth + 21 doubles at seven angles and one frequency per wave: above 64 KB from 481)
                call(n_depth=9, n_nu=0)
        for n_nu in (n, 0):
            for kw in (dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=0)):
                with pytest.raises(ValueError, match="tol >= 0"):
                    solve(n_nu=n_nu, **kw)
        with pytest.raises(ValueError, match="null pointer"):
            solve(S=None)
        with pytest.raises(ValueError, match="null pointer"):
            apply(z=None)
        with pytest.raises(ValueError, match="no output"):
            solve(y=None)
        with pytest.raises(ValueError, match="no output"):
            apply(Lt=None)
        ctx.synchronize()
        assert ctx.profile("k_lambda_adjoint")[0] == 0
        solve()  # and the context still serves
        apply()
        ctx.synchronize()
        assert ctx.profile("k_lambda_adjoint")[0] == 2


# ---- 8. the engine -------------------------------------------------------------------------------------------------------------------------
def test_engine(ctx):
    import line_adjoint_truth as LA
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    m = F.small_model()
    n_depth, n_nu, n_lines = 12, 300, 40
    x_lines = np.arange(0, n_lines, 3)
    ray = m.atm["dist"].reshape(-1, 1) / np.cos(m.thetas)
    mw = ops.mean_weights(m.thetas, m.weights)
    # without both options: what it launched; the keywords at their default give today's arrays
    plain = F.synthesizer(ctx, m, keep_response=True)
    with profiled(ctx):
        plain.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda_adjoint")[0] == 0 and ctx.profile("k_lambda")[0] == 0 and ctx.profile("k_response")[0] == 1
    Ra_lte = np.array(plain.response_opacity.numpy())
    only_x = {k: np.ascontiguousarray(v[x_lines]) for k, v in m.lines.items()}
    side = F.synthesizer(ctx, m, keep_line=True, scattering=True)  # (scattering without keep_response: no adjoint either)
    with profiled(ctx):
        side.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda_adjoint")[0] == 0 and ctx.profile("k_lambda")[0] == 1 and ctx.profile("k_response")[0] == 0
    assert not hasattr(side, "d_sc_Ra")
    with pytest.raises(RuntimeError, match="keep_response=True"):
        side.scattering_response_opacity
    with pytest.raises(RuntimeError, match="keep_response=True"):
        plain.flux_derivative(np.ones((n_depth, n_nu)), scattering=True)
    side.close()
    x_syn = SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, only_x, m.cont, ctx=ctx, track_evaluations=False, keep_line=True)
    x_syn.step()
    ctx.synchronize()
    alpha_x = np.array(x_syn.alpha_line())
    x_syn.close()
    w = np.random.default_rng(1).standard_normal(n_nu)
    lte_derivative = np.array(plain.flux_derivative(alpha_x).numpy())
    lte_sens = np.array(plain.line_sensitivities(w).numpy())
    assert np.array_equal(plain.flux_derivative(alpha_x, scattering=False).numpy(), lte_derivative)
    assert np.array_equal(plain.line_sensitivities(w, scattering=False).numpy(), lte_sens)
    plain.close()

    syn = F.synthesizer(ctx, m, scattering=True, keep_response=True)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda_adjoint")[0] == 1 and ctx.profile("k_lambda")[0] == 1 and ctx.profile("k_response")[0] == 2
    assert np.array_equal(syn.response_opacity.numpy(), Ra_lte)  # the LTE planes stay what they were
    assert np.array_equal(syn.flux_derivative(alpha_x).numpy(), lte_derivative) and np.array_equal(syn.line_sensitivities(w).numpy(), lte_sens)
    total, S, Fsc = np.array(syn.total_alphas()), np.array(syn.scattering_source.numpy()), np.array(syn.scattering_flux.numpy())
    planes = {k: np.array(getattr(syn, "scattering_response_" + k).numpy()) for k in ("opacity", "thermal", "scatter")}
    iterations, status = syn.scattering_response_iterations, syn.scattering_response_status
    print("adjoint iterations", iterations.min(), "..", iterations.max(), "| forward", syn.scattering_iterations.min(), "..", syn.scattering_iterations.max())
    assert (status == 0).all() and iterations.dtype == status.dtype == np.int32 and planes["opacity"].shape == (n_depth, n_nu)
    assert not np.array_equal(planes["opacity"], Ra_lte)
    # the ops path on the step's own planes
    thomson = ops.alpha_electron(1, m.cont["n_e"], ctx=ctx).numpy().reshape(-1)
    direct, cot = ops.response(m.nus, m.atm["temperatures"], ray, m.weights, total, ctx=ctx, source=S)
    got = ops.scatter_response(m.nus, m.atm["temperatures"], ray, mw, total, thomson, S, cot, ctx=ctx, direct=direct)
    assert np.array_equal(got.R_absorption, planes["opacity"]) and np.array_equal(got.R_thermal, planes["thermal"]) and np.array_equal(got.R_scatter, planes["scatter"])
    assert np.array_equal(got.iterations, iterations) and np.array_equal(got.status, status)
    # the solver-level twin on plain namespaces
    stellar_model = types.SimpleNamespace(spherical=False, temperatures=m.atm["temperatures"], geometry=types.SimpleNamespace(dist_to_next_depth_point=m.atm["dist"]))
    entries = dict(alpha_rayleigh=0, alpha_electron=ops.alpha_electron(n_nu, m.cont["n_e"], ctx=ctx).numpy())
    field = types.SimpleNamespace(thetas=m.thetas, I_nus_weights=m.weights, frequencies=m.nus, opacities=types.SimpleNamespace(total_alphas=total, opacities_dict=entries))
    twin = rfs.scattering_response(stellar_model, field)
    assert np.array_equal(twin.S, S) and np.array_equal(twin.R_absorption, planes["opacity"]) and np.array_equal(twin.iterations, iterations)
    with pytest.raises(NotImplementedError):
        rfs.scattering_response(types.SimpleNamespace(spherical=True), field)
    # flux_derivative(scattering=True) against a central difference of scattering_flux over two steps, the strengths of the lines of X
    # scaled by exp(+-h), h = 1e-3.  A central difference of a flux is no clean judge of a derivative AT FIXED WINDOWS: a line's window is
    # an integer function of its strength, and the flux steps where it moves (tests/test_gpu_response.py judges the LTE derivative against
    # extrapolated differences on a thickened model for that reason).  The same two steps also give F_nu, so the LTE derivative — judged
    # there — measures what the difference is worth here, column by column: the scattering derivative may miss its quotient by twice what
    # the LTE one misses its own by, plus the difference's noise (the flux's rounding in thin gaps, 1e-11 of the flux, over h).  What
    # scattering CHANGES is judged apart, where the window steps cancel: (scattering - LTE) of the derivatives against (scattering - LTE)
    # of the quotients, within 2 % of the largest change (the steps' and the truncation's share of it: both are of the relative size of
    # the change itself, 1e-5) plus the noise of two fluxes.
    derivative = np.array(syn.flux_derivative(alpha_x, scattering=True).numpy())
    h, flux, flux_lte = 1e-3, {}, {}
    for sign in (1, -1):
        lines = {k: v.copy() for k, v in m.lines.items()}
        lines["alphas"][x_lines] *= np.exp(sign * h)
        moved = SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, lines, m.cont, ctx=ctx, track_evaluations=False, scattering=True)
        moved.step()
        ctx.synchronize()
        flux[sign], flux_lte[sign] = np.array(moved.scattering_flux.numpy()), np.array(moved.F_nu()[-1])
        moved.close()
    quotient, quotient_lte = (flux[1] - flux[-1]) / (2 * h), (flux_lte[1] - flux_lte[-1]) / (2 * h)
    noise = 1e-11 * np.abs(Fsc).max() / h
    allowed = 2 * np.abs(lte_derivative - quotient_lte) + noise
    change, change_quotient = derivative - lte_derivative, quotient - quotient_lte
    allowed_change = 0.02 * np.abs(change).max() + 2 * noise
    print(f"flux_derivative(scattering=True): max |analytic - quotient| {np.abs(derivative - quotient).max():.3e}, LTE's own {np.abs(lte_derivative - quotient_lte).max():.3e}, "
          f"worst ratio to the allowance {(np.abs(derivative - quotient) / allowed).max():.3f}; largest derivative {np.abs(derivative).max():.3e}; what scattering "
          f"changes: {np.abs(change).max():.3e}, missed by {np.abs(change - change_quotient).max():.3e}, allowed {allowed_change:.3e}")
    assert (np.abs(derivative - quotient) <= allowed).all() and np.abs(derivative).max() > 100 * noise
    assert (np.abs(change - change_quotient) <= allowed_change).all() and np.abs(change).max() > 20 * noise  # (the change is seen: neither check is passed by LTE's plane)
    # line_sensitivities(scattering=True) against flux_derivative of the single-line planes, a handful of lines, strength and shape alike
    # in what they consume: the weight plane
    sens = np.array(syn.line_sensitivities(w, scattering=True).numpy())
    assert sens.shape == (n_lines,) and not np.array_equal(sens, lte_sens)
    for l in (0, 7, 19, 33, 39):
        one = [np.ascontiguousarray(m.lines[k][l:l + 1]) for k in ("line_nus", "doppler_widths", "gammas", "alphas")]
        plane = ops.calc_alan_entries(n_depth, m.nus, *one, ctx=ctx)
        expect = float((w * syn.flux_derivative(plane, scattering=True).numpy()).sum())
        bound = (2 * LA.OPACITY_RTOL + n_depth * n_nu * LA.EPS) * float(np.abs(w[None, :] * planes["opacity"] * (plane / total)).sum())
        assert abs(sens[l] - expect) <= bound, (l, sens[l], expect, bound)
    shapes = syn.line_sensitivities(w, wrt=("damping", "doppler"), scattering=True)
    assert all(np.isfinite(v.numpy()).all() for v in shapes.values())
    assert not np.array_equal(shapes["damping"].numpy(), syn.line_sensitivities(w, wrt="damping").numpy())
    # recorded and replayed
    syn.capture()
    for a in (syn.scattering_response_opacity, syn.scattering_response_thermal, syn.scattering_response_scatter):
        a.zero()
    syn.step()
    ctx.synchronize()
    for k, v in planes.items():
        assert np.array_equal(getattr(syn, "scattering_response_" + k).numpy(), v), k
    assert np.array_equal(syn.scattering_response_iterations, iterations) and np.array_equal(syn.scattering_flux.numpy(), Fsc)
    syn.close()
    # a frequency shard: its own columns
    part = F.synthesizer(ctx, m, scattering=True, keep_response=True, shard=(100, 120))
    part.step()
    ctx.synchronize()
    assert np.array_equal(part.scattering_response_opacity.numpy(), planes["opacity"][:, 100:220])
    part.close()
