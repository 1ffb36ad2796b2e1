"""Ng acceleration of the scattering source iteration on the device (sdx_scatter_source_ng_dev and its host-buffer twin,
ops.scatter_source(acceleration=), radiation_field_solvers.scattering_source(acceleration=), SpectralSynthesizer(scattering=
dict(acceleration="ng"))).  The plain entry point is existing code and the yardstick: the accelerated solve is judged against it on
the columns of scattering_ng_reference.NG_COLUMNS, by the conditions tests/test_scattering_ng_cpu.py states, on the device's own counts.

    fixed point   S within 4 x the plain device solve's distance from the long-double direct solve, per column
    statuses      0 wherever the plain device solve has it
    updates       never more than the plain solve's plus 2 x period; at most half of them on the columns with uniform albedo >= 0.99
                  of the 57-point grids that the plain solve brings to status 0
    counts        iterations within one of the fp64 restatement's own (the slack tests/test_gpu_scattering.py allows itself, on the
                  columns its radius filter keeps), accelerations within one — on the columns whose albedo stays within that test's own
                  range, <= 0.999.  Above it the trip at which a column meets tol = 1e-12 is decided by rounding: one rounding error of
                  J, 1e-16, is amplified by up to 1 / (1 - albedo) = 1e4 .. 1e5 to 1e-12 .. 1e-11 of S, the size of the threshold
                  itself (seen: 9 x 7 at albedo 0.99999, device 51 updates, restatement 53; every other column of the set agrees
                  exactly).  Those columns keep the other checks.
The adjoint solve has no accelerated entry (test_scattering_ng_cpu.py, test_no_safeguard_keeps_the_adjoint_within_the_plain_cost): the end-to-end
check runs the plain adjoint on the accelerated S.  Every test prints its figures before it asserts."""
import functools
import types

import numpy as np
import pytest

import scattering_adjoint_reference as A
import scattering_ng_reference as N
import scattering_reference as R
import test_gpu_scattering as F  # profiled, small_model, synthesizer: imported, not edited
from stardis_amd import ops, synth

pytestmark = pytest.mark.gpu

L = R.L
TOL, MAX_ITER, PERIOD = N.TOL, N.MAX_ITER, N.DEFAULTS["period"]
HIGH = ("0.99", "0.999", "0.9999", "0.99999")
FEW = [("0.5", "flat"), ("0.9", "planck-like"), ("0.99", "flat"), ("rising", "flat"), ("random", "planck-like")]
# (points, tau range, angles, columns): the column set at 57 points; then the smallest shapes — 9 x 7, and 4, 3 and 2 points at one
# angle, the last with fewer points than the history has iterates
SHAPES = [(57, 1e-4, 1e3, 3, None), (57, 1e-4, 1e3, 20, None), (57, 1e-6, 1e2, 3, None), (57, 1e-6, 1e2, 20, None), (9, 1e-2, 1e2, 7, None),
          (4, 0.1, 10.0, 1, None), (3, 0.3, 3.0, 1, FEW), (2, 0.3, 3.0, 1, FEW)]


@pytest.fixture(autouse=True)
def extended_precision():
    if not R.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def solve(ctx, p, acceleration=None, **kw):
    kw.setdefault("thermal", p.B)
    kw.setdefault("tol", TOL)
    kw.setdefault("max_iter", MAX_ITER)
    return ops.scatter_source(p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, ctx=ctx, acceleration=acceleration, **kw)


@functools.lru_cache(maxsize=None)
def truth(n, lo, hi, n_theta, columns):
    """the long-double direct solutions of a shape's columns (one grid: the dense operator once): computed once, left unchanged"""
    p = N.problem(n, lo, hi, n_theta, columns=None if columns is None else list(columns))
    lam = R.operator(p.alphas[:, :1], p.ray, p.m, L).matrix()[:, :, 0]
    w, B = p.albedo.astype(L), p.B.astype(L)
    S = np.stack([R.solve(np.eye(n, dtype=L) - w[:, i][:, None] * lam, (1 - w[:, i]) * B[:, i]) for i in range(p.n_nu)], axis=1)
    S.setflags(write=False)
    return p, S


def distance(x, exact):
    return (np.abs(x.astype(L) - exact).max(axis=0) / np.abs(exact).max(axis=0)).astype(np.float64)


# ---- 1. the conditions, on the device's own counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lo,hi,n_theta,columns", SHAPES, ids=[f"{s[0]}x{s[3]} [{s[1]:g}, {s[2]:g}]" for s in SHAPES])
def test_fixed_point_statuses_and_updates(ctx, n, lo, hi, n_theta, columns):
    p, S80 = truth(n, lo, hi, n_theta, None if columns is None else tuple(columns))
    plain = solve(ctx, p)
    with F.profiled(ctx):
        ng = solve(ctx, p, "ng")
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda_ng"
    print(f"plain {plain.iterations.tolist()} status {plain.status.tolist()}\nng    {ng.iterations.tolist()} status {ng.status.tolist()}\n"
          f"acc   {ng.accelerations.tolist()}")
    assert ng.accelerations.dtype == np.int32 and np.isfinite(ng.S).all()
    solved = plain.status == 0
    assert (ng.status[solved] == 0).all(), ("statuses", p.columns)
    assert (ng.iterations <= plain.iterations + 2 * PERIOD).all(), ("condition 3", (ng.iterations - plain.iterations).tolist())
    d_plain, d_ng = distance(plain.S, S80), distance(ng.S, S80)
    print(f"distance from the direct solve: plain {d_plain}\n                      accelerated {d_ng}")
    assert (d_ng[solved] <= 4 * d_plain[solved]).all(), ("fixed point", (d_ng / d_plain)[solved])
    if n == 57:
        high = np.array([a in HIGH for a, _ in p.columns]) & solved
        print("accelerated / plain updates, albedo >= 0.99:", np.round(ng.iterations[high] / plain.iterations[high], 2).tolist())
        assert high.sum() >= 7 and (2 * ng.iterations[high] <= plain.iterations[high]).all()  # fails without the feature
    # J is the mean intensity of the returned S: the one-application kernel on it, bit for bit
    J_of_S, _ = ops.mean_intensity(p.nus, p.temps, p.ray, p.m, p.alphas, ctx=ctx, source=ng.S, want_L=False)
    assert np.array_equal(ng.J, J_of_S)
    # the counts against the fp64 restatement's own, where the plain test compares them (its radius filter) and the restatement is quick
    op64 = R.operator(p.alphas, p.ray, p.m, np.float64)
    keep = np.flatnonzero((R.spectral_radius(op64, p.albedo) < F.RADIUS_BELOW) & (ng.iterations <= 80) & (p.albedo.max(axis=0) <= 0.999))
    if n >= 4 and keep.size:
        own = N.scatter_source_ng(R.operator(p.alphas[:, keep], p.ray, p.m, np.float64), p.albedo[:, keep], p.B[:, keep], TOL, MAX_ITER, dict(lanes=n_theta))
        print(f"columns {keep.tolist()}: the restatement's own iterations {own['iterations'].tolist()} accelerations {own['accelerations'].tolist()}")
        assert (own["status"] == 0).all() and (ng.status[keep] == 0).all()
        assert (np.abs(own["iterations"] - ng.iterations[keep]) <= 1).all() and (np.abs(own["accelerations"] - ng.accelerations[keep]) <= 1).all()
        at = N.scatter_source_ng(R.operator(p.alphas[:, keep], p.ray, p.m, np.float64), p.albedo[:, keep], p.B[:, keep], options=dict(lanes=n_theta),
                                 counts=ng.iterations[keep])
        rel = np.abs(at["S"] / ng.S[:, keep] - 1).max(axis=0)
        print(f"    at the device's counts: accelerations {at['accelerations'].tolist()}, S apart by {rel}")
        assert (np.abs(at["accelerations"] - ng.accelerations[keep]) <= 1).all()


def test_the_three_point_grid_where_the_plain_iteration_diverges(ctx):
    p, S80 = truth(3, 0.1, 10.0, 1, (("0.999", "flat"), ("0.5", "flat")))
    got = solve(ctx, p, "ng", max_iter=300)
    d = distance(got.S, S80)
    print(got.iterations, got.status, got.accelerations, d)
    assert np.isfinite(got.S).all() and (got.status[0] != 0 or d[0] <= 1e-9) and got.status[1] == 0


# ---- 2. the plain adjoint on the accelerated S: end to end ------------------------------------------------------------------------------------
def test_end_to_end_against_a_difference_quotient(ctx):
    p = N.problem(57, 1e-4, 1e3, 3, columns=[("0.9", "flat")])
    dirs = A.directions(p)
    name = "R_absorption"

    def flux(total, sc, B):
        S = ops.scatter_source(p.nus, p.temps, p.ray, p.m, total, sc, ctx=ctx, thermal=B, tol=A.TOL_DEVICE, max_iter=MAX_ITER, want_J=False, acceleration="ng")
        assert (S.status != 2).all() and S.accelerations.all()
        return ops.raytrace_arrays(p.nus, p.temps, p.ray, p.weights, total, ctx=ctx, source=S.S)[0][-1], S.S

    total, sc, B = A.perturbed(p, name, dirs[name], 0.0, np.float64)
    Phi, S = flux(total, sc, B)
    direct, cot = ops.response(p.nus, p.temps, p.ray, p.weights, p.alphas, ctx=ctx, source=S)
    got = ops.scatter_response(p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, S, cot, ctx=ctx, direct=direct, thermal=p.B, tol=A.TOL_DEVICE,
                               max_iter=MAX_ITER)
    yard = A.restated_gaps(p, ("ng", 57, 3), np.float64, A.H_DEVICE, tol=A.TOL_DEVICE)
    quotient = A.richardson(lambda e: flux(*A.perturbed(p, name, dirs[name], e, np.float64))[0], A.H_DEVICE)
    value, scale = A.weighted(name, {name: got.R_absorption}, p, dirs[name])
    gap = A.gap(value, quotient, scale + np.abs(Phi))
    print(f"{name}: device {gap}, restatement {yard[name]}")
    assert (gap <= 2 * yard[name]).all()


# ---- 3. independence and determinism ---------------------------------------------------------------------------------------------------------
def test_a_column_does_not_depend_on_its_launch(ctx):
    """200 columns on the 57-point grid at 20 angles, albedo 0 .. 0.999 (1 to about 85 updates in one launch, the columns of a wave
    extrapolating, judged and stopping at different trips): a column alone, in a shard, in the whole launch, twice in a row and through
    the host-buffer twin — the same bits"""
    n, n_nu = 57, 200
    tau, dtau = R.log_grid(n, 1e-4, 1e3)
    thetas, weights = synth.thetas_and_weights(20)
    m = ops.mean_weights(thetas, weights)
    ray = dtau.reshape(-1, 1) / np.cos(thetas)
    rng = np.random.default_rng(57)
    albedo = np.repeat(rng.permutation(np.linspace(0.0, 0.999, n_nu))[None, :], n, axis=0)  # (fast and slow columns share every wave)
    alphas, B = np.ones((n, n_nu)), np.repeat((1.0 + tau)[:, None], n_nu, axis=1) * rng.uniform(0.5, 2.0, n_nu)
    nus, temps = np.linspace(7.5e14, 3.0e14, n_nu), np.linspace(9500.0, 3900.0, n)
    names = ("S", "J", "iterations", "status", "change", "accelerations")

    def run(cols):
        cut = lambda a: np.ascontiguousarray(a[:, cols])  # noqa: E731
        return ops.scatter_source(nus[cols], temps, ray, m, cut(alphas), cut(albedo * alphas), ctx=ctx, thermal=cut(B), tol=TOL, max_iter=MAX_ITER,
                                  acceleration="ng")

    whole = run(slice(None))
    print("iterations", whole.iterations.min(), "..", whole.iterations.max(), "accelerations", whole.accelerations.min(), "..", whole.accelerations.max())
    assert (whole.status == 0).all() and whole.iterations.min() == 1 and whole.iterations.max() > 60 and whole.accelerations.max() > 10
    assert whole.accelerations.min() == 0
    again = run(slice(None))
    shard = run(slice(60, 137))
    for name in names:
        assert np.array_equal(getattr(again, name), getattr(whole, name)), name
        assert np.array_equal(getattr(shard, name), getattr(whole, name)[..., 60:137]), name
    for k in (0, 59, 136, 199, int(np.argmax(whole.iterations)), int(np.argmin(whole.iterations))):
        alone = run(slice(k, k + 1))
        for name in names:
            assert np.array_equal(getattr(alone, name), getattr(whole, name)[..., k:k + 1]), (name, k)
    # the host-buffer twin, with every output and with S alone
    ptr = lambda a: a.ctypes.data  # noqa: E731
    h = [np.ascontiguousarray(a, dtype=np.float64) for a in (nus, temps, ray, m, alphas, albedo * alphas, B)]
    S, J, change = np.full((n, n_nu), np.nan), np.full((n, n_nu), np.nan), np.full(n_nu, np.nan)
    iterations, status, accelerations = (np.full(n_nu, -1, dtype=np.int32) for _ in range(3))
    head = (n, n_nu, 20, ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]), ptr(h[4]), ptr(h[5]), 1, ptr(h[6]), TOL, MAX_ITER)
    ctx.call("sdx_scatter_source_ng_f64", *head, ptr(S), ptr(J), ptr(iterations), ptr(status), ptr(change), 4, 4, ptr(accelerations))
    for name, value in zip(names, (S, J, iterations, status, change, accelerations)):
        assert np.array_equal(value, getattr(whole, name)), name
    S2 = np.full((n, n_nu), np.nan)
    ctx.call("sdx_scatter_source_ng_f64", *head, ptr(S2), None, None, None, None, 4, 4, None)
    assert np.array_equal(S2, S)
    # other options are another sequence, stopped by the same rule
    other = ops.scatter_source(nus, temps, ray, m, alphas, albedo * alphas, ctx=ctx, thermal=B, tol=TOL, max_iter=MAX_ITER, acceleration=dict(start=6, period=3))
    assert (other.status == 0).all() and not np.array_equal(other.iterations, whole.iterations)


# ---- 4. the plain path ----------------------------------------------------------------------------------------------------------------------
def test_without_the_option_it_is_the_plain_call(ctx):
    p = N.problem(9, 1e-2, 1e2, 7)
    with F.profiled(ctx):
        got = solve(ctx, p, None)
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda<true>"
    assert not hasattr(got, "accelerations")
    n = p.n_nu
    d = [ctx.upload(a) for a in (p.nus, p.temps, p.ray, p.m, p.alphas, p.albedo * p.alphas, p.B)]
    S, J, change = ctx.empty((9, n)), ctx.empty((9, n)), ctx.empty((n,))
    iterations, status = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32)
    ctx.call("sdx_scatter_source_dev", 9, n, 7, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, d[5].ptr, n, d[6].ptr, n, TOL, MAX_ITER, S.ptr, n, J.ptr, n,
             iterations.ptr, status.ptr, change.ptr)
    for name, value in (("S", S), ("J", J), ("iterations", iterations), ("status", status), ("change", change)):
        assert np.array_equal(value.numpy(), getattr(got, name)), name
    # a column that stops before the first extrapolation is due takes the plain updates alone: the plain solve's bits
    ng = solve(ctx, p, dict(start=4000, period=4))
    assert not ng.accelerations.any()
    for name in ("S", "J", "iterations", "status", "change"):
        assert np.array_equal(getattr(ng, name), getattr(got, name)), name


# ---- 5. limits and refusals -------------------------------------------------------------------------------------------------------------------
def test_the_deepest_model_runs_and_one_more_point_is_refused(ctx):
    n, n_theta = 809, 20
    tau, dtau = R.log_grid(n, 1e-4, 1e3)
    thetas, weights = synth.thetas_and_weights(n_theta)
    m, ray = ops.mean_weights(thetas, weights), dtau.reshape(-1, 1) / np.cos(thetas)
    nus, temps = np.array([5e14]), np.linspace(9500.0, 3900.0, n)
    ones = np.ones((n, 1))
    kw = dict(ctx=ctx, thermal=ones, tol=1e-10, max_iter=400)
    plain = ops.scatter_source(nus, temps, ray, m, ones, 0.9 * ones, **kw)
    ng = ops.scatter_source(nus, temps, ray, m, ones, 0.9 * ones, acceleration="ng", **kw)
    print("809 points: plain", plain.iterations, plain.status, "accelerated", ng.iterations, ng.status, ng.accelerations, np.abs(ng.S / plain.S - 1).max())
    assert plain.status[0] == 0 and ng.status[0] == 0 and ng.accelerations[0] >= 1 and ng.iterations[0] <= plain.iterations[0]
    assert np.abs(ng.S / plain.S - 1).max() <= 1e-7  # (two sequences stopped at 1e-10 of a fixed point whose error propagation has radius ~0.7)
    d = [ctx.upload(a) for a in (nus, temps, ray, m, ones, 0.9 * ones)]
    out = ctx.empty((n, 1))

    def iterate(n_depth=n, n_nu=1, start=4, period=4, S=out.ptr):
        ctx.call("sdx_scatter_source_ng_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, 1, d[5].ptr, 1, None, 0, 1e-10, 5, S, 1,
                 None, 0, None, None, None, start, period, None)

    with F.profiled(ctx):
        for n_nu in (1, 0):  # also at set-up time, with an empty grid
            with pytest.raises(ValueError, match="sdx_scatter_source_dev"):
                iterate(n_depth=n + 1, n_nu=n_nu)  # (the message names the plain entry point, which serves 1352)
            for bad in (dict(start=3), dict(period=0)):
                with pytest.raises(ValueError, match="ng_start >= 4"):
                    iterate(n_nu=n_nu, **bad)
            with pytest.raises(ValueError, match="64 angles"):
                ctx.call("sdx_scatter_source_ng_dev", 9, n_nu, 65, None, None, None, None, None, 0, None, 0, None, 0, 1e-10, 5, None, 0, None, 0, None, None, None,
                         4, 4, None)
        ctx.set_option("mixed_precision", 1)
        try:
            with pytest.raises(ValueError, match="mixed_precision"):
                iterate()
        finally:
            ctx.set_option("mixed_precision", 0)
        with pytest.raises(ValueError, match="null pointer"):
            iterate(S=None)
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 0
        iterate()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 1


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------------------
def test_engine(ctx):
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    m = F.small_model()
    plain = F.synthesizer(ctx, m, scattering=True)
    with F.profiled(ctx):
        plain.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda<true>"
    assert not hasattr(plain, "d_sc_accelerations") and plain.scattering == dict(tol=1e-12, max_iter=2000)
    with pytest.raises(RuntimeError, match='acceleration="ng"'):
        plain.scattering_accelerations
    S0, F0, it0, total = plain.scattering_source.numpy(), np.array(plain.scattering_flux.numpy()), plain.scattering_iterations, np.array(plain.total_alphas())
    plain.close()
    with pytest.raises(ValueError, match="acceleration"):
        F.synthesizer(ctx, m, scattering=dict(acceleration="anderson"))
    syn = F.synthesizer(ctx, m, scattering=dict(acceleration="ng"))
    with F.profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile("k_lambda")[0] == 1 and ctx.profile_variant("k_lambda") == "k_lambda_ng"
    S, Fs, acc, its = syn.scattering_source.numpy(), np.array(syn.scattering_flux.numpy()), syn.scattering_accelerations, syn.scattering_iterations
    print("iterations", its.min(), "..", its.max(), "accelerations", acc.min(), "..", acc.max(), "flux apart by", np.abs(Fs / F0 - 1).max())
    assert np.abs(Fs / F0 - 1).max() <= 1e-10 and (syn.scattering_status == 0).all()
    # the Thomson albedo of the solar model: every column stops before the first extrapolation is due — the plain solve's updates, its bits
    assert acc.dtype == np.int32 and not acc.any() and its.max() < 4
    assert np.array_equal(S, S0) and np.array_equal(Fs, F0) and np.array_equal(its, it0)
    # recorded and replayed
    syn.capture()
    for a in (syn.scattering_source, syn.d_Fsc):
        a.zero()
    syn.d_sc_accelerations.set(np.full(acc.shape, 7, dtype=np.int32))  # (part of the capture: the replay writes the zeros again)
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.scattering_source.numpy(), S) and np.array_equal(syn.scattering_flux.numpy(), Fs) and np.array_equal(syn.scattering_accelerations, acc)
    syn.close()
    # a replayed graph whose columns DO extrapolate: the same engine with its per-depth scattering vector raised to 0.98 of the smallest
    # total opacity of each depth (albedo up to 0.98) — ring reads, the five sums and the safeguard's registers under a capture
    hot = F.synthesizer(ctx, m, scattering=dict(acceleration="ng"))
    hot.d_thomson.set(0.98 * total.min(axis=1))
    hot.step()
    ctx.synchronize()
    want = {k: np.array(getattr(hot, k).numpy()) for k in ("scattering_source", "scattering_mean_intensity", "scattering_flux")}
    acc_hot, its_hot = hot.scattering_accelerations, hot.scattering_iterations
    print("raised albedo: iterations", its_hot.min(), "..", its_hot.max(), "accelerations", acc_hot.min(), "..", acc_hot.max())
    assert (hot.scattering_status == 0).all() and acc_hot.max() >= 3 and (acc_hot > 0).sum() >= acc_hot.size // 2
    hot.capture()
    for a in (hot.scattering_source, hot.scattering_mean_intensity, hot.d_Fsc):
        a.zero()
    hot.d_sc_accelerations.set(np.full(acc_hot.shape, 7, dtype=np.int32))
    hot.d_sc_iterations.set(np.full(acc_hot.shape, 7, dtype=np.int32))
    for _ in range(2):
        hot.step()
    ctx.synchronize()
    for k, v in want.items():
        assert np.array_equal(getattr(hot, k).numpy(), v), k
    assert np.array_equal(hot.scattering_accelerations, acc_hot) and np.array_equal(hot.scattering_iterations, its_hot)
    hot.close()
    # the solver-level twin on columns that extrapolate: the Thomson opacity scaled up through the solver-level twin on the step's total_alphas
    ray = m.atm["dist"].reshape(-1, 1) / np.cos(m.thetas)
    stellar_model = types.SimpleNamespace(spherical=False, temperatures=m.atm["temperatures"], geometry=types.SimpleNamespace(dist_to_next_depth_point=m.atm["dist"]))
    entries = dict(alpha_rayleigh=0, alpha_electron=0.98 * total)
    field = types.SimpleNamespace(thetas=m.thetas, I_nus_weights=m.weights, frequencies=m.nus, opacities=types.SimpleNamespace(total_alphas=total, opacities_dict=entries))
    twin_plain, twin = rfs.scattering_source(stellar_model, field), rfs.scattering_source(stellar_model, field, acceleration="ng")
    direct = ops.scatter_source(m.nus, m.atm["temperatures"], ray, ops.mean_weights(m.thetas, m.weights), total, 0.98 * total, ctx=ctx, acceleration="ng")
    print("albedo 0.98 on the model: plain", twin_plain.iterations.max(), "accelerated", twin.iterations.max(), "accelerations", twin.accelerations.max())
    assert (twin.status == 0).all() and twin.accelerations.all() and np.array_equal(twin.S, direct.S) and np.array_equal(twin.accelerations, direct.accelerations)
    assert np.abs(twin.S / twin_plain.S - 1).max() <= 1e-9 and (twin.iterations <= twin_plain.iterations + 2 * PERIOD).all()
