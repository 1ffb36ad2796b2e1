"""Response functions on the device (sdx_response_dev, sdx_response_f64, sdx_response_project_dev,
SpectralSynthesizer(keep_response=True), ops.response, radiation_field_solvers.response_functions).

The kernel is judged as every kernel of the formal solution is (tests/test_gpu_formal_solution_truth.py): per class of hostile columns
its distance from the 80-bit truth (tests/response_truth.py) is at most formal_solution_truth.bound(the double-precision restatement's
own distance, N_d) — four times the restatement's distance plus 4e-15 per gap; tests/test_response_cpu.py checks what that rests on.
Every test prints its figures before it asserts."""
import contextlib
import types

import numpy as np
import pytest

import formal_solution_truth as T
import response_truth as R
from stardis_amd import ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 4), (3, 5, 4), (9, 7, 16), (56, 20, 8), (40, 64, 2)]
FLUX_PARITY = 5e-13  # the project's documented flux parity (README)
H = 1e-3


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


def columns_run(c):
    """the number of leading columns handed to the kernel: never a multiple of the frequencies per wave, so the last wave is partial"""
    gpw = 64 // c.n_theta
    return c.n_nu if c.n_nu % gpw else c.n_nu - 1


def judge(r, key, a, n, label):
    c = r.case
    keep = r.keep & (np.arange(c.n_nu) < n)
    finite = np.isfinite(r.restated[key]) & keep[None, :]
    d_gpu, d_ref = T.distance(a, r.truth[key], finite), T.distance(r.restated[key], r.truth[key], finite)
    missed = []
    for name in c.classes:
        cols = c.columns(name) & finite.any(axis=0)
        if not cols.any():  # the definition has no value anywhere in this class at this shape (the reference divides by zero)
            continue
        g, o = float(d_gpu[cols].max()), float(d_ref[cols].max())
        print(f"{label} {key} {c.n_depth}/{c.n_theta} {c.order} {name}: kernel {g:.2e} restatement {o:.2e} bound {T.bound(o, c.n_depth):.2e}")
        if not g <= T.bound(o, c.n_depth):
            missed.append((name, g, o))
    assert not missed, (label, key, c.n_depth, c.n_theta, c.order, missed)
    if "transparent" in c.classes:
        assert not a[:, c.columns("transparent") & (np.arange(c.n_nu) < n)].any()  # alpha = 0 everywhere: exactly no response


def launch(ctx, r, n, want_opacity=True, want_source=True):
    c = r.case
    src = None if r.source is None else np.ascontiguousarray(r.source[:, :n])
    out = ops.response(c.nus[:n], c.temps, c.ray, c.weights, np.ascontiguousarray(c.alphas[:, :n]), ctx=ctx, source=src,
                       want_opacity=want_opacity, want_source=want_source)
    return [None if a is None else np.pad(a, ((0, 0), (0, c.n_nu - n)), constant_values=np.nan) for a in out]


# ---- the kernel against the truth ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source_seed", [None, 5], ids=["planck", "source plane"])
@pytest.mark.parametrize("order", ["grouped", "interleaved"])
@pytest.mark.parametrize("n_depth,n_theta,per_class", SHAPES)
def test_kernel_against_truth(ctx, n_depth, n_theta, per_class, order, source_seed):
    r = R.responses(n_depth, n_theta, per_class, order, source_seed)
    n = columns_run(r.case)
    with profiled(ctx):
        Ra, Rs = launch(ctx, r, n)
        assert ctx.profile("k_response")[0] == 1
    judge(r, "Ra", Ra, n, "k_response")
    judge(r, "Rs", Rs, n, "k_response")
    only_a, none = launch(ctx, r, n, want_source=False)
    assert none is None and np.array_equal(only_a, Ra, equal_nan=True)
    none, only_s = launch(ctx, r, n, want_opacity=False)
    assert none is None and np.array_equal(only_s, Rs, equal_nan=True)


def test_host_buffer_twin(ctx):
    r = R.responses(9, 7, 16)
    c = r.case
    Ra, Rs = ops.response(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx)
    out_a, out_s = np.full(c.alphas.shape, np.nan), np.full(c.alphas.shape, np.nan)
    p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data  # noqa: E731
    nus, t, ray, w, al = (np.ascontiguousarray(a, dtype=np.float64) for a in (c.nus, c.temps, c.ray, c.weights, c.alphas))
    ctx.call("sdx_response_f64", c.n_depth, c.n_nu, c.n_theta, p(nus), p(t), p(ray), p(w), p(al), None, out_a.ctypes.data, out_s.ctypes.data)
    assert np.array_equal(out_a, Ra, equal_nan=True) and np.array_equal(out_s, Rs, equal_nan=True)
    only = np.full(c.alphas.shape, np.nan)
    ctx.call("sdx_response_f64", c.n_depth, c.n_nu, c.n_theta, p(nus), p(t), p(ray), p(w), p(al), None, None, only.ctypes.data)
    assert np.array_equal(only, Rs, equal_nan=True)


@pytest.mark.parametrize("n_depth,n_theta,per_class", SHAPES)
def test_source_identity_on_the_device(ctx, n_depth, n_theta, per_class):
    """sum_k R_source[k] S[k] against F_nu[-1] of sdx_raytrace_dev on the same columns: each side within the flux's own bound() of the
    truth's flux, so the two within twice that.  The sum itself in extended precision (no rounding of its own)."""
    r = R.responses(n_depth, n_theta, per_class)
    c = r.case
    ref = c.reference()
    _, Rs = ops.response(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx, want_opacity=False)
    F, _ = ops.raytrace_arrays(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx)
    flux_distance = T.per_class(c, ref["Fo"], ref["Ft"], ref["Fo"])  # {class: (oracle's distance, the same)}
    with np.errstate(all="ignore"):
        total = (Rs.astype(T.L) * r.restated["S"].astype(T.L)).sum(axis=0)
        scale = np.maximum(np.abs(np.where(np.isfinite(ref["Fo"]), ref["Ft"], 0)).max(axis=0), T.L(1e-300))
        d = (np.abs(total - F[-1].astype(T.L)) / scale).astype(np.float64)
    ok = np.isfinite(F[-1]) & np.isfinite(total.astype(np.float64)) & r.keep
    missed = []
    for name in c.classes:
        cols = c.columns(name) & ok
        if not cols.any():
            continue
        worst, allowed = float(d[cols].max()), 2 * T.bound(flux_distance[name][1], n_depth)
        print(f"sum R_source S against F_nu[-1] {n_depth}/{n_theta} {name}: {worst:.2e}, allowed {allowed:.2e} ({int(cols.sum())} columns)")
        if not worst <= allowed:
            missed.append((name, worst, allowed))
    assert not missed, missed
    assert ok[np.isin(c.cls, R.OPAQUE)].all()


# ---- the projection ----------------------------------------------------------------------------------------------------------------
def test_projection_bit_for_bit(ctx):
    rng = np.random.default_rng(3)
    nd, n, ld = 7, 333, 340
    Rp, part, total = (rng.standard_normal((nd, ld)) for _ in range(3))
    part, total = np.abs(part), np.abs(total) + 0.1
    total[2, 5], total[4, 9], part[4, 9] = 0.0, 0.0, 0.0  # x / 0 = inf, 0 / 0 = NaN
    d = [ctx.upload(a) for a in (Rp, part, total)]
    out = ctx.empty((n,))
    ctx.call("sdx_response_project_dev", nd, n, d[0].ptr, ld, d[1].ptr, ld, d[2].ptr, ld, out.ptr)
    expect = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(nd):
            expect = expect + Rp[k, :n] * (part[k, :n] / total[k, :n])
    got = out.numpy()
    assert np.isinf(got[5]) and np.isnan(got[9])
    assert np.array_equal(got, expect, equal_nan=True)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def fixed_window_lines(nus, lines, margin):
    """The reference gives every (line, depth) a window of int(max(10, (gamma + doppler_width) alpha / d_nu 20)) grid points either side
    of the line (opacities_solvers/base.py:561-575): the flux is a step function of a line's strength wherever that integer moves, and
    a difference quotient across a step measures the step.  -> the lines whose windows, clipped to the grid, are the same for every
    strength factor in [1 / margin, margin] at every depth: the floor of 10 points, or a window that covers the grid either way."""
    d_nu = -np.diff(nus).max()
    closest = nus.size - np.searchsorted(nus[::-1], lines["line_nus"])
    reach = (lines["gammas"] + lines["doppler_widths"]) * lines["alphas"] / d_nu * 20
    ok = np.ones(lines["line_nus"].size, dtype=bool)
    for factor in (1.0 / margin, margin):
        hw, hw1 = np.maximum(10, reach * factor).astype(np.int64), np.maximum(10, reach).astype(np.int64)
        lo, hi = np.maximum(closest[:, None] - hw, 0), np.minimum(closest[:, None] + hw, nus.size)
        lo1, hi1 = np.maximum(closest[:, None] - hw1, 0), np.minimum(closest[:, None] + hw1, nus.size)
        ok &= ((lo == lo1) & (hi == hi1)).all(axis=1)
    return np.flatnonzero(ok)


def small_model():
    """12 depth points of the solar structure, 300 frequencies around H alpha, 40 lines.  Species X: the six strongest of the lines
    whose windows do not move under the strength factors of the difference quotients (twice the step, for the margin)."""
    sun = synth.solar_atmosphere()
    pick = np.linspace(0, sun["temperatures"].size - 1, 12).astype(int)
    atm = {k: (v[pick] if isinstance(v, np.ndarray) and v.size == sun["temperatures"].size else v) for k, v in sun.items()}
    atm["dist"] = np.diff(atm["r"])
    nus = synth.tracing_grid(6560.0, 6570.0, n_override=300)
    lines = synth.synth_lines(nus, atm, 40, seed=17, mix=(0.5, 0.4, 0.1))
    fixed = fixed_window_lines(nus, lines, np.exp(2 * H))
    assert fixed.size >= 6
    x_lines = np.sort(fixed[np.argsort(lines["alphas"][fixed].max(axis=1))[-6:]])
    thetas, weights = synth.thetas_and_weights(8)
    return types.SimpleNamespace(atm=atm, nus=nus, lines=lines, x_lines=x_lines, thetas=thetas, weights=weights, cont=synth.synth_continuum_state(atm))


TAU_FLOOR = 0.2  # the smallest optical depth of a gap of the end-to-end column, at any frequency


def smallest_tau(m, total):
    return float((np.sqrt(total[1:] * total[:-1]).min(axis=1) * m.atm["dist"]).min())


def thicken(ctx, m):
    """A difference quotient of the double-precision flux is a fair judge only where that flux is smooth in the opacity: a gap with
    5e-4 <= tau << 1 forms w2 = 2 w1 - tau^2 e^-tau with a rounding error of 1e-16 / tau^3 of its value (formal_solution_truth.py),
    the flux inherits 1e-16 / tau^2 of the source difference per gap, and at h = 1e-3 that exceeds the floor of 5e-13 / h many times over
    (measured on the unchanged column, whose upper gaps have tau ~ 1e-3: the two difference quotients disagree by 1e-11 of the flux,
    at random from column to column).  The opacities do not depend on the geometry, so one step gives them, and the lengths of the
    gaps are then set so that every gap has tau >= TAU_FLOOR at every frequency: rounding below 2e-14 of the source difference."""
    syn = synthesizer(ctx, m)
    syn.step()
    ctx.synchronize()
    total = np.array(syn.total_alphas())
    syn.close()
    m.atm["dist"] = 1.05 * TAU_FLOOR / np.sqrt(total[1:] * total[:-1]).min(axis=1)  # (5 %: the strength factors move the opacities by 0.1 %)
    return m


def synthesizer(ctx, m, lines=None, **kw):
    return SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, m.lines if lines is None else lines, m.cont,
                               ctx=ctx, track_evaluations=False, **kw)


def scaled(m, factor):
    out = {k: v.copy() for k, v in m.lines.items()}
    out["alphas"][m.x_lines] *= factor
    return out


@pytest.fixture(scope="module")
def model(ctx):
    m = thicken(ctx, small_model())
    only_x = {k: np.ascontiguousarray(v[m.x_lines]) for k, v in m.lines.items()}
    syn = synthesizer(ctx, m, only_x, keep_line=True)
    syn.step()
    ctx.synchronize()
    m.alpha_x = np.array(syn.alpha_line())
    syn.close()
    flux = {}
    for h in (H, -H, H / 2, -H / 2):
        syn = synthesizer(ctx, m, scaled(m, np.exp(h)))
        syn.step()
        ctx.synchronize()
        flux[h] = np.array(syn.F_nu()[-1])
        syn.close()
    m.coarse, m.fine = (flux[H] - flux[-H]) / (2 * H), (flux[H / 2] - flux[-H / 2]) / H
    return m


def against_differences(m, derivative, F_last, label, columns=slice(None)):
    coarse, fine = m.coarse[columns], m.fine[columns]
    extrapolated = (4 * fine - coarse) / 3
    error = np.abs(derivative - extrapolated)
    allowed = np.abs(coarse - fine) + FLUX_PARITY * np.abs(F_last).max() / H
    print(f"{label}: max |analytic - extrapolated| {error.max():.3e}, smallest allowance {allowed.min():.3e}, max |dF/dln eps| {np.abs(derivative).max():.3e}, "
          f"worst ratio {(error / allowed).max():.3f}")
    assert np.all(error <= allowed)
    assert np.abs(derivative).max() > 100 * allowed.min()  # the lines of X are seen: the check is not passed by a zero


def test_end_to_end(ctx, model):
    m = model
    assert m.atm["temperatures"].size == 12 and m.nus.size == 300 and m.lines["line_nus"].size == 40 and m.alpha_x.any()
    syn = synthesizer(ctx, m, keep_response=True, keep_line=True)
    syn.step()
    ctx.synchronize()
    assert syn.keep_total and syn.response_opacity.shape == (12, 300) and syn.response_source.shape == (12, 300)
    eager = syn.flux_derivative(m.alpha_x)
    assert eager.shape == (300,)
    eager, F = np.array(eager.numpy()), np.array(syn.F_nu())
    assert smallest_tau(m, syn.total_alphas()) >= TAU_FLOOR
    Ra, Rs = np.array(syn.response_opacity.numpy()), np.array(syn.response_source.numpy())
    against_differences(m, eager, F[-1], "eager step")
    # a DeviceArray in place of the host array: the same bits
    assert np.array_equal(syn.flux_derivative(ctx.upload(m.alpha_x)).numpy(), eager)
    # recorded and replayed
    syn.response_opacity.zero()
    syn.response_source.zero()
    syn.capture()
    syn.response_opacity.zero()
    syn.response_source.zero()
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.response_opacity.numpy(), Ra) and np.array_equal(syn.response_source.numpy(), Rs) and np.array_equal(syn.F_nu(), F)
    against_differences(m, syn.flux_derivative(m.alpha_x).numpy(), F[-1], "capture() and step()")
    # the unfused path: the same launch behind the individual entry points
    syn.response_opacity.zero()
    syn.enqueue_unfused()
    ctx.synchronize()
    against_differences(m, syn.flux_derivative(m.alpha_x).numpy(), syn.F_nu()[-1], "enqueue_unfused")
    with pytest.raises(ValueError, match="keep_response"):
        syn.keep_total = False
    syn.close()
    # a frequency shard: columns 100 .. 219 of the whole-grid result, bit for bit
    part = synthesizer(ctx, m, keep_response=True, shard=(100, 120))
    part.step()
    ctx.synchronize()
    assert np.array_equal(part.response_opacity.numpy(), Ra[:, 100:220]) and np.array_equal(part.response_source.numpy(), Rs[:, 100:220])
    shard_derivative = part.flux_derivative(np.ascontiguousarray(m.alpha_x[:, 100:220])).numpy()
    assert np.array_equal(shard_derivative, eager[100:220])
    against_differences(m, shard_derivative, F[-1], "shard (100, 120)", slice(100, 220))
    part.close()


def test_off_is_off(ctx, model):
    m = model
    outputs = []
    for kw in (dict(), dict(keep_response=False)):
        syn = synthesizer(ctx, m, keep_contribution=True, **kw)
        with profiled(ctx):
            syn.step()
            ctx.synchronize()
            assert ctx.profile("k_response")[0] == 0
        outputs.append((np.array(syn.F_nu()), np.array(syn.total_alphas()), np.array(syn.contribution.numpy())))
        with pytest.raises(RuntimeError, match="keep_response=True"):
            syn.response_opacity
        syn.close()
    on = synthesizer(ctx, m, keep_contribution=True, keep_response=True)
    with profiled(ctx):
        on.step()
        ctx.synchronize()
        assert ctx.profile("k_response")[0] == 1 and ctx.profile("k_contribution")[0] == 1
    outputs.append((np.array(on.F_nu()), np.array(on.total_alphas()), np.array(on.contribution.numpy())))
    on.close()
    for other in outputs[1:]:
        for a, b in zip(outputs[0], other):
            assert np.array_equal(a, b)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    r = R.responses(9, 7, 16)
    c = r.case
    d = [ctx.upload(a) for a in (c.nus, c.temps, c.ray, c.weights, c.alphas)]
    out = ctx.empty(c.alphas.shape)
    n = c.n_nu

    def call(n_depth=c.n_depth, n_theta=c.n_theta, Ra=out.ptr, Rs=out.ptr, n_nu=n):
        ctx.call("sdx_response_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n, None, 0, Ra, n, Rs, n)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for n_nu in (n, 0):  # also at set-up time, with an empty grid
                with pytest.raises(ValueError, match="mixed_precision"):
                    call(n_nu=n_nu)
            with pytest.raises(ValueError, match="mixed_precision"):
                SpectralSynthesizer(c.nus, c.temps, c.dist, c.thetas, c.weights, dict(line_nus=np.zeros(0), doppler_widths=np.zeros((0, c.n_depth)),
                                    gammas=np.zeros((0, c.n_depth)), alphas=np.zeros((0, c.n_depth))), None, ctx=ctx, keep_response=True)
        finally:
            ctx.set_option("mixed_precision", 0)
        for n_nu in (n, 0):
            with pytest.raises(ValueError, match="64 angles"):
                call(n_theta=65, n_nu=n_nu)
            with pytest.raises(ValueError, match="deep"):
                call(n_depth=1000, n_nu=n_nu)  # (9 n_depth + 49 doubles at seven angles and one frequency per wave: above 64 KB)
        with pytest.raises(ValueError, match="no output"):
            call(Ra=None, Rs=None)
        ctx.synchronize()
        assert ctx.profile("k_response")[0] == 0
        call()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile("k_response")[0] == 1


# ---- the plain function and the solver-level twin ----------------------------------------------------------------------------------
def test_response_functions_and_ops_agree_with_the_engine(ctx, model):
    from stardis_amd._lib import default_context
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    m = model
    syn = synthesizer(ctx, m, keep_response=True)
    syn.step()
    ctx.synchronize()
    Ra, Rs, total = np.array(syn.response_opacity.numpy()), np.array(syn.response_source.numpy()), np.array(syn.total_alphas())
    syn.close()
    ray = m.atm["dist"].reshape(-1, 1) / np.cos(m.thetas)
    got = ops.response(m.nus, m.atm["temperatures"], ray, m.weights, total, ctx=ctx)
    assert np.array_equal(got[0], Ra) and np.array_equal(got[1], Rs)
    stellar_model = types.SimpleNamespace(spherical=False, temperatures=m.atm["temperatures"],
                                          geometry=types.SimpleNamespace(dist_to_next_depth_point=m.atm["dist"]))
    field = types.SimpleNamespace(thetas=m.thetas, I_nus_weights=m.weights, frequencies=m.nus, opacities=types.SimpleNamespace(total_alphas=total))
    assert default_context() is not None
    got = rfs.response_functions(stellar_model, field)
    assert np.array_equal(got[0], Ra) and np.array_equal(got[1], Rs)
    with pytest.raises(NotImplementedError):
        rfs.response_functions(types.SimpleNamespace(spherical=True), field)
