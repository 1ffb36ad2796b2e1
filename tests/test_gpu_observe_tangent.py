"""The instrument's tangent on the device (k_observe_tangent, k_rotate_tangent, k_observe_response_grad; Instrument.tangent and
parameter_tangents; SpectralSynthesizer.observed_tangent, observed_jacobian, chi2_instrument_gradient) against its restatement
(tests/observe_tangent_reference.py), against 50-digit mpmath, against difference quotients of the device's own forward and against
the existing reverse mode by the dot identity.  Every comparison also requires the compared quantity to exceed ten times its allowance
somewhere, so a zero cannot pass; figures are printed before they are asserted.  tests/test_observe_tangent_cpu.py asserts the window
lengths and mapping estimates of the (grid, R) pairs used here and fixes the steps of the difference quotients."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import observe_reference as oref
import observe_tangent_reference as tref
import observe_truth as OT
import rotation_reference as rref
from observe_tangent_reference import FLUX_TOL, LD, SUM_TOL
from rotation_reference import ROT_TOL
from stardis_amd import _lib, ops, synth
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from test_gpu_response import H, profiled, scaled, small_model, synthesizer, thicken
from test_observe_tangent_cpu import EPS_STEPS, LSF_STEPS, V_STEPS

pytestmark = pytest.mark.gpu

LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform
IRREGULAR = np.sort(np.random.default_rng(7).uniform(6500.0, 6600.0, 3000))
TWO_DENSITY = np.r_[np.linspace(6500.0, 6550.0, 500, endpoint=False), np.linspace(6550.0, 6600.0, 4000)]
GRIDS = {"S-c2": LAM, "irregular": IRREGULAR, "two-density": TWO_DENSITY}
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)
TINY = float(np.finfo(np.float64).tiny)


def vectors(lam, seed=11):
    """-> flux, reference, dflux (signed), dreference (signed)"""
    rng = np.random.default_rng(seed)
    return 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0), rng.standard_normal(lam.size), rng.standard_normal(lam.size)


def dev_observe(ctx, lam, flux, edges, sigma, v=0.0, reference=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d = [up(a) for a in (lam, flux, reference, edges, np.broadcast_to(sigma, (edges.size - 1,)), np.array([oref.doppler_factor(v)]))]
    out = ctx.empty((edges.size - 1,))
    ctx.call("sdx_observe_dev", lam.size, d[0].ptr, d[1].ptr, _lib.ptr_of(d[2]), edges.size - 1, d[3].ptr, d[4].ptr, d[5].ptr, out.ptr)
    return np.array(out.numpy())


def dev_tangent(ctx, lam, flux, edges, sigma, v=0.0, reference=None, dflux=None, dreference=None, want=("out", "v_rad", "lsf", "flux")):
    """sdx_observe_tangent_dev on uploaded arrays, the Doppler factor through device memory -> {name: host array} of what was asked for"""
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    n_pix = edges.size - 1
    d = [up(a) for a in (lam, flux, reference, edges, np.broadcast_to(sigma, (n_pix,)), np.array([oref.doppler_factor(v)]), dflux, dreference)]
    outs = {k: ctx.empty((n_pix,)) for k in want if k != "flux" or dflux is not None}
    ctx.call("sdx_observe_tangent_dev", lam.size, d[0].ptr, d[1].ptr, _lib.ptr_of(d[2]), n_pix, d[3].ptr, d[4].ptr, d[5].ptr, _lib.ptr_of(d[6]),
             _lib.ptr_of(d[7]), *(_lib.ptr_of(outs.get(k)) for k in ("out", "v_rad", "lsf", "flux")))
    ctx.synchronize()
    return {k: np.array(a.numpy()) for k, a in outs.items()}


def dev_rotate_tangent(ctx, lam, flux, V, eps, reference=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_f, d_g, d_rot = up(lam), up(flux), up(reference), up(np.array([V, eps]))
    new = lambda on: ctx.empty((lam.size,)) if on else None  # noqa: E731
    outs = [new(True), new(reference is not None), new(True), new(reference is not None)]
    ctx.call("sdx_rotate_tangent_dev", lam.size, d_lam.ptr, d_f.ptr, _lib.ptr_of(d_g), d_rot.ptr, *(_lib.ptr_of(a) for a in outs))
    ctx.synchronize()
    return tuple(None if a is None else np.array(a.numpy()) for a in outs)


def dev_rotate(ctx, lam, flux, V, eps, reference=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_f, d_g, d_rot = up(lam), up(flux), up(reference), up(np.array([V, eps]))
    out, out_ref = ctx.empty((lam.size,)), None if reference is None else ctx.empty((lam.size,))
    ctx.call("sdx_rotate_dev", lam.size, d_lam.ptr, d_f.ptr, _lib.ptr_of(d_g), d_rot.ptr, out.ptr, _lib.ptr_of(out_ref))
    ctx.synchronize()
    return np.array(out.numpy()), None if out_ref is None else np.array(out_ref.numpy())


def held(tag, got, ref, scale, tol, nonzero=True):
    """|device - restatement| <= tol scale at every covered pixel (NaN exactly where the restatement is NaN)"""
    ok = ~np.isnan(ref.astype(np.float64))
    assert np.array_equal(np.isnan(got), ~ok), tag
    err, allow = np.abs(got[ok].astype(LD) - ref[ok]).astype(np.float64), tol * scale[ok].astype(np.float64)
    print(f"{tag}: {int(ok.sum())} values, worst |device - restatement| / allowance {float(np.max(err / allow)):.3e}, largest |value| / allowance "
          f"{float(np.max(np.abs(ref[ok]).astype(np.float64) / allow)):.3e}")
    assert np.all(allow > 0) and np.all(err <= allow)
    assert not nonzero or np.any(np.abs(ref[ok]).astype(np.float64) > 10 * allow)


# ---- 1: the response's partials against mpmath -----------------------------------------------------------------------------------------
def response_gradient_distances(ctx):
    """-> (distance of obs_response, of dr/dx, of dr/d ln sigma) from 50 digits on response_grad_points(): r and dr/dx relative to
    themselves, dr/d ln sigma relative to its product-rule scale (tests/observe_tangent_reference.py); values below fp64's range excused"""
    mpmath.mp.dps = 50
    a, b = tref.response_grad_points()
    r, rx, rs = ops.observe_response_grad(a, b, 0.0, 1.0, ctx=ctx)
    worst = [0.0, 0.0, 0.0]
    for k in range(a.size):
        exact_r, G, S, scale = tref.mp_response(a[k], b[k])
        for i, (got, exact, sc) in enumerate(((r[k], exact_r, abs(exact_r)), (rx[k], G, abs(G)), (rs[k], S, scale))):
            if sc > TINY:
                worst[i] = max(worst[i], float(abs(mpmath.mpf(float(got)) - exact) / sc))
            elif exact == 0:
                assert got == 0, (a[k], b[k], i)
    return tuple(worst)


def response_within_its_bound(ctx):
    """obs_response itself, per point of response_grad_points(), against 50 digits:
        |r - exact| <= (U (E(p) + E(q)) / 2 + 4 |r|) 2^-53 + c_args,   c_args = 2^-53 (|a| e^(-a^2) + |b| e^(-b^2)) 2 / sqrt(pi),
    U the recorded error of the device's erf and erfc (tests/observe_truth.py), E(.) the two values the branch subtracts, c_args the
    rounding of a and b carried through the response.  -> the worst |r - exact| / bound"""
    U = OT.device_U()
    a, b = tref.response_grad_points()
    r = ops.observe_response_grad(a, b, 0.0, 1.0, ctx=ctx)[0]
    worst = 0.0
    with mpmath.workdps(50):
        eps = mpmath.mpf(2) ** -53
        for k in range(a.size):
            exact = tref.mp_response(a[k], b[k])[0]
            ma, mb = mpmath.mpf(float(a[k])) / mpmath.sqrt(2), mpmath.mpf(float(b[k])) / mpmath.sqrt(2)
            E = (mpmath.erfc(ma) + mpmath.erfc(mb)) / 2 if ma > 0 else ((mpmath.erfc(-mb) + mpmath.erfc(-ma)) / 2 if mb < 0 else (abs(mpmath.erf(mb)) + abs(mpmath.erf(ma))) / 2)
            c_args = eps * (abs(ma) * mpmath.exp(-ma * ma) + abs(mb) * mpmath.exp(-mb * mb)) * 2 / mpmath.sqrt(mpmath.pi)
            bound = (U * E + 4 * abs(mpmath.mpf(float(r[k])))) * eps + c_args
            err = abs(mpmath.mpf(float(r[k])) - exact)
            assert err <= bound, (float(a[k]), float(b[k]), float(r[k]), float(err), float(bound))
            worst = max(worst, float(err / bound))
    return worst


def test_response_gradient_against_mpmath(ctx):
    """the gradient is allowed four times the distance of obs_response itself on the same points: the same exp and erf family, one more
    product.  obs_response's distance is that of a difference of two erfc for the pixel 1e-4 sigma wide in a tail; the gradient, formed
    through expm1, keeps its relative accuracy there, and what it measures is printed beside what it is allowed.  obs_response in turn
    has its own bound per point (response_within_its_bound), so a worse response does not make the gradient's allowance wider."""
    d_r, d_rx, d_rs = response_gradient_distances(ctx)
    print(f"distance from 50 digits: obs_response {d_r:.3e}, dr/dx {d_rx:.3e}, dr/d ln sigma {d_rs:.3e}; allowed 4 x {d_r:.3e} = {4 * d_r:.3e}")
    print(f"obs_response against its own bound: worst |r - exact| / bound {response_within_its_bound(ctx):.3e}")
    assert 0 < d_rx <= 4 * d_r and 0 < d_rs <= 4 * d_r
    # the host-buffer twin and scalars
    a, b = tref.response_grad_points()
    dev = ops.observe_response_grad(a, b, 0.0, 1.0, ctx=ctx)
    twin = [np.empty(a.size) for _ in range(3)]
    zero, one = np.zeros(a.size), np.ones(a.size)
    p = lambda v: v.ctypes.data  # noqa: E731
    ctx.call("sdx_observe_response_grad_f64", a.size, p(a), p(b), p(zero), p(one), *(p(v) for v in twin))
    assert all(np.array_equal(x, y) for x, y in zip(dev, twin))
    single = ops.observe_response_grad(float(a[40]), float(b[40]), 0.0, 1.0, ctx=ctx)
    assert all(np.ndim(v) == 0 and v == w[40] for v, w in zip(single, dev))


# ---- 2: k_observe_tangent against the restatement ----------------------------------------------------------------------------------------
def check_tangent(ctx, tag, lam, edges, sigma, v=0.0, reference=True, nonzero=True, seed=11):
    f, g, df, dg = vectors(lam, seed)
    g, dg = (g, dg) if reference else (None, None)
    got = dev_tangent(ctx, lam, f, edges, sigma, v, reference=g, dflux=df, dreference=dg)
    assert np.array_equal(got["out"], dev_observe(ctx, lam, f, edges, sigma, v, reference=g), equal_nan=True), tag  # bit for bit k_observe's
    r = tref.observe_tangent(lam, f, edges, sigma, oref.doppler_factor(v), reference=g, dflux=df, dreference=dg)
    for name in ("v_rad", "lsf", "flux"):
        held(f"{tag}, v = {v}{', reference' if reference else ''}: {name}", got[name], r[name], r[name + "_terms"], FLUX_TOL, nonzero=nonzero)
    # each output alone: the same bits, whatever else is asked for
    for name in ("v_rad", "lsf", "flux"):
        alone = dev_tangent(ctx, lam, f, edges, sigma, v, reference=g, dflux=df if name == "flux" else None, dreference=dg if name == "flux" else None, want=(name,))
        assert list(alone) == [name] and np.array_equal(alone[name], got[name], equal_nan=True), (tag, name)
    return got


@pytest.mark.parametrize("R", [2.0e5, 1.2e5, 5.0e4])
def test_tangent_on_the_sc2_grid(ctx, R):
    """windows of 20 points (eight lanes per pixel everywhere), 31 .. 32 (the estimate straddles kObsShort inside the launch) and 72 (a
    wave per pixel), at three velocities, with and without a reference"""
    sigma = oref.sigma_of_R(SC2_EDGES, R)
    for v, reference in ((0.0, False), (37.5, True), (-120.0, False), (-120.0, True)):
        got = check_tangent(ctx, f"S-c2, R = {R:.1e}", LAM, SC2_EDGES, sigma, v, reference)
        nan = int(np.isnan(got["out"]).sum())
        assert nan < 100 and (nan > 0) == (v == -120.0)  # (the blue-shifted grid leaves the detector's red end uncovered)


def test_tangent_with_sigma_varying_along_the_detector(ctx):
    sigma = oref.sigma_of_R(SC2_EDGES, 1.6e5) * np.linspace(1.0, 4.0, 2048)  # eight lanes at the blue end, a wave per pixel at the red
    n = oref.window_lengths(LAM, SC2_EDGES, sigma)
    print(f"windows of {n[n > 0].min()} .. {n.max()} points")
    assert n[n > 0].min() < 32 < n.max()
    check_tangent(ctx, "sigma x 1 .. 4", LAM, SC2_EDGES, sigma, 37.5, True)
    check_tangent(ctx, "sigma x 1 .. 4", LAM, SC2_EDGES, sigma, 0.0, False)


def test_tangent_with_pixels_far_narrower_and_far_wider_than_sigma(ctx):
    """pixels 1e-3 sigma and 50 sigma wide side by side in one detector"""
    sigma = 0.02
    widths = np.tile([50 * sigma, 1e-3 * sigma], 40)
    edges = 6510.0 + np.r_[0.0, np.cumsum(widths)]
    assert edges[-1] < 6560.0 and np.isclose(np.diff(edges).min() / sigma, 1e-3) and np.isclose(np.diff(edges).max() / sigma, 50.0)
    check_tangent(ctx, "1e-3 and 50 sigma", LAM, edges, sigma, 37.5, True)
    check_tangent(ctx, "1e-3 and 50 sigma", LAM, edges, sigma, 0.0, False)


@pytest.mark.parametrize("grid", ["irregular", "two-density", "two-density, eight lanes"])
def test_tangent_on_other_grids(ctx, grid):
    """the mean-spacing estimate is wrong locally; either mapping must serve any window"""
    lam = GRIDS[grid.split(",")[0]]
    edges = np.linspace(6505.0, 6595.0, 301 if grid == "irregular" else 501)
    sigma = oref.sigma_of_R(edges, 2.0e4) if grid == "irregular" else np.full(500, 0.02 if "eight" in grid else 0.05)
    check_tangent(ctx, grid, lam, edges, sigma, -120.0, True)
    check_tangent(ctx, grid, lam, edges, sigma, 37.5, False)


def test_tangent_on_small_detectors_and_small_grids(ctx):
    for n_pix in (1, 7, 9):  # one pixel; a group that is not full; one pixel into the second group
        edges = np.linspace(6540.0, 6540.0 + 0.05 * n_pix, n_pix + 1)
        check_tangent(ctx, f"n_pix = {n_pix}", LAM, edges, oref.sigma_of_R(edges, 5.0e4), 37.5, True)
        check_tangent(ctx, f"n_pix = {n_pix}", LAM, edges, oref.sigma_of_R(edges, 2.0e5), 0.0, False)
    for n in (2, 3, 9):  # no window fits the grid: every pixel is uncovered and every output NaN
        lam = 6560.0 + 0.013 * np.arange(n) ** 1.1
        edges = np.linspace(lam[0], lam[-1], 4)
        f, g, df, dg = vectors(lam)
        got = dev_tangent(ctx, lam, f, edges, 0.05, 0.0, reference=g, dflux=df, dreference=dg)
        assert sorted(got) == ["flux", "lsf", "out", "v_rad"] and all(np.isnan(a).all() and a.size == 3 for a in got.values()), n


def test_a_detector_that_overhangs_both_ends_of_the_grid(ctx):
    edges = np.linspace(6495.0, 6605.0, 1101)
    sigma = oref.sigma_of_R(edges, 5.0e4)
    got = check_tangent(ctx, "overhanging", LAM, edges, sigma, 37.5, True)
    nan = np.isnan(got["out"])
    print(f"{int(nan.sum())} of 1100 pixels are NaN")
    assert 80 < nan.sum() < 150 and nan[0] and nan[-1] and all(np.array_equal(np.isnan(got[k]), nan) for k in ("v_rad", "lsf", "flux"))


def test_constants_are_preserved_and_have_no_parameter_tangent(ctx):
    """a constant flux without reference, and flux == reference with one, give exactly the forward's constant; their parameter tangents
    are pure cancellation: within SUM_TOL of the sum of the absolute terms"""
    sigma = oref.sigma_of_R(SC2_EDGES, 5.0e4)
    g = vectors(LAM)[1]
    for tag, f, ref, expect in (("constant", np.full(LAM.size, 1.7), None, 1.7), ("flux == reference", g, g, 1.0)):
        got = dev_tangent(ctx, LAM, f, SC2_EDGES, sigma, 37.5, reference=ref, want=("out", "v_rad", "lsf"))
        r = tref.observe_tangent(LAM, f, SC2_EDGES, sigma, oref.doppler_factor(37.5), reference=ref)
        ok = ~np.isnan(got["out"])
        assert np.array_equal(got["out"], dev_observe(ctx, LAM, f, SC2_EDGES, sigma, 37.5, reference=ref), equal_nan=True)
        assert ok.sum() > 1900 and (np.all(got["out"][ok] == 1.0) if ref is not None else np.max(np.abs(got["out"][ok] / expect - 1)) <= 1e-14)
        for name in ("v_rad", "lsf"):
            ratio = float(np.max(np.abs(got[name][ok]) / r[name + "_terms"][ok].astype(np.float64)))
            print(f"{tag}: worst |{name}| / absolute terms {ratio:.3e}")
            assert ratio <= SUM_TOL and np.all(r[name + "_terms"][ok] > 0)


# ---- 3: against the device's own difference quotients -------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5.0e4, 2.0e5])
def test_parameter_tangents_against_the_device_s_own_difference_quotients(ctx, R):
    """dout_velocity and dout_lsf against Richardson-extrapolated central differences of sdx_observe_dev at v +- h and sigma (1 +- h),
    the steps fixed by tests/test_observe_tangent_cpu.py; allowance |coarse - fine| + FLUX_TOL scale / h, over the pixels covered at all
    four evaluations.  A point that enters a window between two evaluations carries 1e-15 of the sum: fixed windows cost nothing here."""
    f, g, _, _ = vectors(LAM)
    sigma = oref.sigma_of_R(SC2_EDGES, R)
    v0 = 37.5
    for ref in (None, g):
        got = dev_tangent(ctx, LAM, f, SC2_EDGES, sigma, v0, reference=ref, want=("out", "v_rad", "lsf"))
        scale = float(np.abs(f).max() if ref is None else np.nanmax(np.abs(got["out"])))
        forward = {"v_rad": lambda h: dev_observe(ctx, LAM, f, SC2_EDGES, sigma, v0 + h, reference=ref),  # noqa: B023
                   "lsf": lambda h: dev_observe(ctx, LAM, f, SC2_EDGES, sigma * (1 + h), v0, reference=ref)}  # noqa: B023
        for name, steps in (("v_rad", V_STEPS), ("lsf", LSF_STEPS)):
            coarse, fine = ((forward[name](h).astype(LD) - forward[name](-h)) / (2 * h) for h in steps)
            ok = ~np.isnan((coarse + fine).astype(np.float64)) & ~np.isnan(got[name])
            rich = (4 * fine - coarse) / 3
            allow = (np.abs(coarse - fine) + FLUX_TOL * scale / steps[0]).astype(np.float64)[ok]
            err = np.abs(got[name][ok] - rich[ok]).astype(np.float64)
            print(f"R = {R:.0e}{', reference' if ref is not None else ''}, {name}: {int(ok.sum())} pixels, worst |tangent - Richardson| / allowance "
                  f"{np.max(err / allow):.3e}, largest |tangent| / allowance {np.max(np.abs(got[name][ok]) / allow):.3e}")
            assert ok.sum() > 1900 and np.all(err <= allow) and np.any(np.abs(got[name][ok]) > 10 * allow)


@pytest.mark.parametrize("V", [10.0, 100.0])
def test_dout_eps_against_the_device_s_own_difference_quotients(ctx, V):
    """out is a ratio of two functions linear in eps, so a single quotient does not suffice (at h = 0.1 it is off by 1.6e-05 of the flux,
    tests/test_observe_tangent_cpu.py): the Richardson value of sdx_rotate_dev at eps +- 0.02 and +- 0.01, with the rounding term of the
    rotation stage's own tolerance"""
    lam = LAM[:2500]
    f, g, _, _ = vectors(lam)
    _, _, d, d_ref = dev_rotate_tangent(ctx, lam, f, V, 0.5, reference=g)
    for tag, flux, got in (("flux", f, d), ("reference", g, d_ref)):
        coarse, fine = ((dev_rotate(ctx, lam, flux, V, 0.5 + h)[0].astype(LD) - dev_rotate(ctx, lam, flux, V, 0.5 - h)[0]) / (2 * h) for h in EPS_STEPS)
        allow = (np.abs(coarse - fine) + ROT_TOL * np.abs(flux).max() / EPS_STEPS[0]).astype(np.float64)
        err = np.abs(got - (4 * fine - coarse) / 3).astype(np.float64)
        print(f"V = {V}, {tag}: worst |dout_eps - Richardson| / allowance {np.max(err / allow):.3e}, largest |dout_eps| / allowance {np.max(np.abs(got) / allow):.3e}")
        assert np.all(err <= allow) and np.any(np.abs(got) > 10 * allow)


# ---- 4: k_rotate_tangent -----------------------------------------------------------------------------------------------------------------
def check_rotate_tangent(ctx, tag, lam, V, eps=0.6):
    f, g, _, _ = vectors(lam)
    out, out_ref, d, d_ref = dev_rotate_tangent(ctx, lam, f, V, eps, reference=g)
    plain = dev_rotate(ctx, lam, f, V, eps, reference=g)
    assert np.array_equal(out, plain[0]) and np.array_equal(out_ref, plain[1]), tag  # bit for bit k_rotate's
    alone = dev_rotate_tangent(ctx, lam, f, V, eps)
    assert np.array_equal(alone[0], out) and np.array_equal(alone[2], d) and alone[1] is None and alone[3] is None
    r, r_ref, scale, scale_ref = tref.rotate_tangent(lam, f, V, eps, reference=g)
    single = int(rref.window_lengths(lam, V).max()) == 1  # every window the point alone: an exact 0
    for name, got, ref, sc in (("dout_eps", d, r, scale), ("dout_eps_reference", d_ref, r_ref, scale_ref)):
        assert np.all(np.isfinite(got))
        held(f"{tag}, V = {V}, eps = {eps}: {name}", got, ref, sc, ROT_TOL, nonzero=not single)
    if single:  # dw (F - out) / w with out = (w F) / w: two roundings of F, not an exact 0 (the point's own dw is not 0)
        assert np.max(np.abs(d)) <= 1e-15 * np.abs(f).max() and np.max(np.abs(d_ref)) <= 1e-15 * np.abs(g).max()


@pytest.mark.parametrize("V", [0.2, 2.0, 9.6, 19.3, 211.0])
def test_rotate_tangent_on_the_sc2_grid(ctx, V):
    """windows of 1, 7, 33 (the estimate straddles the switch within the grid), 65 and 704 points"""
    assert rref.window_lengths(LAM, V).max() == {0.2: 1, 2.0: 7, 9.6: 33, 19.3: 65, 211.0: 704}[V]
    check_rotate_tangent(ctx, "S-c2", LAM, V)
    if V == 19.3:
        for eps in (0.0, 1.0):
            check_rotate_tangent(ctx, "S-c2", LAM, V, eps)


@pytest.mark.parametrize("grid,V", [("irregular", 23.7), ("irregular", 100.0), ("two-density", 23.7), ("two-density", 100.0)])
def test_rotate_tangent_on_other_grids(ctx, grid, V):
    check_rotate_tangent(ctx, grid, GRIDS[grid], V)


def test_rotate_tangent_on_small_grids_and_without_rotation(ctx):
    cases = [(f"n = {n}, every window truncated", 6560.0 + 0.013 * np.arange(n) ** 1.1, 40.0) for n in (2, 3, 9)]
    cases += [(f"n = {n}", 6560.0 * np.exp(np.arange(n) / 4.1e5), V) for n, V in ((13, 3.0), (77, 9.0), (1001, 30.0))]
    for tag, lam, V in cases:
        assert rref.clear_of_profile_edge(lam, V, 1e-8), tag
        check_rotate_tangent(ctx, tag, lam, V)
    f, g, _, _ = vectors(LAM)
    for V in (0.0, -1.0, np.nan):  # a copy, and zeros
        out, out_ref, d, d_ref = dev_rotate_tangent(ctx, LAM, f, V, 0.6, reference=g)
        assert np.array_equal(out, f) and np.array_equal(out_ref, g) and not d.any() and not d_ref.any(), V
    twin = ops.rotate_tangent(LAM, f, 19.3, 0.6, reference=g, ctx=ctx)
    assert len(twin) == 4 and all(np.array_equal(a, b) for a, b in zip(twin, dev_rotate_tangent(ctx, LAM, f, 19.3, 0.6, reference=g)))
    pair = ops.rotate_tangent(LAM, f, 19.3, 0.6, ctx=ctx)
    assert len(pair) == 2 and np.array_equal(pair[0], twin[0]) and np.array_equal(pair[1], twin[2])


# ---- 5: forward and reverse agree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v_rot,v_mac", [(None, None), (19.3, None), (None, 3.2), (19.3, 3.2)], ids=["no broadening", "rotation", "macroturbulence", "both"])
def test_the_tangent_and_the_adjoint_satisfy_the_dot_identity(ctx, v_rot, v_mac):
    """sum_j c_j tangent(dF, dg)_j = sum_i (w_flux_i dF_i + w_reference_i dg_i) with (w_flux, w_reference) from Instrument.adjoint: one
    identity that tests forward and reverse mode at once, through every stage, to SUM_TOL per stage of the sum of the absolute terms —
    the same identity with |c|, |dF| and |dg|, where every weight of the chain keeps one sign (flux, reference > 0) — over the covered
    pixels that are not edge-affected"""
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_rot=v_rot, v_mac=v_mac)
    inst.set_radial_velocity(37.5)
    f, g, df, dg = vectors(LAM)
    c = np.random.default_rng(5).standard_normal(2048)
    d_lam, d_f, d_g, d_df, d_dg = (ctx.upload(a) for a in (LAM, f, g, df, dg))
    stages = 1 + (v_rot is not None) + (v_mac is not None)
    for ref_on in (False, True):
        t = np.array(inst.tangent(d_lam, LAM.size, d_f, d_df, reference=d_g if ref_on else None, dreference=d_dg if ref_on else None).numpy())
        use = ~np.isnan(t) & ~inst.edge_affected(LAM)
        cu = np.where(use, c, 0.0)
        assert 1900 < use.sum() <= 2048
        w = inst.adjoint(d_lam, LAM.size, ctx.upload(cu), flux=d_f if ref_on else None, reference=d_g if ref_on else None, out_reference=ref_on)
        w_abs = inst.adjoint(d_lam, LAM.size, ctx.upload(np.abs(cu)), flux=d_f if ref_on else None, reference=d_g if ref_on else None, out_reference=ref_on)
        w, w_abs = [[np.array(a.numpy()) for a in (x if ref_on else (x,))] for x in (w, w_abs)]
        lhs = float(np.sum(np.where(use, cu * t, 0.0).astype(LD)))
        rhs = float(np.sum(w[0].astype(LD) * df) + (np.sum(w[1].astype(LD) * dg) if ref_on else 0))
        terms = float(np.sum(np.abs(w_abs[0]) * np.abs(df)) + (np.sum(np.abs(w_abs[1]) * np.abs(dg)) if ref_on else 0))
        print(f"{'normalised' if ref_on else 'plain'}: <c, tangent> = {lhs:.15e}, <adjoint(c), (dF, dg)> = {rhs:.15e}, difference / allowance "
              f"{abs(lhs - rhs) / (stages * SUM_TOL * terms):.3e}, |value| / allowance {abs(lhs) / (stages * SUM_TOL * terms):.3e}")
        assert abs(lhs - rhs) <= stages * SUM_TOL * terms and abs(lhs) > 10 * stages * SUM_TOL * terms
        # the host twins: the same bits as the device path
        host = inst.tangent_host(LAM, f, df, reference=g if ref_on else None, dreference=dg if ref_on else None)
        assert np.array_equal(host, t, equal_nan=True)
        if ref_on:  # a reference that does not move: the second term is absent
            still = np.array(inst.tangent(d_lam, LAM.size, d_f, d_df, reference=d_g).numpy())
            assert not np.array_equal(still, t, equal_nan=True) and np.array_equal(still, inst.tangent_host(LAM, f, df, reference=g), equal_nan=True)


def test_instrument_parameter_tangents_against_the_instrument_s_own_difference_quotients(ctx):
    """Instrument.parameter_tangents through rotation and macroturbulence: every column against Richardson quotients of observe() under
    the instrument's own setters (a rebuilt Instrument for sigma), the allowance of check 3, over the pixels that are covered at
    every evaluation and not edge-affected; then the host twin, bit for bit"""
    lam = LAM[(LAM > 6520.0) & (LAM < 6580.0)]
    edges = np.linspace(6522.0, 6578.0, 601)
    f, g, _, _ = vectors(lam)
    V, eps, zeta, v0, R = 19.3, 0.5, 3.2, 37.5, 5.0e4
    make = lambda k=1.0: Instrument(edges, sigma=oref.sigma_of_R(edges, R) * k, ctx=ctx, v_rot=V, limb_darkening=eps, v_mac=zeta)  # noqa: E731
    inst = make()
    inst.set_radial_velocity(v0)
    d_lam, d_f, d_g = (ctx.upload(a) for a in (lam, f, g))
    observe = lambda i, ref: np.array(i.observe(d_lam, d_f, lam.size, reference=d_g if ref else None, out=ctx.empty((600,))).numpy())  # noqa: E731
    for ref_on in (False, True):
        cols = {k: np.array(v.numpy()) for k, v in inst.parameter_tangents(d_lam, lam.size, d_f, reference=d_g if ref_on else None).items()}
        assert list(cols) == ["v_rad", "lsf", "v_mac", "limb_darkening"]
        base = observe(inst, ref_on)
        scale = float(np.abs(f).max() if not ref_on else np.nanmax(np.abs(base)))
        host = inst.parameter_tangents_host(lam, f, reference=g if ref_on else None)
        for name, steps, tol in (("v_rad", V_STEPS, FLUX_TOL), ("lsf", LSF_STEPS, FLUX_TOL), ("v_mac", (0.008 * zeta, 0.004 * zeta), FLUX_TOL), ("limb_darkening", EPS_STEPS, FLUX_TOL)):
            def at(h, name=name):
                if name == "lsf":
                    other = make(1 + h)
                    other.set_radial_velocity(v0)
                    return observe(other, ref_on)
                {"v_rad": lambda: inst.set_radial_velocity(v0 + h), "v_mac": lambda: inst.set_macroturbulence(zeta + h),
                 "limb_darkening": lambda: inst.set_rotation(V, eps + h)}[name]()
                out = observe(inst, ref_on)
                inst.set_radial_velocity(v0), inst.set_macroturbulence(zeta), inst.set_rotation(V, eps)
                return out
            coarse, fine = ((at(h).astype(LD) - at(-h)) / (2 * h) for h in steps)
            ok = ~np.isnan((coarse + fine).astype(np.float64)) & ~np.isnan(cols[name]) & ~inst.edge_affected(lam)
            allow = (np.abs(coarse - fine) + tol * scale / steps[0]).astype(np.float64)[ok]
            err = np.abs(cols[name][ok] - ((4 * fine - coarse) / 3)[ok]).astype(np.float64)
            print(f"{'normalised' if ref_on else 'plain'}, {name}: {int(ok.sum())} pixels, worst |column - Richardson| / allowance {np.max(err / allow):.3e}, "
                  f"largest |column| / allowance {np.max(np.abs(cols[name][ok]) / allow):.3e}")
            assert ok.sum() > 500 and np.all(err <= allow) and np.any(np.abs(cols[name][ok]) > 10 * allow)
            assert np.array_equal(host[name], cols[name], equal_nan=True), name
        assert np.array_equal(observe(inst, ref_on), base, equal_nan=True)  # the setters were put back
    one = inst.parameter_tangents(d_lam, lam.size, d_f, wrt="lsf")
    assert list(one) == ["lsf"]


# ---- 6: through the synthesizer ----------------------------------------------------------------------------------------------------------
V_ROT, V_MAC, V_RAD, EPS = 10.0, 3.0, 12.0, 0.6
ENGINE_EDGES = np.r_[6560.75, 6561.2, np.linspace(6562.0, 6568.0, 25), 6571.0]


def engine_instrument(ctx, k=1.0):
    """the detector of tests/test_gpu_macroturbulence.py: two pixels within the broadening's reach of the grid's blue end, 24 clear of
    both ends, one off the red end"""
    inst = Instrument(ENGINE_EDGES, sigma=0.05 * k, ctx=ctx, v_rot=V_ROT, limb_darkening=EPS, v_mac=V_MAC)
    inst.set_radial_velocity(V_RAD)
    return inst


@pytest.fixture(scope="module")
def model(ctx):
    """the small model of tests/test_gpu_response.py (12 depths, 300 points, 40 lines) with the line opacity of its species X"""
    m = thicken(ctx, small_model())
    only_x = {k: np.ascontiguousarray(v[m.x_lines]) for k, v in m.lines.items()}
    syn = synthesizer(ctx, m, only_x, keep_line=True)
    syn.step()
    ctx.synchronize()
    m.alpha_x = np.array(syn.alpha_line())
    syn.close()
    return m


def richardson(tag, got, coarse, fine, scale, h, use):
    allow = (np.abs(coarse - fine) + FLUX_TOL * scale / h).astype(np.float64)[use]
    err = np.abs(got[use] - ((4 * fine - coarse) / 3)[use]).astype(np.float64)
    print(f"{tag}: {int(use.sum())} pixels, worst |column - Richardson| / allowance {np.max(err / allow):.3e}, largest |column| / allowance "
          f"{np.max(np.abs(got[use]) / allow):.3e}")
    assert np.all(err <= allow) and np.any(np.abs(got[use]) > 10 * allow)


def test_engine_jacobian_tangent_and_chi2(ctx, model):
    m = model
    lam = K.nu_to_angstrom(m.nus)
    inst = engine_instrument(ctx)
    syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=inst)
    names = ("v_rad", "lsf", "v_mac", "limb_darkening")
    stages = ("k_observe_tangent", "k_rotate_tangent", "k_observe_response_grad")
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert [ctx.profile(k)[0] for k in stages] == [0, 0, 0] and not hasattr(inst, "_tangent_scratch")  # a step asks for no tangent
        jac = {norm: {k: np.array(v.numpy()) for k, v in syn.observed_jacobian(names, normalized=norm).items()} for norm in (False, True)}
        ctx.synchronize()
        print(f"launches of two observed_jacobian calls: {[ctx.profile(k)[0] for k in stages]}")
        assert ctx.profile("k_observe_tangent")[0] == 6 and ctx.profile("k_rotate_tangent")[0] == 2
    edge = inst.edge_affected(lam)
    observed = {False: np.array(syn.observed.numpy()), True: np.array(syn.observed_normalized.numpy())}
    use = ~np.isnan(observed[False]) & ~edge
    assert use.tolist() == [False, False] + [True] * 24 + [False]

    def runs(knob, steps):
        out = {}
        for h in [s * sign for s in steps for sign in (1, -1)]:
            knob(h)
            syn.step()
            out[h] = (np.array(syn.observed.numpy()), np.array(syn.observed_normalized.numpy()))
        knob(0.0)
        syn.step()
        assert np.array_equal(syn.observed.numpy(), observed[False], equal_nan=True)
        return out

    def rebuilt(h):  # sigma is fixed at construction: a rebuilt Instrument observes the step's own F_lambda
        other = engine_instrument(ctx, 1 + h)
        n = syn.n_nu
        return (np.array(other.observe(syn.d_lambdas, syn.d_Flam, n, out=ctx.empty((27,))).numpy()),
                np.array(other.observe(syn.d_lambdas, syn.d_Flam, n, reference=syn.d_Fclam, out=ctx.empty((27,))).numpy()))

    knobs = {"v_rad": (lambda h: inst.set_radial_velocity(V_RAD + h), V_STEPS), "v_mac": (lambda h: inst.set_macroturbulence(V_MAC + h), (0.008 * V_MAC, 0.004 * V_MAC)),
             "limb_darkening": (lambda h: inst.set_rotation(V_ROT, EPS + h), EPS_STEPS)}
    for name in names:
        steps = LSF_STEPS if name == "lsf" else knobs[name][1]
        r = {h: rebuilt(h) for h in [s * sign for s in steps for sign in (1, -1)]} if name == "lsf" else runs(knobs[name][0], steps)
        for norm in (False, True):
            coarse, fine = ((r[h][norm].astype(LD) - r[-h][norm]) / (2 * h) for h in steps)
            richardson(f"observed_jacobian, {name}{', normalised' if norm else ''}", jac[norm][name], coarse, fine, float(np.nanmax(np.abs(observed[norm]))), steps[0], use)

    # a grid-space tangent: dF / d ln(abundance of X) pushed to the pixels against two syntheses with the strength factor moved
    tangent = {False: np.array(syn.observed_tangent(syn.flux_derivative(m.alpha_x)).numpy()),
               True: np.array(syn.observed_tangent(syn.flux_derivative(m.alpha_x), normalized=True).numpy())}
    assert np.array_equal(syn.observed_tangent(np.array(syn.flux_derivative(m.alpha_x).numpy())).numpy(), tangent[False], equal_nan=True)
    moved = {}
    for h in (H, -H, H / 2, -H / 2):
        other = synthesizer(ctx, m, scaled(m, np.exp(h)), keep_continuum_flux=True, instrument=inst)
        other.step()
        moved[h] = (np.array(other.observed.numpy()), np.array(other.observed_normalized.numpy()))
        other.close()
    for norm in (False, True):
        coarse, fine = ((moved[h][norm].astype(LD) - moved[-h][norm]) / (2 * h) for h in (H, H / 2))
        richardson(f"observed_tangent(flux_derivative){', normalised' if norm else ''}", tangent[norm], coarse, fine, float(np.nanmax(np.abs(observed[norm]))), H, use)
    with pytest.raises(ValueError, match="normalized"):
        syn.observed_tangent(syn.flux_derivative(m.alpha_x), dF_nu_continuum=np.zeros(300))
    with pytest.raises(ValueError, match="dF_nu"):
        syn.observed_tangent(np.zeros(299))

    # chi-square: gradient and Gauss-Newton matrix from the columns, the sums on the host
    rng = np.random.default_rng(8)
    for norm in (False, True):
        obs = observed[norm]
        data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(27))
        ivar = rng.uniform(0.5, 2.0, 27) / np.nanmax(np.abs(obs)) ** 2
        ivar[5] = 0.0
        used = ~np.isnan(obs) & (ivar != 0) & ~edge
        chi2, grad, Hm = syn.chi2_instrument_gradient(data, ivar, names, normalized=norm, curvature=True)
        resid, w = np.where(used, data, 0.0) - np.where(used, obs, 0.0), np.where(used, ivar, 0.0)
        assert used.sum() == 23 and chi2 == float(np.sum(w * resid * resid)) and list(grad) == list(names) and Hm.shape == (4, 4)
        J = np.stack([np.where(used, jac[norm][k], 0.0) for k in names], axis=1)
        expect_g, terms_g = J.T @ (-2.0 * w * resid), np.abs(J).T @ np.abs(2.0 * w * resid)
        expect_H, terms_H = 2.0 * (J * w[:, None]).T @ J, 2.0 * (np.abs(J) * w[:, None]).T @ np.abs(J)
        got_g = np.array([grad[k] for k in names])
        print(f"normalized = {norm}: chi2 {chi2!r}, worst |gradient - numpy| / terms {np.max(np.abs(got_g - expect_g) / terms_g):.3e}, worst |H - numpy| / terms "
              f"{np.max(np.abs(Hm - expect_H) / terms_H):.3e}")
        assert np.all(np.abs(got_g - expect_g) <= SUM_TOL * terms_g) and np.all(np.abs(got_g) > 10 * SUM_TOL * terms_g)
        assert np.array_equal(Hm, Hm.T) and np.all(np.abs(Hm - expect_H) <= SUM_TOL * terms_H) and np.all(np.diag(Hm) > 0)
        assert syn.chi2_instrument_gradient(data, ivar, "lsf", normalized=norm) == (chi2, {"lsf": grad["lsf"]})
        # the tangent route against the adjoint route: J's absolute terms are below 2 max |observed| / zeta per pixel (the profile and its
        # derivative term have the same area), two reordered sums per stage
        _, adjoint_route = syn.chi2_macroturbulence_gradient(data, ivar, normalized=norm)
        allowance = 3 * SUM_TOL * float(np.sum(np.abs(2.0 * w * resid))) * 2 * float(np.nanmax(np.abs(obs))) / V_MAC
        print(f"normalized = {norm}: d chi2 / d zeta by tangents {grad['v_mac']:+.12e}, by the adjoint {adjoint_route:+.12e}, difference / allowance "
              f"{abs(grad['v_mac'] - adjoint_route) / allowance:.3e}, |value| / allowance {abs(adjoint_route) / allowance:.3e}")
        assert abs(grad["v_mac"] - adjoint_route) <= allowance and abs(adjoint_route) > 10 * allowance
    with pytest.raises(ValueError, match="v_rad, lsf, v_mac, limb_darkening"):
        syn.observed_jacobian(("v_rad", "v_rot"))
    syn.close()


# ---- 7: behaviour --------------------------------------------------------------------------------------------------------------------------
def capture(ctx, run):
    ctx.call("sdx_graph_begin")
    try:
        run()
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    return graph


@pytest.mark.parametrize("v_rot,v_mac", [(None, None), (19.3, 3.2)], ids=["no broadening", "both"])
def test_bits_repeat_and_a_captured_tangent_follows_the_velocity(ctx, v_rot, v_mac):
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_rot=v_rot, v_mac=v_mac)
    assert not hasattr(inst, "_tangent_scratch")
    f, g, df, dg = vectors(LAM)
    d_lam, d_f, d_g, d_df, d_dg = (ctx.upload(a) for a in (LAM, f, g, df, dg))
    out = ctx.empty((2048,))
    run = lambda: inst.tangent(d_lam, LAM.size, d_f, d_df, reference=d_g, dreference=d_dg, out=out)  # noqa: E731
    result = lambda: np.array(out.numpy())  # noqa: E731
    run()
    eager0 = result()
    run()
    assert np.array_equal(eager0, result(), equal_nan=True) and np.nan_to_num(eager0).any()
    assert hasattr(inst, "_tangent_scratch") == inst.broadens and len(getattr(inst, "_tangent_scratch", ())) == (6 if inst.broadens else 0)
    inst.set_radial_velocity(30.0)
    run()
    eager1 = result()
    assert not np.array_equal(eager1, eager0, equal_nan=True)
    inst.set_radial_velocity(0.0)
    graph = capture(ctx, run)  # (the scratch was sized by the eager runs: the capture allocates nothing)
    try:
        out.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        inst.set_radial_velocity(30.0)  # no new capture: the kernel reads the factor from device memory
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    print(f"replay against eager: {int(np.sum(replay0 != eager0))} values differ, after set_radial_velocity {int(np.sum(replay1 != eager1))} (NaN pixels count)")
    assert np.array_equal(replay0, eager0, equal_nan=True) and np.array_equal(replay1, eager1, equal_nan=True)
    assert np.array_equal(inst.tangent_host(LAM, f, df, reference=g, dreference=dg), eager1, equal_nan=True)
    if not inst.broadens:  # the pixel stage alone: ops and the host-buffer twin give the device's bits
        dev = dev_tangent(ctx, LAM, f, SC2_EDGES, inst.sigma, 30.0, reference=g, dflux=df, dreference=dg)
        host = ops.observe_tangent(LAM, f, SC2_EDGES, inst.sigma, v_rad=30.0, reference=g, dflux=df, dreference=dg, ctx=ctx)
        assert sorted(host) == sorted(dev) and all(np.array_equal(host[k], dev[k], equal_nan=True) for k in dev) and np.array_equal(dev["flux"], eager1, equal_nan=True)
        assert np.array_equal(host["out"], ops.observe(LAM, f, SC2_EDGES, inst.sigma, v_rad=30.0, reference=g, ctx=ctx), equal_nan=True)
        with pytest.raises(RuntimeError, match="no macroturbulence"):
            inst.parameter_tangents(d_lam, LAM.size, d_f, wrt="v_mac")
        with pytest.raises(RuntimeError, match="no rotation"):
            inst.parameter_tangents(d_lam, LAM.size, d_f, wrt=("lsf", "limb_darkening"))
        assert list(inst.parameter_tangents(d_lam, LAM.size, d_f)) == ["v_rad", "lsf"] and not hasattr(inst, "_tangent_scratch")
    with pytest.raises(ValueError, match="unknown parameter"):
        inst.parameter_tangents(d_lam, LAM.size, d_f, wrt="v_sin_i")
    with pytest.raises(ValueError, match="dreference"):
        inst.tangent(d_lam, LAM.size, d_f, d_df, dreference=d_dg)


def test_refusals_leave_the_context_serving(ctx):
    lib = ctx.lib
    lam = LAM[:500]
    edges = np.linspace(lam[100], lam[400], 33)
    f, g, df, _ = vectors(lam)
    n, n_pix = lam.size, 32
    sigma = np.full(n_pix, 0.02)
    expect = dev_tangent(ctx, lam, f, edges, sigma, 0.0, dflux=df)
    d, e, s = ctx.upload(lam), ctx.upload(edges), ctx.upload(sigma)
    o, o2 = ctx.empty((n_pix,)), ctx.empty((n_pix,))
    r, r2 = ctx.empty((n,)), ctx.empty((n,))
    with profiled(ctx):
        # (ctx, n, lambdas, flux, reference, n_pix, edges, sigma, doppler_dev, dflux, dreference, out, dout_velocity, dout_lsf, dout_flux)
        for args in ((1, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, o.ptr, None, None, None),  # n < 2
                     (n, None, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, o.ptr, None, None, None),
                     (n, d.ptr, None, None, n_pix, e.ptr, s.ptr, None, None, None, o.ptr, None, None, None),
                     (n, d.ptr, d.ptr, None, n_pix, None, s.ptr, None, None, None, o.ptr, None, None, None),
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, None, None, None, None, o.ptr, None, None, None),
                     (n, d.ptr, d.ptr, None, -1, e.ptr, s.ptr, None, None, None, o.ptr, None, None, None),
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, d.ptr, d.ptr, None, None, None, o.ptr),  # dreference without reference
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, d.ptr, None, o.ptr, None, None, None),  # dflux without dout_flux
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, None, None, None, o.ptr),  # dout_flux without dflux
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, s.ptr, None, None, None),  # out is an input
                     (n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, o.ptr, o.ptr, None, None)):  # two outputs in one buffer
            assert lib.sdx_observe_tangent_dev(ctx.handle, *args) == -1 and b"observe_tangent" in lib.sdx_last_error_string(), args
        # (ctx, n, lambdas, flux, reference, rot_dev, out, out_reference, dout_eps, dout_eps_reference)
        for args in ((1, d.ptr, d.ptr, None, d.ptr, r.ptr, None, r2.ptr, None), (n, None, d.ptr, None, d.ptr, r.ptr, None, r2.ptr, None),
                     (n, d.ptr, d.ptr, None, None, r.ptr, None, r2.ptr, None), (n, d.ptr, d.ptr, None, d.ptr, None, None, r2.ptr, None),
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, None, None),  # no dout_eps
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, r.ptr, None, r2.ptr, None),  # reference without out_reference
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, r2.ptr, o.ptr),  # dout_eps_reference without reference
                     (n, d.ptr, d.ptr, None, d.ptr, d.ptr, None, r2.ptr, None), (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, r.ptr, None)):
            assert lib.sdx_rotate_tangent_dev(ctx.handle, *args) == -1 and b"rotate_tangent" in lib.sdx_last_error_string(), args
        # the twin checks what the kernel cannot, before any copy
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = np.full(n_pix, -7.0)
        for tag, kw in dict(lambdas=dict(lam=np.ascontiguousarray(lam[::-1])), edges=dict(edges=np.ascontiguousarray(edges[::-1])), sigma=dict(sigma=-sigma),
                            doppler=dict(doppler=0.0)).items():
            a = dict(dict(lam=lam, edges=edges, sigma=sigma, doppler=1.0), **kw)
            rc = lib.sdx_observe_tangent_f64(ctx.handle, n, p(a["lam"]), p(f), None, n_pix, p(a["edges"]), p(a["sigma"]), a["doppler"], None, None, p(out), None, None, None)
            msg = lib.sdx_last_error_string().decode()
            print(f"{tag}: rc {rc}, '{msg}'")
            assert rc == -1 and np.all(out == -7.0) and tag in msg
        ctx.synchronize()
        assert ctx.profile("k_observe_tangent")[0] == 0 and ctx.profile("k_rotate_tangent")[0] == 0
        # n_pix = 0 and no output asked for: nothing to do, nothing launched
        assert lib.sdx_observe_tangent_dev(ctx.handle, n, d.ptr, d.ptr, None, 0, e.ptr, s.ptr, None, None, None, o.ptr, None, None, None) == 0
        assert lib.sdx_observe_tangent_dev(ctx.handle, n, d.ptr, d.ptr, None, n_pix, e.ptr, s.ptr, None, None, None, None, None, None, None) == 0
        ctx.synchronize()
        assert ctx.profile("k_observe_tangent")[0] == 0
        again = dev_tangent(ctx, lam, f, edges, sigma, 0.0, dflux=df)
        assert all(np.array_equal(again[k], expect[k], equal_nan=True) for k in expect) and ctx.profile("k_observe_tangent")[0] == 1
