"""The adjoint of the instrument model on the device (sdx_observe_adjoint_dev: per-pixel factors, two scans, the gather per grid point)
against its numpy restatement (tests/observe_adjoint_reference.py): per point to FLUX_TOL of the sum of the absolute values of the point's
terms (the pixel vector is signed, the sums cancel), with exact zeros where the restatement has no term; device-only, <observe(f), c>
against <f, adjoint(c)> to SUM_TOL of the sum of |c_j w_ij f_i / den_j|.  Every comparison also requires the compared quantity to exceed
ten times its allowance somewhere, so a zero cannot pass.  Then determinism, graph replay and the device-resident velocity, the
host-buffer twin, the refusals, and the chain through SpectralSynthesizer down to every line of the list.  Figures are printed before
they are asserted."""
import ctypes as C

import numpy as np
import pytest

import line_adjoint_truth as A
import observe_adjoint_reference as aref
import observe_reference as oref
from observe_reference import FLUX_TOL, SUM_TOL
from stardis_amd import _lib, ops, synth
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from test_gpu_response import FLUX_PARITY, H, model, profiled, synthesizer  # noqa: F401  (`model`: the module-scoped fixture)

pytestmark = pytest.mark.gpu

# the S-c2 grid as wavelengths (ascending), 7634 points about 0.013 A apart
LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))
DX = float(np.median(np.diff(LAM)))
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)
SC2_SIGMA = oref.sigma_of_R(SC2_EDGES, 5.0e4)
STAGE = "k_observe_adjoint"


def vectors(lam, n_pix, seed=11):
    """-> c (signed), flux, reference"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n_pix), 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0)


def device(ctx, inst, lam, c, flux=None, reference=None, nus=None):
    """the device entry point on uploaded arrays -> (w_flux, w_reference or None) as host arrays"""
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    res = inst.adjoint(up(lam), lam.size, up(c), flux=up(flux), reference=up(reference), nus=up(nus), out_reference=reference is not None)
    ctx.synchronize()
    return (np.array(res[0].numpy()), np.array(res[1].numpy())) if reference is not None else (np.array(res.numpy()), None)


def held(tag, got, ref, scale):
    err, allow = np.abs(got - ref), FLUX_TOL * scale
    print(f"{tag}: {ref.size} points, {int((scale > 0).sum())} with terms, worst |device - restatement| / allowance "
          f"{float(np.max(err[scale > 0] / allow[scale > 0])) if (scale > 0).any() else 0.0:.3e}, largest |value| / allowance "
          f"{float(np.max(np.abs(ref[scale > 0]) / allow[scale > 0])) if (scale > 0).any() else 0.0:.3e}")
    assert np.all(np.isfinite(got))
    assert np.all(got[scale == 0] == 0.0)  # a point in no covered window: exactly 0
    assert np.all(err <= allow)
    assert np.any(np.abs(ref) > 10 * allow)


def check(ctx, tag, lam, edges, sigma, v=0.0, with_reference=(False, True), with_nus=(False, True), seed=11):
    """device against restatement per point, and the device's own dot identity, in the modes asked for"""
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(edges) - 1,))
    D = oref.doppler_factor(v)
    assert oref.clear_of_grid_ends(lam, edges, sigma, D)
    inst = Instrument(edges, sigma=sigma, ctx=ctx)
    inst.set_radial_velocity(v)
    c, f, g = vectors(lam, sigma.size, seed)
    nus_all = K.C_CGS * 1.0e8 / lam
    for ref_on in with_reference:
        ref = g if ref_on else None
        out = inst.observe_host(lam, f, ref)
        ok = ~np.isnan(out)
        terms = aref.dot_terms(lam, c, f, edges, sigma, D, reference=ref)
        for nus_on in with_nus:
            nus = nus_all if nus_on else None
            mode = f"{tag}{', reference' if ref_on else ''}{', nus' if nus_on else ''}"
            w_flux, w_ref = device(ctx, inst, lam, c, flux=f if ref_on else None, reference=ref, nus=nus)
            r_flux, r_ref, scale, scale_ref = aref.adjoint(lam, c, edges, sigma, D, flux=f, reference=ref, nus=nus)
            held(mode + ": w_flux", w_flux, r_flux, scale)
            if ref_on:
                held(mode + ": w_reference", w_ref, r_ref, scale_ref)
            lhs, rhs = float(np.sum(c[ok] * out[ok])), float(w_flux @ (f * lam / nus if nus_on else f))
            print(f"{mode}: <observe(f), c> = {lhs:.15e}, <f, adjoint(c)> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * terms):.3e}")
            assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms


def expected_pixels(edges, sigma):
    """the estimate that chooses the gather's mapping (include/stardis_hip.h): 1 + 16 sigma / the mean pixel width, against 32"""
    return 1.0 + 16.0 * np.asarray(sigma) / ((edges[-1] - edges[0]) / (len(edges) - 1))


# ---- 1: the grid and the instrument users pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [-300.0, 0.0, 300.0])
def test_sc2_grid_2048_pixels(ctx, v):
    check(ctx, f"S-c2 grid, R = 50000, v = {v:+.0f} km/s", LAM, SC2_EDGES, SC2_SIGMA, v)


# ---- 2: windows that do not ascend -------------------------------------------------------------------------------------------------
def test_nonmonotone_sigma(ctx):
    lam, edges, sigma, v = aref.nonmonotone_input()
    lo, hi = edges[:-1] - 8 * sigma, edges[1:] + 8 * sigma
    gaps = aref.noncontiguous_points(aref.pixel_sets(lam, edges, sigma, oref.doppler_factor(v)))
    print(f"points whose pixel set is not a run of consecutive pixels: {gaps}")
    assert np.any(np.diff(lo) < 0) and np.any(np.diff(hi) < 0) and gaps >= 1
    check(ctx, "non-monotone sigma", lam, edges, sigma, v)


# ---- 3: other grids ------------------------------------------------------------------------------------------------------------------
def test_irregular_grid(ctx):
    rng = np.random.default_rng(99)
    lam = 6500.0 + np.cumsum(rng.uniform(0.003, 0.03, 3000))
    edges = np.linspace(lam[0] + 2.0, lam[-1] - 2.0, 151)
    check(ctx, "irregular grid, R = 40000", lam, edges, oref.sigma_of_R(edges, 4.0e4), with_nus=(False,))
    check(ctx, "irregular grid, sigma = 0.006 A", lam, edges[:60] * 1.0, 0.006, with_nus=(True,))


def test_two_density_grid(ctx):
    lam = np.r_[np.arange(6500.0, 6540.0, 0.05), np.arange(6540.0, 6560.0, 0.004), np.arange(6560.0, 6600.001, 0.05)]
    for tag, edges, sigma in (("dense stretch", 6545.0 + 0.01 * np.arange(41), 0.012), ("coarse stretch", np.linspace(6510.0, 6530.0, 41), 0.02),
                              ("across the joint", np.linspace(6536.0, 6544.0, 33), 0.05)):
        check(ctx, "two-density grid, " + tag, lam, edges, sigma, with_nus=(False,))


# ---- 4, 5, 8: pixels per point where the lane mapping can go wrong -----------------------------------------------------------------
def test_undersampled_line_spread_function(ctx):
    edges = np.linspace(6540.0, 6550.0, 201)
    n = oref.window_lengths(LAM, edges, 0.004)
    print(f"points per window {n.min()} .. {n.max()}")
    assert 1 <= n.min() and n.max() <= 12
    check(ctx, "sigma = 0.004 A, 0.05 A pixels", LAM, edges, 0.004)
    sparse = LAM[::5]  # one to five points per window
    n = oref.window_lengths(sparse, edges, 0.004)
    print(f"every fifth point: points per window {n.min()} .. {n.max()}")
    assert n.min() >= 1 and n.max() <= 5
    check(ctx, "sigma = 0.004 A, 0.05 A pixels, every fifth point", sparse, edges, 0.004)


def test_pixels_narrower_than_a_grid_step(ctx):
    edges = np.linspace(6540.0, 6542.0, 401)  # 0.005 A pixels on a 0.013 A grid
    assert np.diff(edges).max() < np.diff(LAM).min()
    per_point = aref.pixel_sets(LAM, edges, np.full(400, 0.025)).sum(axis=0).max()
    print(f"estimate {expected_pixels(edges, 0.025):.1f} pixels per point, in fact up to {per_point}")
    assert expected_pixels(edges, 0.025) > 32 and per_point > 64  # a wave per point, more than one trip
    check(ctx, "0.005 A pixels, sigma = 0.025 A", LAM, edges, 0.025)
    assert expected_pixels(edges, 0.004) <= 32
    check(ctx, "0.005 A pixels, sigma = 0.004 A", LAM, edges, 0.004, with_nus=(False,))


@pytest.mark.parametrize("side", ["below", "above", "both"])
def test_pixel_count_straddles_the_mapping_switch(ctx, side):
    """the gather takes eight lanes per point up to an estimate of 32 pixels per point and a wave per point above it"""
    edges = 6545.0 + 0.02 * np.arange(121)
    at_switch = 0.02 * 31.0 / 16.0
    sigma = {"below": np.full(120, 0.99 * at_switch), "above": np.full(120, 1.01 * at_switch),
             "both": np.where(np.arange(120) // 20 % 2 == 0, 0.97 * at_switch, 1.03 * at_switch)}[side]
    e = expected_pixels(edges, sigma)
    print(f"{side}: estimate {e.min():.2f} .. {e.max():.2f} pixels per point")
    assert {"below": e.max() <= 32, "above": e.min() > 32, "both": e.min() <= 32 < e.max()}[side] and np.all(np.abs(e - 32) < 1.5)
    check(ctx, f"pixels per point {side} the switch", LAM, edges, sigma, with_nus=(False,))


# ---- 6, 7: sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix", [1, 7, 8, 9, 64, 65])
def test_pixel_counts(ctx, n_pix):
    lam = LAM[(LAM > 6535.0) & (LAM < 6565.0)]
    edges = np.linspace(6540.0, 6560.0, n_pix + 1)
    check(ctx, f"n_pix = {n_pix}", lam, edges, oref.sigma_of_R(edges, 5.0e4), with_nus=(False,))
    check(ctx, f"n_pix = {n_pix}, short windows", lam, 6540.0 + 0.05 * np.arange(n_pix + 1), 0.004, with_reference=(True,), with_nus=(True,))


def test_two_and_three_point_grids(ctx):
    """n = 2: a covered window holds neither point, any other is not covered — no point has a term, the result is exactly 0"""
    for tag, lam, edges, sigma in (("covered, empty window", [6500.0, 6600.0], [6549.0, 6551.0], 0.5), ("reaches below the grid", [6500.0, 6600.0], [6549.0, 6551.0], 10.0),
                                   ("holds both points", [6549.97, 6550.03], [6549.95, 6550.05], 0.005)):
        lam, edges = np.array(lam), np.array(edges)
        inst = Instrument(edges, sigma=sigma, ctx=ctx)
        for flux, ref in ((None, None), (np.array([1.0, 3.0]), np.array([2.0, 2.5]))):
            w_flux, w_ref = device(ctx, inst, lam, np.array([1.5]), flux=flux, reference=ref)
            print(f"n = 2, {tag}{', reference' if ref is not None else ''}: {w_flux} {w_ref}")
            assert np.array_equal(w_flux, np.zeros(2)) and (w_ref is None or np.array_equal(w_ref, np.zeros(2)))
    # n = 3: the first pixel's window holds the middle point and nothing else, the second's holds none
    check(ctx, "n = 3", np.array([6549.0, 6550.0, 6551.0]), np.array([6549.9, 6550.1, 6550.3]), 0.01, with_nus=(False,))


# ---- 9: coverage ---------------------------------------------------------------------------------------------------------------------
def test_partly_covered_pixels(ctx):
    edges = np.linspace(6499.0, 6601.0, 301)
    sigma = oref.sigma_of_R(edges, 5.0e4)
    check(ctx, "300 pixels over 6499 - 6601", LAM, edges, sigma, with_nus=(False,))
    member = aref.pixel_sets(LAM, edges, sigma)
    uncovered, outside = ~member.any(axis=1), ~member.any(axis=0)
    assert uncovered.sum() == 10 and outside.sum() > 0
    inst = Instrument(edges, sigma=sigma, ctx=ctx)
    c, f, g = vectors(LAM, 300)
    for flux, ref in ((None, None), (f, g)):
        zeroed = device(ctx, inst, LAM, np.where(uncovered, 0.0, c), flux=flux, reference=ref)
        poisoned = device(ctx, inst, LAM, np.where(uncovered, np.nan, c), flux=flux, reference=ref)
        for a, b in zip(zeroed, poisoned):
            if a is not None:
                assert np.all(np.isfinite(b)) and np.array_equal(a, b) and np.all(b[outside] == 0.0) and np.any(b != 0.0)
    # an instrument that looks past the grid altogether: zeros
    away = Instrument(np.linspace(6650.0, 6700.0, 7), resolving_power=5.0e4, ctx=ctx)
    assert np.array_equal(device(ctx, away, LAM, np.full(6, np.nan))[0], np.zeros(LAM.size))


# ---- 10: determinism and graphs ------------------------------------------------------------------------------------------------------
def test_bits_repeat_and_graphs_follow_the_velocity(ctx):
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx)
    c, f, g = vectors(LAM, 2048)
    d_lam, d_c, d_f, d_g, d_nus = (ctx.upload(a) for a in (LAM, c, f, g, K.C_CGS * 1.0e8 / LAM))
    out, out_ref = ctx.empty((LAM.size,)), ctx.empty((LAM.size,))

    def run():
        inst.adjoint(d_lam, LAM.size, d_c, flux=d_f, reference=d_g, nus=d_nus, out=out, out_reference=out_ref)

    def result():
        return np.array(out.numpy()), np.array(out_ref.numpy())

    run()
    eager0 = result()
    run()
    again = result()
    print(f"two eager runs differ in {int(np.sum(eager0[0] != again[0]) + np.sum(eager0[1] != again[1]))} values")
    assert all(np.array_equal(a, b) for a, b in zip(eager0, again)) and eager0[0].any() and eager0[1].any()
    inst.set_radial_velocity(30.0)
    run()
    eager30 = result()
    assert not np.array_equal(eager30[0], eager0[0])
    inst.set_radial_velocity(0.0)
    ctx.call("sdx_graph_begin")
    try:
        run()
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    try:
        out.zero(), out_ref.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        inst.set_radial_velocity(30.0)  # no new capture: the kernels read the factor from device memory
        ctx.call("sdx_graph_launch", graph)
        replay30 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    print(f"replay against eager: v = 0 differs in {int(np.sum(replay0[0] != eager0[0]))} values, v = 30 in {int(np.sum(replay30[0] != eager30[0]))}")
    assert all(np.array_equal(a, b) for a, b in zip(replay0, eager0)) and all(np.array_equal(a, b) for a, b in zip(replay30, eager30))


# ---- 11, 12: the host-buffer twin and the refusals -----------------------------------------------------------------------------------
def test_host_twin_bits_validation_and_refusals(ctx):
    lib = ctx.lib
    edges = np.linspace(6540.0, 6560.0, 66)
    sigma = oref.sigma_of_R(edges, 5.0e4)
    inst = Instrument(edges, sigma=sigma, ctx=ctx)
    inst.set_radial_velocity(30.0)
    c, f, g = vectors(LAM, 65)
    nus = K.C_CGS * 1.0e8 / LAM
    for kw in (dict(), dict(nus=nus), dict(flux=f, reference=g), dict(flux=f, reference=g, nus=nus)):
        expect = device(ctx, inst, LAM, c, **kw)
        got = inst.adjoint_host(LAM, c, **kw)
        got = got if isinstance(got, tuple) else (got, None)
        print(f"host twin against the device entry ({', '.join(kw) or 'plain'}): {int(np.sum(got[0] != expect[0]))} values differ")
        assert np.array_equal(got[0], expect[0]) and expect[0].any() and (expect[1] is None or (np.array_equal(got[1], expect[1]) and expect[1].any()))
        via_ops = ops.observe_adjoint(LAM, c, edges, sigma, v_rad=30.0, ctx=ctx, **kw)
        assert np.array_equal(via_ops[0] if isinstance(via_ops, tuple) else via_ops, expect[0])
    plain = device(ctx, inst, LAM, c)[0]

    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def twin(lam=LAM, edges=edges, sigma=sigma, doppler=inst.doppler, n=None, out=True, flux=None, reference=None, w_ref=False):
        res, res_ref = np.full(lam.size, -7.0), np.full(lam.size, -7.0)
        rc = lib.sdx_observe_adjoint_f64(ctx.handle, lam.size if n is None else n, p(lam), p(flux), p(reference), sigma.size, p(edges), p(sigma), doppler,
                                         p(c), None, p(res) if out else None, p(res_ref) if w_ref else None)
        return rc, res

    repeated, with_nan, zero_sigma = edges.copy(), edges.copy(), sigma.copy()
    repeated[10], with_nan[20], zero_sigma[3] = repeated[9], np.nan, 0.0
    bad = dict(
        lambdas=dict(lam=np.ascontiguousarray(LAM[::-1])), edges=dict(edges=repeated), sigma=dict(sigma=zero_sigma), doppler=dict(doppler=0.0),
        nan_edge=dict(edges=with_nan), n_1=dict(n=1), null_out=dict(out=False), inf_doppler=dict(doppler=np.inf), nan_lambda=dict(lam=np.r_[LAM[:-1], np.nan]),
        w_ref_alone=dict(w_ref=True), ref_without_flux=dict(reference=g),
    )
    d = ctx.upload(LAM)
    n = LAM.size
    # (ctx, n, lambdas, flux, reference, n_pix, edges, sigma, doppler_dev, pixel_weight, nus, w_flux, w_reference)
    refused = ((1, d.ptr, None, None, 4, d.ptr, d.ptr, None, d.ptr, None, d.ptr, None), (n, None, None, None, 4, d.ptr, d.ptr, None, d.ptr, None, d.ptr, None),
               (n, d.ptr, None, None, 4, d.ptr, d.ptr, None, d.ptr, None, None, None), (n, d.ptr, None, None, 4, None, d.ptr, None, d.ptr, None, d.ptr, None),
               (n, d.ptr, None, None, 4, d.ptr, None, None, d.ptr, None, d.ptr, None), (n, d.ptr, None, None, 4, d.ptr, d.ptr, None, None, None, d.ptr, None),
               (n, d.ptr, None, None, -1, d.ptr, d.ptr, None, d.ptr, None, d.ptr, None), (n, d.ptr, None, None, 4, d.ptr, d.ptr, None, d.ptr, None, d.ptr, d.ptr),
               (n, d.ptr, None, d.ptr, 4, d.ptr, d.ptr, None, d.ptr, None, d.ptr, None))
    with profiled(ctx):
        for tag, kw in bad.items():
            rc, res = twin(**kw)
            msg = lib.sdx_last_error_string().decode()
            print(f"{tag}: rc {rc}, '{msg}'")
            assert rc == -1 and lib.sdx_last_error_code() == -1 and "observe" in msg and np.all(res == -7.0)
            named = {"nan_edge": "edges", "n_1": "n >= 2", "null_out": "w_flux", "inf_doppler": "doppler", "nan_lambda": "lambdas", "w_ref_alone": "w_reference",
                     "ref_without_flux": "flux"}.get(tag, tag)
            assert named in msg
        for args in refused:
            assert lib.sdx_observe_adjoint_dev(ctx.handle, *args) == -1
        ctx.synchronize()
        launches = ctx.profile(STAGE)[0]
        print(f"{STAGE} stages recorded during the refusals: {launches}")
        assert launches == 0
        # n_pix = 0: zeros, and no kernel
        zeros = ctx.upload(np.full(n, 3.0))
        assert lib.sdx_observe_adjoint_dev(ctx.handle, n, d.ptr, None, None, 0, None, None, None, None, None, zeros.ptr, None) == 0
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 0 and np.array_equal(zeros.numpy(), np.zeros(n))
        # the context still serves
        assert np.array_equal(device(ctx, inst, LAM, c)[0], plain)
        assert ctx.profile(STAGE)[0] == 1
    rc, after = twin()
    assert rc == 0 and np.array_equal(after, plain)


# ---- 13: the engine ------------------------------------------------------------------------------------------------------------------
def engine_instrument(ctx, v=12.0):
    """24 pixels inside the 6560 - 6570 A grid of the small model, one off its red end"""
    inst = Instrument(np.r_[np.linspace(6562.0, 6568.0, 25), 6571.0], sigma=0.05, ctx=ctx)
    inst.set_radial_velocity(v)
    return inst


def test_engine_chain(ctx, model):
    m = model
    n_depth, n_nu, n_lines = 12, 300, 40
    lam = K.nu_to_angstrom(m.nus)
    inst = engine_instrument(ctx)
    c = np.random.default_rng(5).standard_normal(25)
    c[-1] = np.nan  # the pixel off the grid's end: never read
    syn = synthesizer(ctx, m, keep_response=True, instrument=inst)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 0 and ctx.profile("k_line_adjoint")[0] == 0 and ctx.profile("k_observe")[0] == 1  # on demand
        sens = syn.observed_line_sensitivities(c)
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 1 and ctx.profile("k_line_adjoint")[0] == 1
    observed = np.array(syn.observed.numpy())
    assert np.isnan(observed[-1]) and not np.isnan(observed[:-1]).any()
    assert sens.shape == (n_lines,)
    sens = np.array(sens.numpy())
    grid_w = syn.pixel_weights_to_grid(c)
    assert grid_w.shape == (n_nu,) and np.all(np.isfinite(grid_w.numpy()))
    assert np.array_equal(syn.line_sensitivities(grid_w).numpy(), sens)
    assert np.array_equal(syn.observed_line_sensitivities(ctx.upload(c)).numpy(), sens)
    per_depth = syn.observed_line_sensitivities(c, per_depth=True)
    assert per_depth.shape == (n_lines, n_depth) and np.array_equal(per_depth.numpy(), syn.line_sensitivities(grid_w, per_depth=True).numpy())
    with pytest.raises(ValueError, match="c must hold"):
        syn.observed_line_sensitivities(np.ones(24))

    # per line against the forward chain: c . observe(flux_derivative(single-line plane) nu / lambda).  The bound of
    # test_gpu_line_adjoint.test_engine_identity, (2 OPACITY_RTOL + n_depth n_nu EPS) of the sum of the absolute terms, with the weights |c|
    # pulled through the instrument in place of |w|, and SUM_TOL of the same for the instrument's reordered sums
    c0 = np.where(np.isnan(c), 0.0, c)
    w_abs = np.array(syn.pixel_weights_to_grid(np.abs(c0)).numpy())
    assert np.all(w_abs >= 0) and w_abs.any()
    Ra, total = np.array(syn.response_opacity.numpy()), np.array(syn.total_alphas())
    d_lam = ctx.upload(lam)
    worst, seen = 0.0, False
    for l in range(n_lines):
        one = [np.ascontiguousarray(m.lines[k][l:l + 1]) for k in ("line_nus", "doppler_widths", "gammas", "alphas")]
        plane = ops.calc_alan_entries(n_depth, m.nus, *one, ctx=ctx)
        dF_lam = np.array(syn.flux_derivative(plane).numpy()) * m.nus / lam
        pushed = np.array(inst.observe(d_lam, ctx.upload(dF_lam), n_nu, out=ctx.empty((25,))).numpy())
        expect = float(np.sum(c0[:-1] * pushed[:-1]))
        allowed = (2 * A.OPACITY_RTOL + n_depth * n_nu * A.EPS + SUM_TOL) * float(np.abs(w_abs[None, :] * Ra * (plane / total)).sum())
        assert abs(sens[l] - expect) <= allowed, (l, sens[l], expect, allowed)  # (a line outside every pixel's window: 0 against 0)
        worst = max(worst, abs(sens[l] - expect) / allowed) if allowed > 0 else worst
        seen |= abs(sens[l]) > 10 * allowed
    print(f"observed_line_sensitivities against the forward chain per line: worst difference / bound {worst:.3e}")
    assert seen

    # against difference quotients of whole syntheses: species X (m.x_lines scaled together); the plain mode is linear, so the quotients
    # go through the device's observe
    F_last = np.array(syn.F_nu()[-1])
    push = lambda a: np.array(inst.observe(d_lam, ctx.upload(np.ascontiguousarray(a * m.nus / lam)), n_nu, out=ctx.empty((25,))).numpy())[:-1]  # noqa: E731
    extrapolated = float(np.sum(c0[:-1] * (4 * push(m.fine) - push(m.coarse)) / 3))
    allowance = float(np.sum(np.abs(c0[:-1]) * push(np.abs(m.coarse - m.fine) + FLUX_PARITY * np.abs(F_last).max() / H)))
    value = float(sens[m.x_lines].sum())
    print(f"species X: sum of its lines' sensitivities {value:+.6e}, Richardson value of the difference quotients {extrapolated:+.6e}, allowance {allowance:.3e}")
    assert abs(value - extrapolated) <= allowance and abs(value) > 10 * allowance
    syn.close()


def test_engine_chi2_and_normalized(ctx, model):
    m = model
    inst = engine_instrument(ctx, v=-8.0)
    syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=inst)
    syn.step()
    ctx.synchronize()
    rng = np.random.default_rng(8)
    for normalized in (False, True):
        obs = np.array((syn.observed_normalized if normalized else syn.observed).numpy())
        assert np.isnan(obs[-1]) and not np.isnan(obs[:-1]).any()
        data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(25))
        ivar = rng.uniform(0.5, 2.0, 25) / np.nanmax(np.abs(obs)) ** 2
        ivar[3] = 0.0
        data[3] = np.nan  # a pixel without weight: whatever its datum, it is left out
        use = ~np.isnan(obs) & (ivar != 0)
        assert use.sum() == 23
        chi2, grad = syn.chi2_line_gradient(data, ivar, normalized=normalized)
        r = np.where(use, data, 0.0) - np.where(use, obs, 0.0)
        w = np.where(use, ivar, 0.0)
        expect = float(np.sum(w * r * r))
        print(f"normalized = {normalized}: chi2 {chi2!r} against numpy {expect!r}")
        assert chi2 == expect and chi2 > 0
        assert np.array_equal(grad.numpy(), syn.observed_line_sensitivities(-2.0 * w * r, normalized=normalized).numpy()) and np.array(grad.numpy()).any()
        assert syn.chi2_line_gradient(data, ivar, normalized=normalized, per_depth=True)[1].shape == (40, 12)
    with pytest.raises(ValueError, match="no pixel left"):
        syn.chi2_line_gradient(np.ones(25), np.zeros(25))
    with pytest.raises(ValueError, match="inverse_variance"):
        syn.chi2_line_gradient(np.ones(25), np.ones(24))

    # the normalised weights: their dot identity on the device, and the continuum cotangent against the restatement
    lam = K.nu_to_angstrom(m.nus)
    c = rng.standard_normal(25)
    w, w_cont = syn.pixel_weights_to_grid(c, normalized=True, with_continuum=True)
    F, Fc = np.array(syn.F_nu()[-1]), np.array(syn.F_nu_continuum[-1])
    f_lam, g_lam = F * m.nus / lam, Fc * m.nus / lam
    r_flux, r_ref, scale, scale_ref = aref.adjoint(lam, c, inst.edges, inst.sigma, inst.doppler, flux=f_lam, reference=g_lam, nus=m.nus)
    held("engine, normalised weights", np.array(w.numpy()), r_flux, scale)
    held("engine, continuum weights", np.array(w_cont.numpy()), r_ref, scale_ref)
    norm = np.array(syn.observed_normalized.numpy())
    lhs, rhs = float(np.sum(c[:-1] * norm[:-1])), float(np.array(w.numpy()) @ F)
    terms = aref.dot_terms(lam, c, f_lam, inst.edges, inst.sigma, inst.doppler, reference=g_lam)
    print(f"normalised: <observed_normalized, c> = {lhs:.15e}, <F_nu, weights> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * terms):.3e}")
    assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms
    plain, plain_cont = syn.pixel_weights_to_grid(c, with_continuum=True)  # the plain spectrum does not depend on the continuum
    assert np.array_equal(plain.numpy(), syn.pixel_weights_to_grid(c).numpy()) and np.array_equal(plain_cont.numpy(), np.zeros(300))
    syn.close()


def test_engine_missing_options_raise_before_any_launch(ctx, model):
    m = model
    inst = engine_instrument(ctx)
    c = np.ones(25)
    bare, no_response, no_continuum = synthesizer(ctx, m, keep_response=True), synthesizer(ctx, m, instrument=inst), synthesizer(ctx, m, keep_response=True, instrument=inst)
    for syn in (bare, no_response, no_continuum):
        syn.step()
    ctx.synchronize()
    with profiled(ctx):
        for syn, call, match in ((bare, lambda s: s.pixel_weights_to_grid(c), "no instrument"), (bare, lambda s: s.observed_line_sensitivities(c), "no instrument"),
                                 (bare, lambda s: s.chi2_line_gradient(c, c), "no instrument"), (no_response, lambda s: s.observed_line_sensitivities(c), "keep_response=True"),
                                 (no_response, lambda s: s.chi2_line_gradient(c, c), "keep_response=True"),
                                 (no_continuum, lambda s: s.pixel_weights_to_grid(c, normalized=True), "keep_continuum_flux=True"),
                                 (no_continuum, lambda s: s.observed_line_sensitivities(c, normalized=True), "keep_continuum_flux=True"),
                                 (no_continuum, lambda s: s.chi2_line_gradient(c, c, normalized=True), "keep_continuum_flux=True")):
            with pytest.raises(RuntimeError, match=match):
                call(syn)
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 0 and ctx.profile("k_line_adjoint")[0] == 0 and ctx.profile("k_response_weight")[0] == 0
        # without keep_response the instrument's transpose alone is still there
        assert no_response.pixel_weights_to_grid(c).shape == (300,)
    for syn in (bare, no_response, no_continuum):
        syn.close()
