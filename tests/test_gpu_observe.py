"""The instrument model on the device (k_observe: Doppler shift, line-spread function, pixel integration) against its numpy
restatement (tests/observe_reference.py), to the project's FLUX_TOL = 1e-10 of |ref| with coinciding NaN patterns; identities between
reordered sums to SUM_TOL = 1e-12; bit-for-bit determinism, graph replay and the device-resident radial velocity; the host-buffer
twin and its validation; the engine option, DeviceSpectrum.observed and run_stardis(..., instrument=)."""
import ctypes as C
import types

import numpy as np
import pytest

import observe_reference as oref
from observe_reference import FLUX_TOL, SUM_TOL
from stardis_amd import _lib, ops, synth
from stardis_amd import constants as K
from stardis_amd.engine import SpectralSynthesizer
from stardis_amd.instrument import Instrument
from stardis_amd.postprocess import DeviceSpectrum

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace

# the S-c2 grid as wavelengths (ascending), 7634 points about 0.013 A apart
LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))
FLUX = 1.0 + 0.1 * np.random.default_rng(2024).standard_normal(LAM.size)
DX = float(np.median(np.diff(LAM)))


def device(ctx, lam, flux, edges, sigma, v=0.0, reference=None):
    inst = Instrument(edges, sigma=sigma, ctx=ctx)
    if v:
        inst.set_radial_velocity(v)
    return inst.observe_host(lam, flux, reference)


def compare(tag, got, ref, expect_nan=0):
    """print, then assert: the same NaN pixels (expect_nan of them) and FLUX_TOL of |ref| elsewhere"""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    ok = ~nan_r
    err = float(np.max(np.abs(got[ok & ~nan_g] - ref[ok & ~nan_g]) / np.abs(ref[ok & ~nan_g]))) if (ok & ~nan_g).any() else 0.0
    print(f"{tag}: {ref.size} pixels, NaN device {int(nan_g.sum())} / restatement {int(nan_r.sum())}, max rel err {err:.3e}")
    assert int(nan_r.sum()) == expect_nan
    assert np.array_equal(nan_g, nan_r)
    assert err <= FLUX_TOL
    return err


def check(ctx, tag, lam, flux, edges, sigma, v=0.0, expect_nan=0):
    D = oref.doppler_factor(v)
    assert oref.clear_of_grid_ends(lam, edges, sigma, D)
    got = device(ctx, lam, flux, edges, sigma, v)
    compare(tag, got, oref.observe(lam, flux, edges, sigma, D), expect_nan)
    return got


# ---- 1, 2: the two grids users pass ------------------------------------------------------------------------------------------------
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)
SC2_SIGMA = oref.sigma_of_R(SC2_EDGES, 5.0e4)


def test_sc2_grid_2048_pixels_three_velocities(ctx):
    got = {v: check(ctx, f"S-c2 grid, R = 50000, v = {v:+.0f} km/s", LAM, FLUX, SC2_EDGES, SC2_SIGMA, v) for v in (-30.0, 0.0, 30.0)}
    moved = np.max(np.abs(got[30.0] - got[0.0]))
    print(f"max |observed(+30) - observed(0)| = {moved:.3e}")
    assert moved > 1e-3


def test_linear_grid_unequal_pixels_random_resolving_power(ctx):
    rng = np.random.default_rng(7)
    lam = np.arange(6560.0, 6570.0, 0.01)
    flux = 1.0 + 0.1 * rng.standard_normal(lam.size)
    widths = rng.uniform(0.02, 0.1, 119)
    edges = 6562.6 + np.r_[0.0, np.cumsum(widths)] * (4.8 / widths.sum())  # (8 sigma is up to 2.23 A at R = 10000)
    sigma = oref.sigma_of_R(edges, rng.uniform(1.0e4, 4.0e4, 119))
    check(ctx, "linear grid, 119 unequal pixels", lam, flux, edges, sigma)
    check(ctx, "linear grid, 119 unequal pixels, v = -12.5", lam, flux, edges, sigma, v=-12.5)


# ---- 3: window lengths where the lane mapping can go wrong -------------------------------------------------------------------------
def sigma_for_counts(lam, edges, counts):
    """per pixel the sigma whose window [e0 - 8 sigma, e1 + 8 sigma] holds exactly counts[j] grid points"""
    sigma = np.empty(len(counts))
    for j, want in enumerate(counts):
        e0, e1 = edges[j], edges[j + 1]
        guess = max(((want - 0.5) * DX - (e1 - e0)) / 16.0, 1e-4 * DX)
        for s in guess * np.linspace(0.5, 1.5, 2001):
            if np.searchsorted(lam, e1 + 8 * s, "right") - np.searchsorted(lam, e0 - 8 * s, "left") == want:
                sigma[j] = s
                break
        else:
            raise AssertionError(f"no sigma gives pixel {j} a window of {want} points")
    assert np.array_equal(oref.window_lengths(lam, edges, sigma), counts)
    return sigma


def test_undersampled_line_spread_function(ctx):
    """sigma = 0.004 A: about five grid points under the line-spread function plus the pixel's own (several pixels per wave)"""
    edges = np.linspace(6540.0, 6550.0, 201)
    n = oref.window_lengths(LAM, edges, 0.004)
    print(f"points per window {n.min()} .. {n.max()}")
    assert 5 <= n.min() and n.max() <= 12
    check(ctx, "sigma = 0.004 A, 0.05 A pixels", LAM, FLUX, edges, 0.004)


def test_pixels_narrower_than_a_grid_step(ctx):
    edges = np.linspace(6540.0, 6542.0, 401)  # 0.005 A pixels on a 0.013 A grid
    assert np.diff(edges).max() < np.diff(LAM).min()
    n = oref.window_lengths(LAM, edges, 0.004)
    print(f"points per window {n.min()} .. {n.max()}")
    check(ctx, "0.005 A pixels, sigma = 0.004 A", LAM, FLUX, edges, 0.004)


@pytest.mark.parametrize("counts", [
    [63, 64, 65, 128, 129, 64, 63, 65],                         # around one and two trips of a 64-lane pixel
    [32, 5, 17, 8, 9, 1, 2, 31, 36, 5, 17, 8, 9, 1, 2, 31],     # a group at the several-pixels-per-wave limit, and one above it
    [1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 32, 3],              # around one, two, three, four trips of an 8-lane segment; a short last group
    [129, 3, 3],                                                # one long window makes its whole group take a wave per pixel
], ids=["63-129", "32|33", "segments", "mixed"])
def test_exact_window_lengths(ctx, counts):
    counts = np.array(counts)
    edges = 6545.0 + 0.6 * DX * np.arange(counts.size + 1)
    sigma = sigma_for_counts(LAM, edges, counts)
    check(ctx, f"windows of exactly {counts.tolist()} points", LAM, FLUX, edges, sigma)


LONG_EDGES = np.linspace(6520.0, 6580.0, 17)
LONG_SIGMA = oref.sigma_of_R(LONG_EDGES, 3000.0)


def test_long_windows(ctx):
    n = oref.window_lengths(LAM, LONG_EDGES, LONG_SIGMA)
    print(f"points per window {n.min()} .. {n.max()}")
    assert n.min() > 1400
    check(ctx, "16 pixels at R = 3000", LAM, FLUX, LONG_EDGES, LONG_SIGMA)


@pytest.mark.parametrize("n_pix", [1, 2, 63, 65])
def test_pixel_counts(ctx, n_pix):
    edges = np.linspace(6540.0, 6560.0, n_pix + 1)
    check(ctx, f"n_pix = {n_pix}", LAM, FLUX, edges, oref.sigma_of_R(edges, 5.0e4))
    short = 6540.0 + 0.05 * np.arange(n_pix + 1)
    check(ctx, f"n_pix = {n_pix}, short windows", LAM, FLUX, short, 0.004)


def test_two_point_grid(ctx):
    """n = 2: a window inside the grid holds neither point (0 / 0), any other is not covered — NaN either way, as in the restatement"""
    flux = np.array([1.0, 3.0])
    cases = (("covered, empty window", [6500.0, 6600.0], [6549.0, 6551.0], 0.5), ("reaches below the grid", [6500.0, 6600.0], [6549.0, 6551.0], 10.0),
             ("holds both points", [6549.97, 6550.03], [6549.95, 6550.05], 0.005), ("above the grid", [6500.0, 6510.0], [6549.0, 6551.0], 0.5))
    for tag, lam, edges, sigma in cases:
        lam, edges = np.array(lam), np.array(edges)
        assert oref.clear_of_grid_ends(lam, edges, sigma)
        got, ref = device(ctx, lam, flux, edges, sigma), oref.observe(lam, flux, edges, sigma)
        print(f"n = 2, {tag}: device {got}, restatement {ref}")
        assert np.isnan(ref).all() and np.array_equal(np.isnan(got), np.isnan(ref))
    # n = 3: the first pixel's window holds the middle point and nothing else, the second's holds none
    lam, edges = np.array([6549.0, 6550.0, 6551.0]), np.array([6549.9, 6550.1, 6550.3])
    compare("n = 3", device(ctx, lam, np.array([1.0, 3.0, 2.0]), edges, 0.01), oref.observe(lam, np.array([1.0, 3.0, 2.0]), edges, 0.01), expect_nan=1)


def test_two_density_grid(ctx):
    """The mapping is chosen from the windows' expected lengths at the grid's MEAN spacing.  On a grid with a dense stretch the pixels
    mapped eight to a wave meet windows of a hundred points, and the pixels mapped one to a wave windows of sixteen."""
    rng = np.random.default_rng(5)
    lam = np.r_[np.arange(6500.0, 6540.0, 0.05), np.arange(6540.0, 6560.0, 0.002), np.arange(6560.0, 6600.001, 0.05)]
    flux = 1.0 + 0.1 * rng.standard_normal(lam.size)
    mean = (lam[-1] - lam[0]) / (lam.size - 1)
    for tag, edges, sigma, short_mapping in (("dense stretch", 6545.0 + 0.01 * np.arange(41), 0.012, True), ("coarse stretch", np.linspace(6510.0, 6530.0, 41), 0.02, False)):
        expected = (np.diff(edges) + 16 * sigma) / mean
        n = oref.window_lengths(lam, edges, sigma)
        print(f"{tag}: expected {expected.min():.1f} .. {expected.max():.1f} points per window, in fact {n.min()} .. {n.max()}")
        assert (expected.max() <= 32 and n.min() > 64) if short_mapping else (expected.min() > 32 and n.max() <= 32)
        check(ctx, "two-density grid, " + tag, lam, flux, edges, sigma)


def test_irregular_grid(ctx):
    rng = np.random.default_rng(99)
    lam = 6500.0 + np.cumsum(rng.uniform(0.003, 0.03, 6000))
    flux = 1.0 + 0.1 * rng.standard_normal(lam.size)
    edges = np.linspace(lam[0] + 2.0, lam[-1] - 2.0, 301)
    check(ctx, "irregular grid, R = 40000", lam, flux, edges, oref.sigma_of_R(edges, 4.0e4))
    check(ctx, "irregular grid, sigma = 0.006 A", lam, flux, edges[:120] * 1.0, 0.006)


# ---- 4: coverage -------------------------------------------------------------------------------------------------------------------
def test_partly_covered_pixels_are_nan(ctx):
    edges = np.linspace(6499.0, 6601.0, 301)
    got = check(ctx, "300 pixels over 6499 - 6601", LAM, FLUX, edges, oref.sigma_of_R(edges, 5.0e4), expect_nan=10)
    assert np.isnan(got[:5]).all() and np.isnan(got[-5:]).all() and not np.isnan(got[5:-5]).any()
    for lo, hi in ((6400.0, 6450.0), (6650.0, 6700.0)):
        edges = np.linspace(lo, hi, 7)
        out = check(ctx, f"pixels over {lo:.0f} - {hi:.0f}", LAM, FLUX, edges, oref.sigma_of_R(edges, 5.0e4), expect_nan=6)
        assert np.isnan(out).all()


# ---- 5, 6: identities --------------------------------------------------------------------------------------------------------------
def test_flat_spectrum(ctx):
    flat = np.full(LAM.size, 3.25)
    for tag, edges, sigma in (("short windows", np.linspace(6540.0, 6550.0, 201), 0.004), ("1425-point windows", LONG_EDGES, LONG_SIGMA)):
        got = device(ctx, LAM, flat, edges, sigma)
        err = np.max(np.abs(got / 3.25 - 1.0))
        print(f"flat spectrum, {tag}: max |out / 3.25 - 1| = {err:.3e}")
        assert not np.isnan(got).any() and err <= SUM_TOL


def test_reference_is_the_ratio_of_two_observations(ctx):
    g = 2.0 + 0.5 * np.sin(LAM / 3.0)
    for tag, edges, sigma in (("R = 50000", SC2_EDGES, SC2_SIGMA), ("short windows", np.linspace(6540.0, 6550.0, 201), 0.004), ("long", LONG_EDGES, LONG_SIGMA)):
        both = device(ctx, LAM, FLUX * g, edges, sigma, v=30.0, reference=g)
        ratio = device(ctx, LAM, FLUX * g, edges, sigma, v=30.0) / device(ctx, LAM, g, edges, sigma, v=30.0)
        one = device(ctx, LAM, FLUX, edges, sigma, reference=FLUX)
        e1, e2 = np.max(np.abs(both - ratio) / np.abs(ratio)), np.max(np.abs(one - 1.0))
        print(f"{tag}: observe(f, g) against observe(f) / observe(g) {e1:.3e}; observe(f, f) against 1 {e2:.3e}")
        assert e1 <= SUM_TOL and e2 <= SUM_TOL
        compare(tag + ", with reference", both, oref.observe(LAM, FLUX * g, edges, sigma, oref.doppler_factor(30.0), reference=g))
    assert np.array_equal(ops.observe(LAM, FLUX * g, SC2_EDGES, SC2_SIGMA, v_rad=30.0, reference=g, ctx=ctx),
                          device(ctx, LAM, FLUX * g, SC2_EDGES, SC2_SIGMA, v=30.0, reference=g))


# ---- 7: determinism and graphs -----------------------------------------------------------------------------------------------------
def test_bits_repeat_and_graphs_follow_the_velocity(ctx):
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx)
    assert np.array_equal(inst.sigma, SC2_SIGMA)
    d_lam, d_f = ctx.upload(LAM), ctx.upload(FLUX)
    eager0 = inst.observe(d_lam, d_f, LAM.size).numpy()
    again = inst.observe(d_lam, d_f, LAM.size).numpy()
    print(f"two eager runs differ in {int(np.sum(eager0 != again))} pixels")
    assert np.array_equal(eager0, again) and not np.isnan(eager0).any()
    inst.set_radial_velocity(30.0)
    eager30 = inst.observe(d_lam, d_f, LAM.size).numpy()
    assert not np.array_equal(eager30, eager0)
    inst.set_radial_velocity(0.0)
    ctx.call("sdx_graph_begin")
    try:
        inst.observe(d_lam, d_f, LAM.size)
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    try:
        inst.d_out.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = inst.d_out.numpy()
        inst.set_radial_velocity(30.0)  # no new capture: the kernel reads the factor from device memory
        ctx.call("sdx_graph_launch", graph)
        replay30 = inst.d_out.numpy()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    print(f"replay against eager: v = 0 differs in {int(np.sum(replay0 != eager0))} pixels, v = 30 in {int(np.sum(replay30 != eager30))}")
    assert np.array_equal(replay0, eager0) and np.array_equal(replay30, eager30)
    compare("eager v = 30", eager30, oref.observe(LAM, FLUX, SC2_EDGES, SC2_SIGMA, oref.doppler_factor(30.0)))


# ---- 8: the host-buffer twin ---------------------------------------------------------------------------------------------------------
def test_host_twin_bits_and_validation(ctx):
    lib = ctx.lib
    edges = np.linspace(6540.0, 6560.0, 66)
    sigma = oref.sigma_of_R(edges, 5.0e4)
    D = oref.doppler_factor(30.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def twin(lam=LAM, flux=FLUX, edges=edges, sigma=sigma, doppler=D, n=None, out=True, reference=None):
        res = np.full(sigma.size, -7.0)
        rc = lib.sdx_observe_f64(ctx.handle, lam.size if n is None else n, p(lam), p(flux), None if reference is None else p(reference),
                                 sigma.size, p(edges), p(sigma), doppler, p(res) if out else None)
        return rc, res

    expect = device(ctx, LAM, FLUX, edges, sigma, v=30.0)
    rc, got = twin()
    assert rc == 0
    print(f"host twin against the device path: {int(np.sum(got != expect))} pixels differ")
    assert np.array_equal(got, expect)
    rc, got_ref = twin(reference=FLUX)
    assert rc == 0 and np.array_equal(got_ref, device(ctx, LAM, FLUX, edges, sigma, v=30.0, reference=FLUX))

    repeated = edges.copy()
    repeated[10] = repeated[9]
    with_nan = edges.copy()
    with_nan[20] = np.nan
    zero_sigma = sigma.copy()
    zero_sigma[3] = 0.0
    bad = dict(
        lambdas=dict(lam=np.ascontiguousarray(LAM[::-1])), edges=dict(edges=repeated), sigma=dict(sigma=zero_sigma), doppler=dict(doppler=0.0),
        nan_edge=dict(edges=with_nan), n_1=dict(n=1), null_out=dict(out=False), inf_doppler=dict(doppler=np.inf), nan_lambda=dict(lam=np.r_[LAM[:-1], np.nan]),
    )
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        for tag, kw in bad.items():
            rc, res = twin(**kw)
            msg = lib.sdx_last_error_string().decode()
            print(f"{tag}: rc {rc}, '{msg}'")
            assert rc == -1 and lib.sdx_last_error_code() == -1 and "observe" in msg
            assert np.all(res == -7.0)
            named = {"nan_edge": "edges", "n_1": "n >= 2", "null_out": "out", "inf_doppler": "doppler", "nan_lambda": "lambdas"}.get(tag, tag)
            assert named in msg
        ctx.synchronize()
        launches = ctx.profile("k_observe")[0]
        # the device entry point's own refusals
        d = ctx.upload(LAM)
        for args in ((1, d.ptr, d.ptr, None, 4, d.ptr, d.ptr, None, d.ptr), (LAM.size, d.ptr, d.ptr, None, 4, d.ptr, d.ptr, None, None),
                     (LAM.size, None, d.ptr, None, 4, d.ptr, d.ptr, None, d.ptr), (LAM.size, d.ptr, d.ptr, None, -1, d.ptr, d.ptr, None, d.ptr)):
            assert lib.sdx_observe_dev(ctx.handle, *args) == -1
        assert lib.sdx_observe_dev(ctx.handle, LAM.size, None, None, None, 0, None, None, None, None) == 0  # n_pix = 0: at once
        ctx.synchronize()
        launches += ctx.profile("k_observe")[0]
    finally:
        ctx.call("sdx_profile_enable", 0)
    print(f"k_observe launches during the refusals: {launches}")
    assert launches == 0
    rc, after = twin()
    assert rc == 0 and np.array_equal(after, expect)


# ---- 9: the engine -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sc2():
    w = synth.make_workload("S-c2")
    atm = w["atm"]
    return w, (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])


STAGES = ("k_dnu_partial", "k_prepass_continuum", "k_hlist", "k_line_far", "k_reduce_partials", "k_total_alphas", "k_raytrace", "k_contribution",
          "k_flux_nu_to_lambda", "k_divide", "k_convolve1d_reflect", "k_bf_coef", "k_classify", "k_far_ranges")


def profiled_step(ctx, syn):
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        syn.enqueue()
        ctx.synchronize()
        return {k: ctx.profile(k)[0] for k in STAGES + ("k_observe",)}
    finally:
        ctx.call("sdx_profile_enable", 0)


def restated(syn, inst, continuum=False):
    """the restatement fed the synthesizer's own F_lambda (and continuum F_lambda)"""
    lam = K.nu_to_angstrom(syn.nus_host)
    f = syn.F_nu()[-1] * syn.nus_host / lam
    g = syn.F_nu_continuum[-1] * syn.nus_host / lam if continuum else None
    return oref.observe(lam, f, inst.edges, inst.sigma, inst.doppler, reference=g)


def test_engine_option(ctx, sc2):
    w, args = sc2
    assert np.array_equal(K.nu_to_angstrom(w["nus"]), LAM)
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx)
    inst.set_radial_velocity(30.0)
    off, on = SpectralSynthesizer(*args, ctx=ctx), SpectralSynthesizer(*args, ctx=ctx, instrument=inst)
    n_off, n_on = profiled_step(ctx, off), profiled_step(ctx, on)
    print("launches off", n_off, "\nlaunches on ", n_on)
    assert n_off["k_observe"] == 0 and n_off["k_flux_nu_to_lambda"] == 0
    assert n_on["k_observe"] == 1 and n_on["k_flux_nu_to_lambda"] == 1
    assert {k: v for k, v in n_on.items() if k not in ("k_observe", "k_flux_nu_to_lambda")} == {k: v for k, v in n_off.items() if k not in ("k_observe", "k_flux_nu_to_lambda")}
    assert n_off["k_raytrace"] >= 1
    for name in ("F_nu", "total_alphas", "alpha_line"):
        assert np.array_equal(getattr(on, name)(), getattr(off, name)()), name
    observed = on.observed.numpy()
    assert observed.shape == (2048,)
    assert np.array_equal(DeviceSpectrum(on).observed(inst).numpy(), observed)
    compare("engine, observed", observed, restated(on, inst))
    with pytest.raises(RuntimeError):
        off.observed
    with pytest.raises(RuntimeError):
        on.observed_normalized
    # replays of a captured step and of a captured batch equal the eager step
    on.capture(batch=2)
    try:
        for run in (on.step, on.step_batch):
            on.d_observed.zero()
            run()
            assert np.array_equal(on.observed.numpy(), observed), run.__name__
        inst.set_radial_velocity(0.0)  # a recorded step follows the velocity
        on.step()
        compare("engine, replay after set_radial_velocity(0)", on.observed.numpy(), restated(on, inst))
        assert not np.array_equal(on.observed.numpy(), observed)
    finally:
        on.close()
    with pytest.raises(ValueError, match="whole spectrum"):
        SpectralSynthesizer(*args, ctx=ctx, instrument=inst, shard=(0, 4000))
    with pytest.raises(ValueError, match="context"):
        SpectralSynthesizer(*args, ctx=_lib.Context(ctx.device), instrument=inst)


def test_engine_with_continuum_and_mixed_precision(ctx, sc2):
    w, args = sc2
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx)
    inst.set_radial_velocity(-30.0)
    off = SpectralSynthesizer(*args, ctx=ctx, keep_continuum_flux=True)
    on = SpectralSynthesizer(*args, ctx=ctx, keep_continuum_flux=True, instrument=inst)
    off.step()
    n_on = profiled_step(ctx, on)
    assert n_on["k_observe"] == 2 and n_on["k_flux_nu_to_lambda"] == 2
    for name in ("F_nu", "total_alphas", "alpha_line"):
        assert np.array_equal(getattr(on, name)(), getattr(off, name)()), name
    assert np.array_equal(on.F_nu_continuum, off.F_nu_continuum)
    observed, normalized = on.observed.numpy(), on.observed_normalized.numpy()
    compare("engine + continuum, observed", observed, restated(on, inst))
    compare("engine + continuum, observed_normalized", normalized, restated(on, inst, continuum=True))
    spec = DeviceSpectrum(on)
    assert np.array_equal(spec.observed(inst, normalized=True).numpy(), normalized) and np.array_equal(spec.observed(inst).numpy(), observed)
    assert 0.0 < normalized.min() and normalized.max() <= 1.0 + 1e-9
    with pytest.raises(RuntimeError):
        DeviceSpectrum(SpectralSynthesizer(*args, ctx=ctx)).observed(inst, normalized=True)
    try:
        ctx.set_option("mixed_precision", 1)
        mixed = SpectralSynthesizer(*args, ctx=ctx, instrument=inst)
        mixed.step()
        got = mixed.observed.numpy()
        compare("engine, mixed_precision = 1 (the observation stays fp64)", got, restated(mixed, inst))
    finally:
        ctx.set_option("mixed_precision", 0)
    assert not np.array_equal(got, observed)  # the mode really ran: another flux, observed to the same tolerance


# ---- 10: the drop-in ---------------------------------------------------------------------------------------------------------------
def test_run_stardis_carries_the_observed_spectra(ctx, monkeypatch):
    import stardis_amd.base as gpu_base
    from test_gpu_run_stardis import Quantity, install_stubs

    lambdas = np.arange(6555.0, 6575.0, 0.02)
    nus = K.C_CGS * 1.0e8 / lambdas
    plasma, model, config, _ = synth.fake_plasma(nus, synth.solar_atmosphere(), 300, seed=43)
    config.n_threads = 2
    config.result_options = NS(return_model=False, return_plasma=False, return_radiation_field=False)
    install_stubs(monkeypatch, plasma, model, config, [])
    inst = Instrument(np.linspace(6558.0, 6572.0, 101), resolving_power=2.0e4, ctx=ctx)
    inst.set_radial_velocity(12.0)
    sim = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"), instrument=inst, continuum=True)
    lam, f, g = sim.lambdas.value, np.asarray(sim.spectrum_lambda), np.asarray(sim.spectrum_lambda_continuum)
    assert sim.spectrum_observed.shape == sim.spectrum_observed_normalized.shape == (100,)
    compare("run_stardis, spectrum_observed", sim.spectrum_observed, oref.observe(lam, f, inst.edges, inst.sigma, inst.doppler))
    compare("run_stardis, spectrum_observed_normalized", sim.spectrum_observed_normalized, oref.observe(lam, f, inst.edges, inst.sigma, inst.doppler, reference=g))
    only = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"), instrument=inst)
    assert np.array_equal(only.spectrum_observed, sim.spectrum_observed) and not hasattr(only, "spectrum_observed_normalized")
    plain = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"))
    assert not hasattr(plain, "spectrum_observed") and not hasattr(plain, "spectrum_observed_normalized")
    assert np.array_equal(plain.spectrum_nu, sim.spectrum_nu)
