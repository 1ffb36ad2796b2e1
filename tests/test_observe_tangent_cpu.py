"""The instrument's tangent at build time and on the host: the six entry points are declared, exported and mirrored; the new kernels
compile for gfx950 without spilled vector registers; a null context is refused; validation raises before any device is asked for; the
restatement (tests/observe_tangent_reference.py) against 50-digit mpmath and by its own properties; and what
tests/test_gpu_observe_tangent.py relies on — the window lengths and mapping estimates of every (grid, R) pair it uses, and the steps
of its difference quotients."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import observe_reference as oref
import observe_tangent_reference as tref
import rotation_reference as rref
from conftest import ROOT
from observe_tangent_reference import FLUX_TOL, LD, RESTATEMENT_TOL, SUM_TOL
from rotation_reference import ROT_TOL
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib, synth
from stardis_amd import constants as K

ENTRIES = {"sdx_observe_tangent_dev": 15, "sdx_observe_tangent_f64": 15, "sdx_observe_response_grad_dev": 9, "sdx_observe_response_grad_f64": 9,
           "sdx_rotate_tangent_dev": 10, "sdx_rotate_tangent_f64": 11}

LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform
IRREGULAR = np.sort(np.random.default_rng(7).uniform(6500.0, 6600.0, 3000))
TWO_DENSITY = np.r_[np.linspace(6500.0, 6550.0, 500, endpoint=False), np.linspace(6550.0, 6600.0, 4000)]
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)
# the GPU file's steps (h, h / 2): km/s of v_rad, relative steps of sigma, steps of eps
V_STEPS, LSF_STEPS, EPS_STEPS = (0.02, 0.01), (0.01, 0.005), (0.02, 0.01)


def test_entry_points_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
    # the Doppler factor, v sin i and eps by value in the host-buffer twins; the device entries read them from device memory
    assert _lib.PROTOTYPES["sdx_observe_tangent_f64"][1][8] is ctypes.c_double and _lib.PROTOTYPES["sdx_observe_tangent_dev"][1][8] is ctypes.c_void_p
    assert _lib.PROTOTYPES["sdx_rotate_tangent_f64"][1][5:7] == [ctypes.c_double] * 2 and _lib.PROTOTYPES["sdx_rotate_tangent_dev"][1][5] is ctypes.c_void_p


def test_tangent_kernels_do_not_spill(resources):  # noqa: F811
    """k_observe_tangent carries erf / erfc, two exp and an expm1 of the device library and eight accumulators: 133 vector registers,
    three waves per SIMD against k_observe's five, no spill, no scratch, no LDS.  k_rotate_tangent keeps k_rotate's eight waves, and
    k_rotate itself its registers (the derivative is compiled out of it)."""
    for name, vgpr, occ in (("k_observe_tangent", 144, 3), ("k_rotate_tangent", 64, 8), ("k_observe_response_grad", 64, 8), ("k_rotate", 52, 8)):
        found = [v for k, v in resources.items() if k == name]
        assert len(found) == 1, sorted(resources)
        print(name, found[0])
        assert found[0]["spill"] == 0 and found[0]["lds"] == 0 and found[0]["occ"] >= occ and found[0]["vgpr"] <= vgpr, (name, found[0])


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    none = [None] * 9
    assert lib.sdx_observe_tangent_dev(None, 4, None, None, None, 3, *none) == -1
    assert b"observe_tangent" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_observe_tangent_f64(None, 4, None, None, None, 3, None, None, 1.0, *none[:6]) == -1
    assert lib.sdx_observe_response_grad_dev(None, 4, *none[:7]) == -1 and b"observe_response_grad" in lib.sdx_last_error_string()
    assert lib.sdx_observe_response_grad_f64(None, 4, *none[:7]) == -1
    assert lib.sdx_rotate_tangent_dev(None, 4, *none[:8]) == -1 and b"rotate_tangent" in lib.sdx_last_error_string()
    assert lib.sdx_rotate_tangent_f64(None, 4, None, None, None, 10.0, 0.6, None, None, None, None) == -1


def test_validation_needs_no_device():
    from stardis_amd import ops
    from stardis_amd.instrument import Instrument

    class Host(Instrument):  # the name checks are plain Python: an instrument without a device
        def __init__(self, v_rot=None, v_mac=None):
            self.rotates, self.macroturbulent, self.v_rot, self.v_mac = v_rot is not None, v_mac is not None, v_rot, v_mac

    with pytest.raises(ValueError, match="v_rad, lsf, v_mac, limb_darkening"):
        Host()._wrt(("v_rad", "v_sin_i"))
    with pytest.raises(RuntimeError, match="no macroturbulence"):
        Host(v_rot=10.0)._wrt("v_mac")
    with pytest.raises(ValueError, match="zeta"):
        Host(v_mac=0.0)._wrt("v_mac")
    with pytest.raises(RuntimeError, match="no rotation"):
        Host(v_mac=3.0)._wrt("limb_darkening")
    with pytest.raises(ValueError, match="v_rot"):
        Host(v_rot=0.0)._wrt("limb_darkening")
    assert Host()._wrt(None) == ("v_rad", "lsf") and Host(v_rot=10.0, v_mac=3.0)._wrt(None) == Instrument.PARAMETERS
    assert Host(v_rot=10.0)._wrt("lsf") == ("lsf",)
    lam, edges = np.linspace(6560.0, 6570.0, 50), np.linspace(6562.0, 6568.0, 11)
    for call in (lambda: ops.observe_tangent(lam[::-1], np.ones(50), edges, 0.05), lambda: ops.observe_tangent(lam, np.ones(49), edges, 0.05),
                 lambda: ops.observe_tangent(lam, np.ones(50), edges, -0.05), lambda: ops.observe_tangent(lam, np.ones(50), edges, 0.05, dreference=np.ones(50)),
                 lambda: ops.observe_tangent(lam, np.ones(50), edges, 0.05, reference=np.ones(50), dreference=np.ones(50)),
                 lambda: ops.observe_tangent(lam, np.ones(50), edges, 0.05, dflux=np.ones(3)), lambda: ops.observe_tangent(lam[:1], np.ones(1), edges, 0.05),
                 lambda: ops.rotate_tangent(lam, np.ones(50), -1.0), lambda: ops.rotate_tangent(lam, np.ones(50), 10.0, limb_darkening=1.5),
                 lambda: ops.rotate_tangent(lam, np.ones(50), 10.0, reference=np.ones(3)), lambda: ops.rotate_tangent(lam[::-1], np.ones(50), 10.0)):
        with pytest.raises(ValueError):
            call()
    if _lib.load().sdx_device_count() == 0:  # valid arguments: then, and only then, the device is asked for (no CPU fallback)
        with pytest.raises(RuntimeError):
            ops.observe_tangent(lam, np.ones(50), edges, 0.05)
        with pytest.raises(RuntimeError):
            ops.rotate_tangent(lam, np.ones(50), 10.0)
        with pytest.raises(RuntimeError):
            ops.observe_response_grad(-1.0, 1.0, 0.0, 1.0)


# ---- the response's partials ---------------------------------------------------------------------------------------------------
def mp_of(v):
    """a longdouble as an mpf, exactly (its two fp64 halves)"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - LD(hi)))


def test_response_gradient_of_the_restatement_against_mpmath():
    """dr/dx and dr/d ln sigma of the restatement (longdouble) against 50 digits on response_grad_points(): both tails out to +-8, pixels
    1e-4 sigma and 1e3 sigma wide, x exactly on an edge and at the pixel's centre.  dr/dx relative to itself, dr/d ln sigma relative to
    PRODUCT_RULE_SCALE (the module's header), both to RESTATEMENT_TOL; a value below fp64's range (-1000 phi(1000)) is excused."""
    mpmath.mp.dps = 50
    a, b = tref.response_grad_points()
    assert a.size == 917 and np.all(a < b) and a.min() <= -1000 and b.max() >= 1000 and np.any(a == 0) and np.any(b == 0) and np.any(a == -b)
    assert np.any((a >= 7.5) & (b - a <= 1.1e-4)) and np.any((b <= -7.5) & (b - a <= 1.1e-4))
    rx, rs = tref.response_grad(a, b, 0.0, 1.0)
    tiny = float(np.finfo(np.float64).tiny)
    worst_x = worst_s = 0.0
    for k in range(a.size):
        _, G, S, scale = tref.mp_response(a[k], b[k])
        if G == 0:
            assert rx[k] == 0
        elif abs(G) > tiny:
            worst_x = max(worst_x, float(abs(mp_of(rx[k]) - G) / abs(G)))
        if scale > tiny:
            worst_s = max(worst_s, float(abs(mp_of(rs[k]) - S) / scale))
    print(f"worst |dr/dx - 50 digits| / |dr/dx| {worst_x:.3e}, worst |dr/d ln sigma - 50 digits| / product-rule scale {worst_s:.3e}, allowed {RESTATEMENT_TOL:.1e}")
    assert 0 < worst_x <= RESTATEMENT_TOL and 0 < worst_s <= RESTATEMENT_TOL
    assert np.any(np.abs(rx.astype(np.float64)) > 0.1) and np.any(np.abs(rs.astype(np.float64)) > 0.1)


def test_response_gradient_is_the_derivative_of_the_response():
    """the closed forms against mpmath.diff of the response itself, at a few (a', b') and a sigma other than 1"""
    mpmath.mp.dps = 50
    for e0, e1, x, s in ((6565.0, 6565.05, 6565.02, 0.03), (6565.0, 6565.05, 6564.9, 0.03), (6565.0, 6565.0001, 6565.1, 0.04), (1.0, 3.0, 9.0, 1.5)):
        r = lambda xx, ss: (mpmath.erf((e1 - xx) / (ss * mpmath.sqrt(2))) - mpmath.erf((e0 - xx) / (ss * mpmath.sqrt(2)))) / 2  # noqa: E731
        dx = mpmath.diff(lambda xx: r(xx, mpmath.mpf(s)), mpmath.mpf(x))
        ds = mpmath.diff(lambda t: r(mpmath.mpf(x), mpmath.mpf(s) * mpmath.exp(t)), 0)
        rx, rs = tref.response_grad(e0, e1, x, s)
        print(f"({e0}, {e1}, {x}, {s}): dr/dx {float(rx)!r} against {float(dx)!r}, dr/d ln sigma {float(rs)!r} against {float(ds)!r}")
        assert abs(float(rx) - float(dx)) <= 1e-14 * abs(float(dx)) and abs(float(rs) - float(ds)) <= 1e-14 * max(abs(float(ds)), abs(float(dx)) * s)


def test_a_constant_has_no_parameter_tangent():
    """a constant flux without reference, and flux == reference with one, observe to the constant; every parameter tangent is a
    cancellation of its absolute terms"""
    s = oref.sigma_of_R(SC2_EDGES, 5.0e4)
    for tag, f, g, expect in (("constant", np.full(LAM.size, 1.7), None, 1.7), ("flux == reference", 2.0 + 0.5 * np.sin(LAM / 3.0), 2.0 + 0.5 * np.sin(LAM / 3.0), 1.0)):
        t = tref.observe_tangent(LAM[:3000], f[:3000], SC2_EDGES[:700], s[:699], oref.doppler_factor(37.5), reference=None if g is None else g[:3000])
        ok = ~np.isnan(t["out"].astype(np.float64))
        assert ok.sum() > 600 and np.max(np.abs(t["out"][ok] / LD(expect) - 1)) <= 1e-15
        for name in ("v_rad", "lsf"):
            ratio = float(np.max(np.abs(t[name][ok]) / t[name + "_terms"][ok]))
            print(f"{tag}: worst |{name}| / absolute terms {ratio:.3e}")
            assert ratio <= SUM_TOL


def test_rotation_rows_are_rotation_reference_s():
    lam = LAM[:400]
    for V, eps in ((10.0, 0.6), (100.0, 0.3)):
        for (i, j, w), (i2, j2, w2, dw) in zip(rref.point_rows(lam, V, eps), tref.rotate_eps_rows(lam, V, eps)):
            assert i == i2 and np.array_equal(j, j2) and np.array_equal(w, w2) and dw.shape == w.shape
    # K is linear in eps: dw is the difference of two w
    w1 = [w for _, _, w in rref.point_rows(lam, 10.0, 1.0)]
    w0 = [w for _, _, w in rref.point_rows(lam, 10.0, 0.0)]
    for a, b, (_, _, _, dw) in zip(w1, w0, tref.rotate_eps_rows(lam, 10.0, 0.4)):
        assert np.max(np.abs((a - b) - dw)) <= 1e-18 * np.max(np.abs(a))


# ---- the GPU file's inputs -----------------------------------------------------------------------------------------------------
def estimate(lam, edges, sigma, doppler=1.0):
    """k_observe's mapping estimate per pixel: the points in the window at the grid's mean spacing"""
    x = lam * doppler
    return (edges[1:] - edges[:-1] + 16.0 * sigma) * (lam.size - 1) / (x[-1] - x[0])


def test_window_lengths_and_mapping_estimates_of_the_gpu_test():
    assert LAM.size == 7634 and SC2_EDGES.size == 2049
    figures = {}
    for R in (2.0e5, 1.2e5, 5.0e4):
        s = oref.sigma_of_R(SC2_EDGES, R)
        n, e = oref.window_lengths(LAM, SC2_EDGES, s), estimate(LAM, SC2_EDGES, s)
        figures[R] = (int(n[n > 0].min()), int(n.max()), round(float(e.min()), 2), round(float(e.max()), 2))
    print(figures)
    assert figures == {2.0e5: (20, 21, 20.44, 20.69), 1.2e5: (31, 32, 31.68, 32.1), 5.0e4: (71, 72, 71.03, 72.03)}
    e = estimate(LAM, SC2_EDGES, oref.sigma_of_R(SC2_EDGES, 1.2e5))
    groups = e[: 2048 // 8 * 8].reshape(-1, 8).max(axis=1)
    assert (groups <= 32).sum() > 50 and (groups > 32).sum() > 50  # eight lanes and a wave per pixel inside one launch
    for v in (37.5, -120.0):  # the Doppler factor moves neither decision
        D = oref.doppler_factor(v)
        assert estimate(LAM, SC2_EDGES, oref.sigma_of_R(SC2_EDGES, 2.0e5), D).max() < 21 and estimate(LAM, SC2_EDGES, oref.sigma_of_R(SC2_EDGES, 5.0e4), D).min() > 70
    # the other grids: the mean-spacing estimate is wrong locally, and either mapping must serve any window
    edges = np.linspace(6505.0, 6595.0, 301)
    s = oref.sigma_of_R(edges, 2.0e4)
    n, e = oref.window_lengths(IRREGULAR, edges, s), estimate(IRREGULAR, edges, s)
    print(f"irregular: windows of {n.min()} .. {n.max()} points, estimate {e.min():.1f} .. {e.max():.1f}")
    assert n.min() > 40 and e.min() > 32
    edges = np.linspace(6505.0, 6595.0, 501)
    n, e = oref.window_lengths(TWO_DENSITY, edges, np.full(500, 0.05)), estimate(TWO_DENSITY, edges, np.full(500, 0.05))
    print(f"two-density: windows of {n.min()} .. {n.max()} points, estimate {e.min():.1f} .. {e.max():.1f}")
    assert n.min() <= 11 and n.max() >= 75 and e.min() > 32  # a wave per pixel also where ten points are there
    n, e = oref.window_lengths(TWO_DENSITY, edges, np.full(500, 0.02)), estimate(TWO_DENSITY, edges, np.full(500, 0.02))
    print(f"two-density, sigma 0.02: windows of {n.min()} .. {n.max()} points, estimate {e.min():.1f} .. {e.max():.1f}")
    assert n.max() >= 38 and e.max() <= 32  # eight lanes per pixel also where forty points are there


def test_difference_quotient_steps_of_the_gpu_test():
    """tests/test_gpu_observe_tangent.py holds the device's dout_velocity, dout_lsf and dout_eps against Richardson-extrapolated central
    differences of the device's own forward at v +- h, sigma (1 +- h) and eps +- h and allows |coarse - fine| + TOL scale / h (TOL =
    FLUX_TOL for the pixel stage, ROT_TOL for the rotation; scale = max |F|, or max |out| with a reference).  Where the first term
    cancels the second must cover the Richardson value's remainder: at these steps the RESTATEMENT's own remainder stays below it at
    every covered pixel.  Measured, remainder against room: v_rad at (0.02, 0.01) km/s 1.6e-10 against 6.9e-09 (R = 5e4) and 7.1e-10
    against 6.9e-09 (R = 2e5) — below 0.02 km/s the fp64 forward's own rounding over h takes over (2.4e-09 at h = 0.005); ln kappa at
    (0.01, 0.005) 2.5e-10 and 9.2e-11 against 1.4e-08; eps at (0.02, 0.01) 1.0e-11 (V = 10) and 2.1e-12 (V = 100) against 6.8e-10.
    out is a ratio of two functions linear in eps, not linear itself: one quotient at h = 0.1 is off by 1.6e-05."""
    f = 1.0 + 0.1 * np.random.default_rng(11).standard_normal(LAM.size)  # (the GPU file's flux)
    g = 2.0 + 0.5 * np.sin(LAM / 3.0)
    v0 = 37.5
    D = oref.doppler_factor(v0)
    for R, ref in ((5.0e4, None), (2.0e5, None), (5.0e4, g)):
        s = oref.sigma_of_R(SC2_EDGES, R)
        t = tref.observe_tangent(LAM, f, SC2_EDGES, s, D, reference=ref)
        scale = float(np.abs(f).max() if ref is None else np.nanmax(np.abs(t["out"].astype(np.float64))))
        forward = {"v_rad": lambda h: oref.observe(LAM, f, SC2_EDGES, s, oref.doppler_factor(v0 + h), reference=ref),  # noqa: B023
                   "lsf": lambda h: oref.observe(LAM, f, SC2_EDGES, s * (1 + h), D, reference=ref)}  # noqa: B023
        for name, steps in (("v_rad", V_STEPS), ("lsf", LSF_STEPS)):
            q = [(forward[name](h) - forward[name](-h)) / (2 * h) for h in steps]
            rich = (4 * q[1] - q[0]) / 3
            ok = ~np.isnan(rich) & ~np.isnan(t[name].astype(np.float64))
            remainder, room = float(np.max(np.abs(t[name][ok] - rich[ok]))), FLUX_TOL * scale / steps[0]
            print(f"R = {R:.0e}{', reference' if ref is not None else ''}, {name}: the Richardson value's remainder {remainder:.3e} against FLUX_TOL scale / h = {room:.3e}")
            assert ok.sum() > 1900 and remainder < room and float(np.max(np.abs(t[name][ok]))) > 100 * room
    lam, fl = LAM[:2500], f[:2500]
    for V in (10.0, 100.0):
        d = tref.rotate_tangent(lam, fl, V, 0.5)[0]
        q = [(rref.rotate(lam, fl, V, 0.5 + h)[0] - rref.rotate(lam, fl, V, 0.5 - h)[0]) / (2 * h) for h in EPS_STEPS]
        remainder, room = float(np.max(np.abs(d - (4 * q[1] - q[0]) / 3))), ROT_TOL * float(np.abs(fl).max()) / EPS_STEPS[0]
        single = float(np.max(np.abs(d - (rref.rotate(lam, fl, V, 0.6)[0] - rref.rotate(lam, fl, V, 0.4)[0]) / 0.2)))
        print(f"V = {V}, eps: the Richardson value's remainder {remainder:.3e} against ROT_TOL max |F| / h = {room:.3e}; one quotient at h = 0.1 is off by {single:.3e}")
        assert remainder < room and float(np.max(np.abs(d))) > 100 * room and single > 100 * room
