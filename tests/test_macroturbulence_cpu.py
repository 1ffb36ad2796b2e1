"""Radial-tangential macroturbulence at build time and on the host: the four entry points are declared, exported and mirrored; the
three kernels compile for gfx950 without spilled vector registers; validation raises before any device is asked for; the properties of
the restatement (tests/macroturbulence_reference.py) that pin the definition the device is held against — K and s against 40-digit
mpmath, the profile's area, s = -u dK/du, the derivative outputs against difference quotients in ln zeta, the transpose — and the
window lengths and mapping estimates that tests/test_gpu_macroturbulence.py relies on."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest
from scipy.integrate import quad

import macroturbulence_reference as mref
from conftest import ROOT
from macroturbulence_reference import LD, MACRO_TOL, SUM_TOL
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib, synth
from stardis_amd import constants as K

ENTRIES = {"sdx_macroturbulence_dev": 10, "sdx_macroturbulence_f64": 10, "sdx_macroturbulence_adjoint_dev": 9, "sdx_macroturbulence_adjoint_f64": 9}

LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform


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
    # zeta by value in the host-buffer twins; the device entries read it from device memory
    assert _lib.PROTOTYPES["sdx_macroturbulence_f64"][1][5] is ctypes.c_double and _lib.PROTOTYPES["sdx_macroturbulence_adjoint_f64"][1][3] is ctypes.c_double
    assert _lib.PROTOTYPES["sdx_macroturbulence_dev"][1][5] is ctypes.c_void_p and _lib.PROTOTYPES["sdx_macroturbulence_adjoint_dev"][1][3] is ctypes.c_void_p


def test_macroturbulence_kernels_do_not_spill(resources):  # noqa: F811
    """the figures DESIGN.md quotes: the fp64 exp and erfc of the device library take 128, 112 and 106 vector registers — four waves
    per SIMD, as many as a 256-thread block needs to place two blocks per CU — no spill, no scratch, no LDS"""
    for name, vgpr in (("k_macroturbulence", 128), ("k_macroturbulence_adjoint_den", 128), ("k_macroturbulence_adjoint", 128)):
        found = [v for k, v in resources.items() if k == name]
        assert len(found) == 1, sorted(resources)
        print(name, found[0])
        assert found[0]["spill"] == 0 and found[0]["lds"] == 0 and found[0]["occ"] >= 4 and found[0]["vgpr"] <= vgpr, (name, found[0])


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_macroturbulence_dev(None, 4, None, None, None, None, None, None, None, None) == -1
    assert b"macroturbulence" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_macroturbulence_f64(None, 4, None, None, None, 3.0, None, None, None, None) == -1
    assert lib.sdx_macroturbulence_adjoint_dev(None, 4, None, None, None, None, None, None, None) == -1
    assert b"macroturbulence_adjoint" in lib.sdx_last_error_string()
    assert lib.sdx_macroturbulence_adjoint_f64(None, 4, None, 3.0, None, None, None, None, None) == -1


def test_validation_needs_no_device():
    from stardis_amd import ops
    from stardis_amd.instrument import Instrument, macroturbulence_zeta

    edges = np.linspace(6560.0, 6570.0, 11)
    assert macroturbulence_zeta(0.0) == 0.0 and macroturbulence_zeta(4.5) == 4.5 and macroturbulence_zeta(499.0) == 499.0
    for bad in (-1.0, np.nan, np.inf, 500.0, "wide"):
        with pytest.raises(ValueError, match="v_mac"):
            macroturbulence_zeta(bad)
        with pytest.raises(ValueError, match="v_mac"):
            Instrument(edges, resolving_power=5e4, v_mac=bad)
    lam = np.linspace(6560.0, 6570.0, 50)
    for call in (lambda: ops.macroturbulence(lam, np.ones(50), -3.0), lambda: ops.macroturbulence(lam[::-1], np.ones(50), 3.0),
                 lambda: ops.macroturbulence(lam, np.ones(49), 3.0), lambda: ops.macroturbulence(lam, np.ones(50), 3.0, reference=np.ones(3)),
                 lambda: ops.macroturbulence(lam[:1], np.ones(1), 3.0), lambda: ops.observe(lam, np.ones(50), edges, 0.05, v_mac=-1.0),
                 lambda: ops.observe_adjoint(lam, np.ones(10), edges, 0.05, v_mac=500.0)):
        with pytest.raises(ValueError):
            call()
    if _lib.load().sdx_device_count() == 0:  # valid arguments: then, and only then, the device is asked for (no CPU fallback)
        with pytest.raises(RuntimeError):
            ops.macroturbulence(lam, np.ones(50), 3.0)


# ---- the profile -----------------------------------------------------------------------------------------------------------------
def mp_K(u):
    return mpmath.exp(-u * u) - mpmath.sqrt(mpmath.pi) * u * mpmath.erfc(u)


def test_profile_against_mpmath():
    """K and s of the restatement (fp64, scipy's erfc) against 40 digits on u in [0, 7], to 1e-15 of the peak K(0) = 1"""
    mpmath.mp.dps = 40
    u = np.r_[np.linspace(0.0, 7.0, 1401), np.random.default_rng(2).uniform(0.0, 7.0, 600), 6.0]
    Kd, sd = mref.profile(u)
    exact_K = [mp_K(mpmath.mpf(float(x))) for x in u]
    exact_s = [mpmath.sqrt(mpmath.pi) * mpmath.mpf(float(x)) * mpmath.erfc(mpmath.mpf(float(x))) for x in u]
    err_K = max(abs(float(mpmath.mpf(float(a)) - b)) for a, b in zip(Kd, exact_K))
    err_s = max(abs(float(mpmath.mpf(float(a)) - b)) for a, b in zip(sd, exact_s))
    print(f"worst |K - K_40| {err_K:.3e}, worst |s - s_40| {err_s:.3e}, K(6) = {float(mp_K(mpmath.mpf(6))):.3e}")
    assert err_K <= 1e-15 and err_s <= 1e-15
    assert Kd[0] == 1.0 and sd[0] == 0.0 and np.all(Kd > 0) and np.all(np.diff(Kd[:1401]) < 0)
    assert 3.0e-18 < float(mp_K(mpmath.mpf(6))) < 3.2e-18
    # K ~ exp(-u^2) / (2 u^2) for large u
    assert abs(float(mp_K(mpmath.mpf(6)) / (mpmath.exp(-36) / 72)) - 1) < 0.05


def test_profile_area_and_tail():
    """integral of K du = sqrt(pi) / 4 per side; the mass beyond u = 6 is 5.6e-19 of it"""
    mpmath.mp.dps = 40
    area = mpmath.quad(mp_K, [0, 1, 3, 6, mpmath.inf])
    tail = mpmath.quad(mp_K, [6, 8, mpmath.inf]) / area
    print(f"area {float(area)!r} against sqrt(pi) / 4 = {float(mpmath.sqrt(mpmath.pi) / 4)!r}; tail beyond 6: {float(tail):.3e}")
    assert abs(area - mpmath.sqrt(mpmath.pi) / 4) < mpmath.mpf(10) ** -30 and 5.0e-19 < tail < 6.0e-19
    got = quad(lambda x: float(mref.profile(x)[0]), 0.0, 6.0, epsabs=1e-14, epsrel=0.0)[0]  # the restatement's own K
    assert abs(got - np.sqrt(np.pi) / 4) <= 1e-13
    assert abs(quad(lambda x: float(mref.profile(x)[1]), 0.0, 7.0, epsabs=1e-14, epsrel=0.0)[0] - np.sqrt(np.pi) / 4) <= 1e-13  # and s: the same area


def test_s_is_the_derivative_to_ln_zeta():
    """s = -u dK/du (K depends on zeta through u = |dv| / zeta alone, so dK / d ln zeta = -u dK/du) against mpmath.diff"""
    mpmath.mp.dps = 40
    for x in (0.05, 0.3, 1.0, 2.2, 4.0, 5.9):
        exact = -mpmath.mpf(x) * mpmath.diff(mp_K, mpmath.mpf(x))
        got = float(mref.profile(x)[1])
        print(f"u = {x}: s = {got!r}, -u dK/du = {float(exact)!r}")
        assert abs(got - float(exact)) <= 1e-15


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
def small_grids():
    rng = np.random.default_rng(3)
    return (("log-uniform", 6560.0 * np.exp(np.arange(700) / 3.0e5)), ("irregular", np.sort(rng.uniform(6560.0, 6575.0, 600))),
            ("two-density", np.r_[np.linspace(6560.0, 6565.0, 60, endpoint=False), np.linspace(6565.0, 6570.0, 500)]))


def test_a_constant_is_preserved_and_its_derivative_is_zero():
    for tag, lam in small_grids():
        for zeta in (0.0, 1.0, 8.0):
            r = mref.macroturbulence(lam, np.full(lam.size, 1.7), zeta, reference=np.full(lam.size, -0.3))
            err = max(float(np.max(np.abs(r["out"] / LD(1.7) - 1))), float(np.max(np.abs(r["out_reference"] / LD(-0.3) - 1))))
            assert err <= 3e-16 and float(np.max(np.abs(r["dout"]))) <= 1e-15, (tag, zeta, err)


def test_dout_against_difference_quotients_in_ln_zeta():
    """the restatement's dout against Richardson-extrapolated central differences of its own forward at zeta exp(+-h): the quotients'
    truncation error is O(h^4) after extrapolation and is allowed what the two quotients differ by, an O(h^2) quantity; their rounding
    error is that of the fp64 K, 3e-16 of the peak, over h; points whose windows change with zeta gain or lose 3e-18 of the peak"""
    rng = np.random.default_rng(9)
    for tag, lam in small_grids():
        f = 1.0 + 0.3 * rng.standard_normal(lam.size)
        for zeta in (1.0, 8.0):
            r = mref.macroturbulence(lam, f, zeta)
            q = {}
            for h in (0.02, 0.01):
                q[h] = (mref.macroturbulence(lam, f, zeta * np.exp(h))["out"] - mref.macroturbulence(lam, f, zeta * np.exp(-h))["out"]) / (2 * h)
            rich = (4 * q[0.01] - q[0.02]) / 3
            allow = np.abs(q[0.02] - q[0.01]) + 1e-15 * r["scale"] / 0.01  # (the quotients' own disagreement; the fp64 K's 3e-16 over h)
            err = np.abs(r["dout"] - rich)
            print(f"{tag}, zeta = {zeta}: worst |dout - Richardson| / allowance {float(np.max(err / allow)):.3e}, largest |dout| {float(np.max(np.abs(r['dout']))):.3e}")
            assert np.all(err <= allow) and np.any(np.abs(r["dout"]) > 10 * allow)


def test_the_adjoint_is_the_transpose():
    rng = np.random.default_rng(4)
    for tag, lam in small_grids():
        f, g, u, u_ref = (rng.standard_normal(lam.size) for _ in range(4))
        nus = K.C_CGS * 1.0e8 / lam
        for zeta in (0.0, 1.0, 8.0):
            rows = list(mref.point_rows(lam, zeta)) if zeta > 0 else None
            r = mref.macroturbulence(lam, f, zeta, reference=g, rows=rows)
            w, w_ref, scale, _ = mref.adjoint(lam, u, zeta, u_reference=u_ref, rows=rows)
            terms = mref.dot_terms(lam, u, f, zeta, rows=rows)
            lhs, rhs = float(np.sum(r["out"] * u)), float(np.sum(w * f))
            print(f"{tag}, zeta = {zeta}: <M f, u> = {lhs:.15e}, <f, M^T u> = {rhs:.15e}, terms {terms:.3e}")
            assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms
            assert abs(float(np.sum(r["out_reference"] * u_ref) - np.sum(w_ref * g))) <= SUM_TOL * mref.dot_terms(lam, u_ref, g, zeta, rows=rows)
            assert np.all(scale > 0)  # every point is in a window: its own
            with_nus = mref.adjoint(lam, u, zeta, nus=nus, rows=rows)[0]  # weights over F_nu: F_lambda = F_nu nu / lambda
            assert abs(float(np.sum(with_nus * (f * lam / nus))) - lhs) <= SUM_TOL * terms


# ---- the GPU file's inputs -----------------------------------------------------------------------------------------------------
def test_window_lengths_and_mapping_estimates_on_the_sc2_grid():
    assert LAM.size == 7634
    interior = slice(1000, -1000)
    lengths = {zeta: int(mref.window_lengths(LAM, zeta)[interior].max()) for zeta in (0.05, 0.3, 1.5, 1.6, 1.62, 3.2, 35.0)}
    print(lengths)
    assert lengths == {0.05: 1, 0.3: 7, 1.5: 31, 1.6: 33, 1.62: 33, 3.2: 65, 35.0: 701}
    for zeta in lengths:
        n = mref.window_lengths(LAM, zeta)[interior]
        assert n.min() >= n.max() - 1, zeta  # log-uniform: one length, give or take a point at a rounding
    e = {zeta: mref.mapping_estimate(LAM, zeta) for zeta in (1.5, 1.6, 1.62)}
    print({zeta: (float(v.min()), float(v.max())) for zeta, v in e.items()})
    assert e[1.5].max() <= 30.3  # eight lanes per point everywhere
    assert (round(float(e[1.6].min()), 2), round(float(e[1.6].max()), 2)) == (31.78, 32.27) and e[1.6].min() <= 32 < e[1.6].max()  # both mappings in one launch
    assert round(float(e[1.62].min()), 2) >= 32.18 and 32 < e[1.62].min() < 33  # a wave per point, just past the switch
    assert MACRO_TOL == 1e-12


def test_difference_quotient_steps_of_the_gpu_test():
    """tests/test_gpu_macroturbulence.py holds the device's dout against Richardson-extrapolated quotients of the device's forward at
    zeta (1 +- h) and allows |coarse - fine| + MACRO_TOL max |F| / h.  Where the first term cancels the second must cover the O(h^4)
    remainder: at h = 0.008 and 0.004 the restatement's own remainder stays below it at every point of the S-c2 grid"""
    f = 1.0 + 0.1 * np.random.default_rng(11).standard_normal(LAM.size)  # (the GPU file's flux)
    coarse_h, fine_h = 0.008, 0.004
    for zeta in (1.6, 3.2):
        q = [(mref.macroturbulence(LAM, f, zeta * (1 + h))["out"] - mref.macroturbulence(LAM, f, zeta * (1 - h))["out"]) / (2 * h) for h in (coarse_h, fine_h)]
        remainder = float(np.max(np.abs(mref.macroturbulence(LAM, f, zeta)["dout"] - (4 * q[1] - q[0]) / 3)))
        room = MACRO_TOL * np.abs(f).max() / coarse_h
        print(f"zeta = {zeta}: the Richardson value's remainder {remainder:.3e} against MACRO_TOL max |F| / h = {room:.3e}")
        assert remainder < room


def test_edge_affected_uses_the_combined_reach():
    from stardis_amd.instrument import Instrument, doppler_factor

    class Host(Instrument):  # the mask is plain numpy: an instrument without a device
        def __init__(self, edges, sigma, v_rot, v_mac, v_rad):
            self.edges, self.sigma = np.asarray(edges, dtype=np.float64), np.broadcast_to(np.float64(sigma), (len(edges) - 1,))
            self.v_rot, self.v_mac, self.doppler = v_rot, v_mac, doppler_factor(v_rad)

    edges = np.linspace(6498.0, 6602.0, 400)
    for v_rot, v_mac, v_rad in ((None, 4.0, 0.0), (40.0, 4.0, 25.0), (10.0, 0.0, 0.0), (None, None, 3.0), (100.0, 35.0, -200.0)):
        got = Host(edges, 0.05, v_rot, v_mac, v_rad).edge_affected(LAM)
        beta = ((v_rot or 0.0) + 6.0 * (v_mac or 0.0)) / K.C_KMS
        D = doppler_factor(v_rad)
        expect = ((edges[:-1] - 0.4) / D * (1 - beta) < LAM[0]) | ((edges[1:] + 0.4) / D * (1 + beta) > LAM[-1])
        assert np.array_equal(got, expect) and got.any() and not got.all()
        # no unflagged pixel sees a point whose macroturbulence window is truncated, or that sees a point whose rotation window is
        b_mac, b_rot = 6.0 * (v_mac or 0.0) / K.C_KMS, (v_rot or 0.0) / K.C_KMS
        rot_cut = (LAM * (1 - b_rot) < LAM[0]) | (LAM * (1 + b_rot) > LAM[-1])
        lo, hi = np.searchsorted(LAM, LAM * (1 - b_mac), "left"), np.searchsorted(LAM, LAM * (1 + b_mac), "right")
        cut = (LAM * (1 - b_mac) < LAM[0]) | (LAM * (1 + b_mac) > LAM[-1]) | np.array([rot_cut[a:b].any() for a, b in zip(lo, hi)])
        x = LAM * D
        for j in np.flatnonzero(~got):
            assert not np.any(cut & (x >= edges[j] - 0.4) & (x <= edges[j + 1] + 0.4)), j
        if v_mac:
            assert got.sum() > Host(edges, 0.05, v_rot, None, v_rad).edge_affected(LAM).sum()
