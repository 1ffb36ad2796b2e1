"""Rotational broadening at build time and on the host: the four entry points are declared, exported and mirrored; the three kernels
compile for gfx950 without spilled vector registers; validation raises before any device is asked for; the properties of the
longdouble restatement (tests/rotation_reference.py) that pin the definition the device is held against; every grid / V pair of
tests/test_gpu_rotation.py keeps clear of the profile's square-root edge; and Instrument.edge_affected against a loop."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.integrate import quad

import rotation_reference as rref
from conftest import ROOT
from rotation_reference import LD, SUM_TOL
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib, synth
from stardis_amd import constants as K

ENTRIES = {"sdx_rotate_dev": 8, "sdx_rotate_f64": 9, "sdx_rotate_adjoint_dev": 9, "sdx_rotate_adjoint_f64": 10}

# the grids of tests/test_gpu_rotation.py
LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform
IRREGULAR = np.sort(np.random.default_rng(7).uniform(6500.0, 6600.0, 3000))
TWO_DENSITY = np.r_[np.linspace(6500.0, 6550.0, 500, endpoint=False), np.linspace(6550.0, 6600.0, 4000)]
GPU_CASES = [("S-c2", LAM, V) for V in (0.2, 2.0, 9.0, 9.6, 9.7, 19.3, 211.0)] + [(tag, lam, V) for tag, lam in (("irregular", IRREGULAR), ("two-density", TWO_DENSITY))
                                                                             for V in (23.7, 100.0)]


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
    # V and eps by value in the host-buffer twins; the device entries read the pair from device memory
    assert _lib.PROTOTYPES["sdx_rotate_f64"][1][5:7] == [ctypes.c_double] * 2 and _lib.PROTOTYPES["sdx_rotate_adjoint_f64"][1][3:5] == [ctypes.c_double] * 2
    assert _lib.PROTOTYPES["sdx_rotate_dev"][1][5] is ctypes.c_void_p and _lib.PROTOTYPES["sdx_rotate_adjoint_dev"][1][3] is ctypes.c_void_p


def test_rotation_kernels_do_not_spill(resources):  # noqa: F811
    """the figures DESIGN.md quotes: 52, 48 and 44 vector registers, eight waves per SIMD, no LDS"""
    for name, vgpr in (("k_rotate", 52), ("k_rotate_adjoint_den", 48), ("k_rotate_adjoint", 44)):
        found = [v for k, v in resources.items() if k == name]
        assert len(found) == 1, sorted(resources)
        print(name, found[0])
        assert found[0]["spill"] == 0 and found[0]["lds"] == 0 and found[0]["occ"] == 8 and found[0]["vgpr"] <= vgpr, (name, found[0])


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_rotate_dev(None, 4, None, None, None, None, None, None) == -1
    assert b"rotate" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_rotate_f64(None, 4, None, None, None, 10.0, 0.6, None, None) == -1
    assert lib.sdx_rotate_adjoint_dev(None, 4, None, None, None, None, None, None, None) == -1
    assert b"rotate_adjoint" in lib.sdx_last_error_string()
    assert lib.sdx_rotate_adjoint_f64(None, 4, None, 10.0, 0.6, None, None, None, None, None) == -1


def test_validation_needs_no_device():
    from stardis_amd import ops
    from stardis_amd.instrument import Instrument, rotation_pair

    edges = np.linspace(6560.0, 6570.0, 11)
    assert rotation_pair(0.0) == (0.0, 0.6) and rotation_pair(12.5, 1.0) == (12.5, 1.0) and rotation_pair(2999.0, 0.0) == (2999.0, 0.0)
    for bad in (dict(v_rot=-1.0), dict(v_rot=np.nan), dict(v_rot=np.inf), dict(v_rot=3000.0), dict(v_rot=10.0, limb_darkening=-0.1),
                dict(v_rot=10.0, limb_darkening=1.5), dict(v_rot=10.0, limb_darkening=np.nan), dict(v_rot="fast")):
        with pytest.raises(ValueError):
            rotation_pair(**bad)
        with pytest.raises(ValueError):
            Instrument(edges, resolving_power=5e4, **bad)
    lam = np.linspace(6560.0, 6570.0, 50)
    for call in (lambda: ops.rotate(lam, np.ones(50), -3.0), lambda: ops.rotate(lam[::-1], np.ones(50), 10.0), lambda: ops.rotate(lam, np.ones(49), 10.0),
                 lambda: ops.rotate(lam, np.ones(50), 10.0, reference=np.ones(3)), lambda: ops.rotate(lam[:1], np.ones(1), 10.0),
                 lambda: ops.observe(lam, np.ones(50), edges, 0.05, v_rot=-1.0), lambda: ops.observe_adjoint(lam, np.ones(10), edges, 0.05, v_rot=5000.0)):
        with pytest.raises(ValueError):
            call()
    if _lib.load().sdx_device_count() == 0:  # valid arguments: then, and only then, the device is asked for (no CPU fallback)
        with pytest.raises(RuntimeError):
            ops.rotate(lam, np.ones(50), 10.0)


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
def small_grids():
    rng = np.random.default_rng(3)
    return (("log-uniform", 6560.0 * np.exp(np.arange(700) / 3.0e5)), ("irregular", np.sort(rng.uniform(6560.0, 6575.0, 600))),
            ("two-density", np.r_[np.linspace(6560.0, 6565.0, 60, endpoint=False), np.linspace(6565.0, 6570.0, 500)]))


def test_a_constant_is_preserved():
    for tag, lam in small_grids():
        for V in (0.0, 3.0, 40.0):
            for eps in (0.0, 0.6, 1.0):
                out, out_ref, _, _ = rref.rotate(lam, np.full(lam.size, 1.7), V, eps, reference=np.full(lam.size, -0.3))
                err = max(float(np.max(np.abs(out / LD(1.7) - 1))), float(np.max(np.abs(out_ref / LD(-0.3) - 1))))
                assert err <= 3e-16, (tag, V, eps, err)


def test_the_adjoint_is_the_transpose():
    rng = np.random.default_rng(4)
    for tag, lam in small_grids():
        f, g, u, u_ref = (rng.standard_normal(lam.size) for _ in range(4))
        nus = K.C_CGS * 1.0e8 / lam
        for V, eps in ((0.0, 0.6), (3.0, 0.0), (40.0, 0.6), (40.0, 1.0)):
            out, out_ref, _, _ = rref.rotate(lam, f, V, eps, reference=g)
            w, w_ref, scale, _ = rref.adjoint(lam, u, V, eps, u_reference=u_ref)
            terms = rref.dot_terms(lam, u, f, V, eps)
            lhs, rhs = float(np.sum(out * u)), float(np.sum(w * f))
            print(f"{tag}, V = {V}, eps = {eps}: <rotate(f), u> = {lhs:.15e}, <f, adjoint(u)> = {rhs:.15e}, terms {terms:.3e}")
            assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms
            assert abs(float(np.sum(out_ref * u_ref) - np.sum(w_ref * g))) <= SUM_TOL * rref.dot_terms(lam, u_ref, g, V, eps)
            assert np.all(scale > 0)  # every point is in a window: its own
            with_nus = rref.adjoint(lam, u, V, eps, nus=nus)[0]  # weights over F_nu: F_lambda = F_nu nu / lambda
            assert abs(float(np.sum(with_nus * (f * lam / nus))) - lhs) <= SUM_TOL * terms


def gray_convolution(lam_i, V, eps, F):
    """the continuous operator at lam_i: integral F(lam_i (1 + y beta)) K(y) dy / integral K(y) dy over -1 <= y <= 1"""
    beta = V / rref.C_KMS
    kern = lambda y: 2 * (1 - eps) * np.sqrt(1 - y * y) + np.pi / 2 * eps * (1 - y * y)  # noqa: E731
    num = quad(lambda y: F(lam_i * (1 + y * beta)) * kern(y), -1, 1, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
    return num / ((1 - eps) * np.pi + np.pi / 2 * eps * 4 / 3)


def test_converges_to_the_continuous_convolution():
    """a Gaussian absorption line on log-uniform grids of R and 2R against the continuous Gray convolution: the trapezoid rule at a
    square-root edge is O(h^1.5), so the error falls by at least 2"""
    V, eps, centre, width = 30.0, 0.6, 6565.0, 0.08
    F = lambda x: 1.0 - 0.6 * np.exp(-0.5 * ((x - centre) / width) ** 2)  # noqa: E731
    errs = []
    for R in (2.0e5, 4.0e5):
        lam = 6555.0 * np.exp(np.arange(int(np.log(6575.0 / 6555.0) * R) + 1) / R)
        out = rref.rotate(lam, F(lam), V, eps)[0]
        at = np.flatnonzero(np.abs(lam - centre) < 1.2)[::7]
        exact = np.array([gray_convolution(lam[i], V, eps, F) for i in at])
        errs.append(float(np.max(np.abs(out[at].astype(np.float64) - exact))))
        print(f"R = {R:.0e}: {rref.window_lengths(lam, V)[at].max()} points per window, worst error over {at.size} points {errs[-1]:.3e}")
    assert errs[1] > 1e-12 and errs[0] / errs[1] >= 2.0


# ---- the GPU file's inputs -----------------------------------------------------------------------------------------------------
def test_gpu_cases_keep_clear_of_the_profile_edge():
    worst = np.inf
    for tag, lam, V in GPU_CASES:
        margin = rref.profile_edge_margin(lam, V)
        print(f"{tag}, V = {V}: windows of {rref.window_lengths(lam, V).min()} .. {rref.window_lengths(lam, V).max()} points, margin {margin:.2e}")
        assert margin >= 1e-8, (tag, V, margin)
        worst = min(worst, margin)
    assert worst >= 1e-8
    n = rref.window_lengths(LAM, 0.2)
    assert n.max() == 1
    assert rref.window_lengths(LAM, 9.0).max() <= 32 < rref.window_lengths(LAM, 9.7).max() and rref.window_lengths(LAM, 19.3).max() > 64


def test_edge_affected_against_a_loop():
    from stardis_amd.instrument import Instrument, doppler_factor

    class Host(Instrument):  # the mask is plain numpy: an instrument without a device
        def __init__(self, edges, sigma, v_rot, v_rad):
            self.edges, self.sigma = np.asarray(edges, dtype=np.float64), np.broadcast_to(np.float64(sigma), (len(edges) - 1,))
            self.v_rot, self.doppler = v_rot, doppler_factor(v_rad)

    lam = LAM
    edges = np.linspace(6498.0, 6602.0, 400)
    for v_rot, v_rad in ((None, 0.0), (0.0, 0.0), (10.0, 0.0), (100.0, 30.0), (100.0, -200.0), (300.0, 12.0)):
        inst = Host(edges, 0.05, v_rot, v_rad)
        got = inst.edge_affected(lam)
        beta = (v_rot or 0.0) / K.C_KMS
        expect = np.zeros(edges.size - 1, dtype=bool)
        reach_lo, reach_hi = lam[0] / (1 - beta), lam[-1] / (1 + beta)  # a point below / above this has a truncated window
        for j in range(edges.size - 1):
            lo, hi = (edges[j] - 8 * 0.05) / inst.doppler, (edges[j + 1] + 8 * 0.05) / inst.doppler
            expect[j] = lo < reach_lo or hi > reach_hi
        differ = got != expect
        # (the two spellings round differently: they may differ where an end sits within rounding of the threshold, and nowhere else)
        assert not differ.any(), (v_rot, v_rad, np.flatnonzero(differ))
        assert got.any() and not got.all()
        # no unflagged pixel sees a point whose rotation window is truncated
        x = lam * inst.doppler
        truncated = (lam * (1 - beta) < lam[0]) | (lam * (1 + beta) > lam[-1])
        for j in np.flatnonzero(~got):
            seen = (x >= edges[j] - 8 * 0.05) & (x <= edges[j + 1] + 8 * 0.05)
            assert not np.any(truncated & seen), j
        if v_rot:
            assert got.sum() > Host(edges, 0.05, None, v_rad).edge_affected(lam).sum()
