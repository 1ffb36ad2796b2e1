"""Continuum scattering without a GPU: the mean weights conserve photons, the restatement of the definition
(tests/scattering_reference.py) has the limits the definition promises — J = S deep inside a uniform medium, the two-stream surface
value sqrt(epsilon) at second order in the grid spacing —, the entry points are declared, exported and mirrored, and the Python-side
validation raises before any device is asked for."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import scattering_reference as R
from conftest import ROOT

from stardis_amd import _lib, ops, synth

ENTRIES = {"sdx_mean_intensity_dev": 16, "sdx_scatter_source_dev": 23, "sdx_mean_intensity_f64": 12, "sdx_scatter_source_f64": 19}


# ---- the definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_theta", [1, 3, 7, 20, 64])
def test_mean_weights_sum_to_one_half(n_theta):
    thetas, w = synth.thetas_and_weights(n_theta)
    m = ops.mean_weights(thetas, w)
    assert m.shape == (n_theta,) and (m > 0).all()
    total = math.fsum(2.0 * m)  # (doubling is exact, fsum is the exact sum rounded once)
    print(n_theta, (total - 1.0) / np.finfo(np.float64).eps, "ulp")
    assert abs(total - 1.0) <= 2 * np.finfo(np.float64).eps
    assert np.allclose(m, R.mean_weights(thetas, w), rtol=1e-15, atol=0)  # the restatement's plain sum: the same weights


@pytest.mark.parametrize("n_theta", [1, 3, 20])
def test_constant_source_in_an_opaque_medium_is_its_own_mean_intensity(n_theta):
    thetas, w = synth.thetas_and_weights(n_theta)
    m = ops.mean_weights(thetas, w)
    rng = np.random.default_rng(n_theta)
    n_depth = 9
    dist = rng.uniform(0.5e6, 2e6, n_depth - 1)
    ray = dist.reshape(-1, 1) / np.cos(thetas)
    alphas = 10.0 ** rng.uniform(-3.5, 0.0, (n_depth, 6))  # every vertical gap >= 100 * 1e6 * 1e-3.5 * 0.5 ... : checked below
    assert R.optical_depths(alphas, ray, np.float64).min() >= 100.0
    S = np.full((n_depth, 6), 3.25)
    J, _ = R.mean_intensity(alphas, ray, m, S, np.float64)
    assert np.abs(J[1:-1] / S[1:-1] - 1.0).max() <= 1e-15
    assert np.abs(J[0] / S[0] - 1.0).max() <= 1e-15  # the thermalised lower boundary: U = S there, D has arrived at S
    assert np.abs(J[-1] / S[-1] - 0.5).max() <= 1e-15  # the surface sees one hemisphere


def _two_stream_surface(n_points):
    mu, eps = 1.0 / math.sqrt(3.0), 0.01
    tau = np.linspace(60.0, 0.0, n_points)  # row 0 deepest
    dtau = tau[:-1] - tau[1:]
    ray = dtau.reshape(-1, 1) / mu
    op = R.operator(np.ones((n_points, 1)), ray, np.array([0.5]), np.float64)
    w = np.full((n_points, 1), 1.0 - eps)
    S = R.direct_solve(op, w, np.ones((n_points, 1)))
    return float(S[-1, 0]), math.sqrt(eps)


def test_two_stream_surface_value_converges_at_second_order():
    """one angle mu = 1 / sqrt(3), m = 1/2, B = 1, epsilon = 0.01: the Eddington two-stream problem, whose surface source function is
    sqrt(epsilon).  Prototype errors over 101 / 201 / 401 / 801 points: 7.0e-3, 1.9e-3, 4.9e-4, 1.2e-4."""
    errors = []
    for n in (101, 201, 401, 801):
        got, exact = _two_stream_surface(n)
        errors.append(abs(got - exact))
        print(n, got, exact, errors[-1])
    assert errors[0] < 1e-2
    for coarse, fine in zip(errors, errors[1:]):
        assert coarse / fine >= 3.5, errors


def test_iteration_reaches_the_direct_solution():
    """the restatement's iteration against its own dense solve, in extended precision where the host has it: 57 points over 7 decades"""
    dt = R.L if R.EXTENDED else np.float64
    thetas, wts = synth.thetas_and_weights(3)
    _, dtau = R.log_grid(57, 1e-4, 1e3)
    op = R.operator(np.ones((57, 3)), dtau.reshape(-1, 1) / np.cos(thetas), R.mean_weights(thetas, wts), dt)
    Ld = op.diagonal()
    assert Ld.min() > 0 and Ld.max() < 1
    w = np.broadcast_to(np.array([0.5, 0.9, 0.99]), (57, 3)).astype(dt)
    r = R.iterate(op, w, np.ones((57, 3)), tol=1e-12, max_iter=2000)
    assert (r["status"] == 0).all() and list(r["iterations"]) == [23, 75, 236]
    assert np.abs(r["S"] - R.direct_solve(op, w, np.ones((57, 3)))).max() <= 2e-11


def test_coarse_grid_has_no_contraction():
    """3 points over [0.1, 10], one angle, albedo 0.999: the diagonal leaves [0, 1] and the iteration's spectral radius is far above 1"""
    thetas, wts = synth.thetas_and_weights(1)
    _, dtau = R.log_grid(3, 0.1, 10.0)
    op = R.operator(np.ones((3, 1)), dtau.reshape(-1, 1) / np.cos(thetas), R.mean_weights(thetas, wts), np.float64)
    assert op.diagonal().max() > 1.0
    assert R.spectral_radius(op, np.full((3, 1), 0.999))[0] > 5.0
    r = R.iterate(op, np.full((3, 1), 0.999), np.ones((3, 1)), tol=1e-12, max_iter=2000)
    assert r["status"][0] != 0


# ---- the build -------------------------------------------------------------------------------------------------------------------
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
        declared = [("int64_t" in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ("double" in a and ctypes.c_double) or ctypes.c_int
                    for a in m.group(1).split(",")]
        assert declared == list(args), name


def test_null_context_and_bad_loop_arguments_are_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_mean_intensity_dev(None, 4, 1, 1, None, None, None, None, None, 1, None, 0, None, 0, None, 0) == -1
    assert b"mean_intensity" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_scatter_source_dev(None, 4, 1, 1, None, None, None, None, None, 1, None, 0, None, 0, 1e-12, 10, None, 0, None, 0, None, None, None) == -1
    assert b"scatter_source" in lib.sdx_last_error_string()
    assert lib.sdx_mean_intensity_f64(None, 4, 1, 1, None, None, None, None, None, None, None, None) == -1
    assert lib.sdx_scatter_source_f64(None, 4, 1, 1, None, None, None, None, None, None, 0, None, 1e-12, 10, None, None, None, None, None) == -1


# ---- validation on the host ------------------------------------------------------------------------------------------------------
class NoDevice:
    """a context that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_validation_needs_no_device():
    from stardis_amd.engine import SpectralSynthesizer
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    # a spherical model
    for fn in (rfs.mean_intensity, rfs.scattering_source):
        with pytest.raises(NotImplementedError, match="plane-parallel"):
            fn(types.SimpleNamespace(spherical=True), None)
    # wrong shapes, too many angles, a bad loop
    nus, temps, m = np.linspace(7e14, 4e14, 5), np.linspace(4000.0, 9000.0, 4), np.array([0.25, 0.25])
    ray, alphas = np.ones((3, 2)), np.ones((4, 5))
    base = dict(tracing_nus=nus, temperatures=temps, ray_distances=ray, mean_weights=m, total_alphas=alphas, ctx=NoDevice())
    for kw in (dict(ray_distances=np.ones((3, 3))), dict(ray_distances=np.ones((2, 2))), dict(total_alphas=np.ones((4, 4))),
               dict(total_alphas=np.ones((5, 4))), dict(source=np.ones((4, 6))), dict(want_J=False, want_L=False),
               dict(mean_weights=np.full(65, 1 / 130), ray_distances=np.ones((3, 65)))):
        with pytest.raises(ValueError):
            ops.mean_intensity(**dict(base, **kw))
    base["alpha_scatter"] = np.ones(4)
    for kw in (dict(ray_distances=np.ones((3, 3))), dict(total_alphas=np.ones((4, 4))), dict(thermal=np.ones((4, 6))), dict(alpha_scatter=np.ones(5)),
               dict(alpha_scatter=np.ones((4, 4))), dict(alpha_scatter=np.ones((5, 4))), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=0),
               dict(mean_weights=np.full(65, 1 / 130), ray_distances=np.ones((3, 65)))):
        with pytest.raises(ValueError):
            ops.scatter_source(**dict(base, **kw))
    with pytest.raises(ValueError):
        ops.mean_weights(np.ones(3), np.ones(4))
    # the synthesizer's option: checked before anything is uploaded; keep_total stays on under it; results refused when it is off
    for bad in (dict(tol=-1.0), dict(max_iter=0), dict(relaxation=1.0)):
        with pytest.raises(ValueError, match="scattering"):
            SpectralSynthesizer._scattering_options(bad, continuum={})
    with pytest.raises(ValueError, match="continuum"):
        SpectralSynthesizer._scattering_options(True, continuum=None)
    assert SpectralSynthesizer._scattering_options(None, None) is None and SpectralSynthesizer._scattering_options(False, None) is None
    assert SpectralSynthesizer._scattering_options(dict(max_iter=7), {}) == dict(tol=1e-12, max_iter=7)
    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.keep_contribution, syn.keep_response, syn._keep_total, syn.d_total = NoDevice(), False, False, True, object()
    assert syn.scattering is None
    for ask in (lambda: syn.scattering_source, lambda: syn.scattering_mean_intensity, lambda: syn.scattering_flux, lambda: syn.scattering_iterations,
                lambda: syn.scattering_status):
        with pytest.raises(RuntimeError, match="scattering=True"):
            ask()
    syn.scattering = dict(tol=1e-12, max_iter=2000)
    with pytest.raises(ValueError, match="scattering"):
        syn.keep_total = False
    assert syn.keep_total is True
