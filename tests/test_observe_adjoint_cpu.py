"""No-GPU checks of the instrument adjoint (sdx_observe_adjoint_dev): the numpy restatement tests/observe_adjoint_reference.py pinned by
its own properties — the dot identity with the forward restatement in both modes, the reference cotangent against a central difference,
uncovered pixels ignored, exact zeros outside every window, and the bracket by prefix maximum / suffix minimum that the device's gather
searches — then the ABI surface, the Python argument errors, and the new kernels' register figures."""
import inspect
import os
import re

import numpy as np
import pytest

import observe_adjoint_reference as aref
import observe_reference as oref
from conftest import ROOT
from observe_reference import SUM_TOL
from stardis_amd import _lib, ops
from stardis_amd.instrument import Instrument, adjoint_host_arguments
from test_kernel_resources_cpu import resources  # noqa: F401  (the module fixture: one `make resources` for both files)

HEADER = os.path.join(ROOT, "include", "stardis_hip.h")


def constant_R_input():
    """1500 points on 6500 - 6600 A, 60 pixels over 6499 - 6601 A at R = 20000: the outermost pixels are not covered"""
    lam = np.linspace(6500.0, 6600.0, 1500)
    edges = np.linspace(6499.0, 6601.0, 61)
    return lam, edges, oref.sigma_of_R(edges, 2.0e4), -30.0


INPUTS = {"non-monotone sigma": aref.nonmonotone_input, "constant R": constant_R_input}


def spectra(lam, n_pix, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n_pix), 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0)


def test_the_nonmonotone_input_is_what_it_claims():
    lam, edges, sigma, v = aref.nonmonotone_input()
    lo, hi = edges[:-1] - 8 * sigma, edges[1:] + 8 * sigma
    member = aref.pixel_sets(lam, edges, sigma, oref.doppler_factor(v))
    gaps, outside = aref.noncontiguous_points(member), int((~member.any(axis=0)).sum())
    print(f"lo ascends: {bool(np.all(np.diff(lo) >= 0))}, hi ascends: {bool(np.all(np.diff(hi) >= 0))}, points with a gap in their pixel set: {gaps}, in no window: {outside}")
    assert np.any(np.diff(lo) < 0) and np.any(np.diff(hi) < 0)
    assert gaps >= 1 and outside >= 1 and member.any(axis=1).sum() >= 30


@pytest.mark.parametrize("name", INPUTS)
def test_bracket_holds_every_member(name):
    """the candidates [jA, jB) of a point — jA the first j with PH_j >= x, jB one past the last with SL_j <= x — hold its whole pixel set"""
    lam, edges, sigma, v = INPUTS[name]()
    x = lam * oref.doppler_factor(v)
    lo, hi = edges[:-1] - 8 * sigma, edges[1:] + 8 * sigma
    PH, SL = np.maximum.accumulate(hi), np.minimum.accumulate(lo[::-1])[::-1]
    assert np.all(np.diff(PH) >= 0) and np.all(np.diff(SL) >= 0)
    jA, jB = np.searchsorted(PH, x, "left"), np.searchsorted(SL, x, "right")
    member = aref.pixel_sets(lam, edges, sigma, oref.doppler_factor(v))
    inside = (np.arange(sigma.size)[:, None] >= jA[None, :]) & (np.arange(sigma.size)[:, None] < jB[None, :])
    assert np.all(inside[member])
    # the forward's own predicate on the candidates gives the set back exactly
    covered = (lo >= x[0]) & (hi <= x[-1])
    predicate = covered[:, None] & (lo[:, None] <= x[None, :]) & (x[None, :] <= hi[:, None])
    assert np.array_equal(predicate & inside, member)


@pytest.mark.parametrize("name", INPUTS)
def test_dot_identity_in_both_modes(name):
    lam, edges, sigma, v = INPUTS[name]()
    D = oref.doppler_factor(v)
    c, f, g = spectra(lam, sigma.size)
    for tag, ref in (("plain", None), ("with a reference", g)):
        out = oref.observe(lam, f, edges, sigma, D, reference=ref)
        ok = ~np.isnan(out)
        w_flux = aref.adjoint(lam, c, edges, sigma, D, flux=f, reference=ref)[0]
        lhs, rhs, terms = float(np.sum(c[ok] * out[ok])), float(w_flux @ f), aref.dot_terms(lam, c, f, edges, sigma, D, reference=ref)
        print(f"{name}, {tag}: <c, observe(f)> = {lhs:.15e}, <adjoint(c), f> = {rhs:.15e}, difference / sum of |terms| = {abs(lhs - rhs) / terms:.2e}")
        assert 0 < ok.sum() and abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms
    # with nus the weights are those of F_nu = F_lambda lambda / nu
    nus = 2.99792458e18 / lam
    w_nu = aref.adjoint(lam, c, edges, sigma, D, nus=nus)[0]
    out = oref.observe(lam, f, edges, sigma, D)
    ok = ~np.isnan(out)
    assert abs(float(np.sum(c[ok] * out[ok])) - float(w_nu @ (f * lam / nus))) <= SUM_TOL * aref.dot_terms(lam, c, f, edges, sigma, D)


@pytest.mark.parametrize("name", INPUTS)
def test_reference_cotangent_against_a_central_difference(name):
    """per pixel out(g_i + d) = num / (den + w d), so the central difference is the derivative times 1 / (1 - (w d / den)^2); each
    observed value carries a few 1e-16 of itself from the sums (all terms positive): 1e-15 |out_j| / d per pixel of the point"""
    lam, edges, sigma, v = INPUTS[name]()
    D = oref.doppler_factor(v)
    c, f, g = spectra(lam, sigma.size)
    _, w_ref, _, scale_ref = aref.adjoint(lam, c, edges, sigma, D, flux=f, reference=g)
    out = oref.observe(lam, f, edges, sigma, D, reference=g)
    member = aref.pixel_sets(lam, edges, sigma, D)
    d = 1.0e-3
    points = np.argsort(-np.abs(w_ref))[:: max(1, lam.size // 12)][:12]
    seen = False
    for i in points:
        up, dn = g.copy(), g.copy()
        up[i] += d
        dn[i] -= d
        ok = member[:, i]
        diff = (oref.observe(lam, f, edges, sigma, D, reference=up)[ok] - oref.observe(lam, f, edges, sigma, D, reference=dn)[ok]) / (2 * d)
        value = float(np.sum(c[ok] * diff))
        allow = 1.0e-15 / d * float(np.sum(np.abs(c[ok] * out[ok]))) + 2.0 * (d / g.min()) ** 2 * scale_ref[i]  # (w / den <= 1 / min g)
        print(f"{name}, point {i}: w_ref {w_ref[i]:+.6e}, central difference {value:+.6e}, allowance {allow:.1e}")
        assert abs(value - w_ref[i]) <= allow
        seen |= abs(w_ref[i]) > 10 * allow
    assert seen


@pytest.mark.parametrize("name", INPUTS)
def test_uncovered_pixels_are_ignored_and_points_outside_are_zero(name):
    lam, edges, sigma, v = INPUTS[name]()
    D = oref.doppler_factor(v)
    c, f, g = spectra(lam, sigma.size)
    member = aref.pixel_sets(lam, edges, sigma, D)
    uncovered = ~member.any(axis=1)
    if name == "constant R":
        assert uncovered.sum() >= 2
    poisoned = np.where(uncovered, np.nan, c)
    for ref in (None, g):
        clean = aref.adjoint(lam, np.where(uncovered, 0.0, c), edges, sigma, D, flux=f, reference=ref)
        dirty = aref.adjoint(lam, poisoned, edges, sigma, D, flux=f, reference=ref)
        for a, b in zip(clean[:2], dirty[:2]):
            assert (a is None and b is None) or (np.array_equal(a, b) and np.all(np.isfinite(b)))
        outside = ~member.any(axis=0)
        assert outside.sum() >= 1 and np.all(dirty[0][outside] == 0.0) and np.any(dirty[0][~outside] != 0.0)
        if ref is not None:
            assert np.all(dirty[1][outside] == 0.0)


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_and_prototyped_with_matching_arity():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("sdx_observe_adjoint_dev", "sdx_observe_adjoint_f64"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len(params) == len(argtypes) == 13, (name, params)
        assert [("double" in p and "*" not in p) for p in params] == [a is _lib.C.c_double for a in argtypes]
        assert [("int64_t" in p) for p in params] == [a is _lib.C.c_int64 for a in argtypes]
        assert hasattr(_lib.C.CDLL(_lib.LIB_PATH), name)


def test_python_argument_errors_need_no_device():
    lam = np.linspace(6500.0, 6600.0, 50)
    edges = np.linspace(6520.0, 6580.0, 11)
    ok = np.ones(10)
    for kw, named in ((dict(pixel_weights=np.ones(9)), "pixel_weights"), (dict(flux=np.ones(49), reference=np.ones(50)), "flux"),
                      (dict(flux=np.ones(50), reference=np.ones(51)), "reference"), (dict(nus=np.ones(3)), "nus"),
                      (dict(reference=np.ones(50)), "reference needs the flux"), (dict(lambdas=lam[::-1]), "lambdas"), (dict(lambdas=lam[:1]), "lambdas")):
        args = dict(lambdas=lam, pixel_weights=ok, pixel_edges=edges, sigma=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=named):
            ops.observe_adjoint(**args)
        args.pop("pixel_edges"), args.pop("sigma")
        with pytest.raises(ValueError, match=named):
            adjoint_host_arguments(10, **args)
    for method in (Instrument.adjoint, Instrument.adjoint_host):
        assert "pixel_weights" in inspect.signature(method).parameters
    from stardis_amd.engine import SpectralSynthesizer

    for name in ("pixel_weights_to_grid", "observed_line_sensitivities", "chi2_line_gradient"):
        assert "normalized" in inspect.signature(getattr(SpectralSynthesizer, name)).parameters


# ---- the kernels' registers ----------------------------------------------------------------------------------------------------------
def test_adjoint_kernels_exist_and_do_not_spill(resources):  # noqa: F811
    for k in ("k_observe_adjoint_pixels", "k_observe_adjoint_tiles", "k_observe_adjoint_scan", "k_observe_adjoint", "k_observe"):
        assert k in resources, sorted(r for r in resources if "observe" in r)
        print(k, resources[k])
        assert resources[k]["spill"] == 0
