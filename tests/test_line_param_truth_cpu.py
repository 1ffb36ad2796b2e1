"""The line-profile sensitivities without a GPU: what the restatement of tests/line_param_truth.py rests on, the condition on the models
that lets the sums be judged without leaving a term out, the ABI surface, the Python-side validation and the registers of the new
kernels.

Every figure is printed before it is asserted."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import line_param_truth as T
import oracle
from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: its `make resources` parsing)
from test_response_cpu import NoDevice

from stardis_amd import _lib, ops

ENTRIES = {"sdx_voigt_grad_dev": 9, "sdx_line_param_adjoint_dev": 20, "sdx_line_param_adjoint_f64": 17}
NAMES = ["small", "ragged", "tiny", "odd", "long", "inner"]
INSIDE = 1e-3  # the points of the point-wise tests lie at least this far inside their region


def region_points(n=60, seed=5):
    """-> (x, y) fp64, points of all four regions at least INSIDE away from every region boundary (in s = |x| + y and in y - (0.195 |x| -
    0.176)) and from x = 0 (where |x| has a kink), y > INSIDE (the quotients step in y)"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-30, 30, 4 * n), rng.uniform(-6, 6, 6 * n)])
    y = np.concatenate([10.0 ** rng.uniform(-6, 1.3, 4 * n), 10.0 ** rng.uniform(-8, 0.7, 6 * n)])
    s, edge = np.abs(x) + y, y - (0.195 * np.abs(x) - 0.176)
    keep = (np.abs(s - 15.0) > 10 * INSIDE) & (np.abs(s - 5.5) > 10 * INSIDE) & (np.abs(edge) > 10 * INSIDE) & (np.abs(x) > 10 * INSIDE) & (y > INSIDE)
    x, y = x[keep], y[keep]
    reg = T.region(x, y)
    assert all((reg == r).sum() >= n // 2 for r in (1, 2, 3, 4)), [(r, int((reg == r).sum())) for r in (1, 2, 3, 4)]
    return x, y


def test_derivatives_against_mpmath_diff():
    """the z-derivatives written out in line_param_truth._formulas against mpmath's numerical differentiation of the w formulas"""
    x, y = region_points(n=12)
    reg = T.region(x, y)
    worst = {}
    with mpmath.workdps(T.DPS):
        for xx, yy, r in zip(x, y, reg):
            z = mpmath.mpc(float(xx), float(yy))
            got = T.dw_mp(int(r), z)
            ref = mpmath.diff(lambda v: T.w_mp(int(r), v), z)
            worst[int(r)] = max(worst.get(int(r), 0.0), float(abs(got - ref) / abs(ref)))
    print("written-out w' against mpmath.diff, worst relative difference per region:", worst)
    assert set(worst) == {1, 2, 3, 4} and max(worst.values()) <= 1e-25  # (mpmath.diff at 50 digits: good to ~1e-30)


def test_extended_precision_against_mpmath():
    """the vectorised extended-precision statement (the truth of the sums) against the mpmath statement, and both choose the region
    with the reference's predicates"""
    x, y = region_points()
    reg, w, dw = T.truth_points(x, y)
    w_ld, dw_ld = T.w_dw_ld(x, y)
    for r in (1, 2, 3, 4):
        sel = reg == r
        d_w = float((np.abs(w_ld[sel].astype(np.complex128) - w[sel]) / np.abs(w[sel])).max())
        d_dw = float((np.abs(dw_ld[sel].astype(np.complex128) - dw[sel]) / np.abs(dw[sel])).max())
        print(f"region {r}: {int(sel.sum())} points, extended precision against mpmath: |dw| / |w| {d_w:.2e}, |dw'| / |w'| {d_dw:.2e}")
        assert d_w <= 1e-15 and d_dw <= 1e-15  # (the comparison itself rounds both to fp64: up to 2.2e-16 each)
    # w of the restatement is the reference's function: the oracle's Faddeeva (voigt.py:17-86 in fp64) within its own rounding
    ref = oracle.faddeeva(x + 1j * y)
    worst = float((np.abs(ref - w) / np.abs(w)).max())
    print(f"oracle.faddeeva against the restated w: {worst:.2e} of |w|")
    assert worst <= 1e-12


def test_derivatives_against_difference_quotients_of_the_oracle():
    """K_x and K_y of the restatement against central difference quotients of oracle.voigt_profile (doppler_width = 1: x = delta_nu,
    y = gamma / (sqrt(pi) pi), phi = K / sqrt(pi)), steps h and h / 2 Richardson-extrapolated.  h = 1e-4 keeps every evaluation inside
    the point's region.  Allowed: 1e-9 (|w| + |w'|) — the quotient's rounding is ~4 ulp of phi / h x 3 ~ 1e-11 |w|, its truncation
    h^4 |w^(5)| / 30 ~ 1e-14 |w|; a wrong sign, factor or region is an error of order |w'|."""
    x, y = region_points()
    reg, w, dw = T.truth_points(x, y)
    h = 1e-4
    assert h < INSIDE
    g = y * (T.SQRT_PI * T.PI)

    def quotient(step, dx, dg):
        return (oracle.voigt_profile(x + step * dx, 1.0, g + step * dg) - oracle.voigt_profile(x - step * dx, 1.0, g - step * dg)) / (2 * step)

    kx = (4 * quotient(h / 2, 1, 0) - quotient(h, 1, 0)) / 3 * T.SQRT_PI
    ky = (4 * quotient(h / 2, 0, 1) - quotient(h, 0, 1)) / 3 * T.SQRT_PI * (T.SQRT_PI * T.PI)
    allowed = 1e-9 * (np.abs(w) + np.abs(dw))
    for r in (1, 2, 3, 4):
        sel = reg == r
        ex, ey = np.abs(kx - dw.real)[sel] / allowed[sel], np.abs(ky + dw.imag)[sel] / allowed[sel]
        print(f"region {r}: difference quotients of oracle.voigt_profile against K_x = Re w', K_y = -Im w': worst / allowed {ex.max():.3e}, {ey.max():.3e}; "
              f"largest |w'| {np.abs(dw[sel]).max():.3e}")
        assert ex.max() <= 1.0 and ey.max() <= 1.0
    assert (np.abs(dw) > 100 * allowed).all()  # a zero cannot pass


@pytest.mark.parametrize("name", NAMES)
def test_no_term_of_the_models_lies_on_a_region_boundary(name):
    """the condition that lets the sums be judged without leaving a term out: on every model no evaluation changes its region between
    the reference's x = delta_nu / doppler and the kernels' forms of it, and none lies within 1e-12 of a boundary"""
    m = T.model(name)
    c = oracle.count_region_flips(*T.A.line_args(m))
    print(name, c)
    assert c["evaluations"] > 0 and c["flips_product_form"] == 0 and c["flips_tile_form"] == 0 and c["within_near_of_a_boundary"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement(name):
    """S0 of the restatement is line_adjoint_truth's sum (the reference's own terms) within fp64 rounding; every item has positive
    scales; the Doppler derivative cancels in the Lorentz wing (its scale exceeds its value by orders there); a shard's restatement has
    the shard's terms"""
    m = T.model(name)
    r, a = T.restated(name), T.A.restated(name)
    s0 = np.array([[float((m.W[d, t.col[t.seg[d]:t.seg[d + 1]]] * t.k[t.seg[d]:t.seg[d + 1]]).sum()) for d in range(m.n_depth)] for t in T.terms(name)])
    worst = float((np.abs(s0 - a.s_ld) / T.bound(a.scale_ld, a.terms_ld)).max())
    print(f"{name}: sum W amp K against line_adjoint_truth, worst difference / bound {worst:.3e}")
    assert worst <= 1.0
    for key in ("damping", "doppler", "centre"):
        q = getattr(r, key)
        assert np.array_equal(q.terms_ld, a.terms_ld) and (q.scale_ld > 0).all() and (q.scale_l > 0).all()
        assert (np.abs(q.s_ld) <= q.scale_ld * (1 + 1e-15)).all() and np.isfinite(q.s_ld).all()
        print(f"{name}, {key}: |value| / scale per item from {float((np.abs(q.s_ld) / q.scale_ld).min()):.2e} to {float((np.abs(q.s_ld) / q.scale_ld).max()):.2e}")
    part = T.restated(name, shard=(m.n_nu // 3, m.n_nu // 3))
    for key in ("damping", "doppler", "centre"):
        q = getattr(part, key)
        assert (q.terms_ld <= a.terms_ld).all() and np.array_equal(q.terms_ld == 0, q.scale_ld == 0) and not q.s_ld[q.terms_ld == 0].any()


def test_entry_points_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    for cite in ("voigt.py:39-84", "voigt.py:148-149"):
        assert cite in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        declared = [("int64_t" in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ctypes.c_int for a in m.group(1).split(",")]
        assert declared == list(args), name
    # the twin of sdx_line_adjoint_dev: its arguments, followed by the six outputs
    assert _lib.PROTOTYPES["sdx_line_param_adjoint_dev"][1][:14] == _lib.PROTOTYPES["sdx_line_adjoint_dev"][1][:14]
    assert _lib.PROTOTYPES["sdx_line_param_adjoint_f64"][1][:11] == _lib.PROTOTYPES["sdx_line_adjoint_f64"][1][:11]


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_line_param_adjoint_dev(None, 4, 1, None, 0, 1, 1, None, None, None, 4, None, None, 1, None, None, None, None, None, None) == -1
    assert b"line_param_adjoint" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_line_param_adjoint_f64(None, 4, 1, None, 1, None, None, None, 4, None, None, None, None, None, None, None, None) == -1
    assert b"line_param_adjoint" in lib.sdx_last_error_string()
    assert lib.sdx_voigt_grad_dev(None, 1, None, None, None, None, None, None, None) == -1
    assert b"voigt_grad" in lib.sdx_last_error_string()


def test_validation_needs_no_device():
    from stardis_amd.engine import LINE_WRT, SpectralSynthesizer

    nus = np.linspace(7e14, 4e14, 5)
    ln, dw, g, al = np.array([5e14, 6e14]), np.ones((2, 4)), np.ones((2, 4)), np.ones((2, 4))
    good = dict(no_of_depth_points=4, tracing_nus_values=nus, line_nus=ln, doppler_widths=dw, gammas=g, alphas_array=al, weight=np.ones((4, 5)),
                ctx=NoDevice())
    for kw in (dict(weight=np.ones((4, 4))), dict(gammas=np.ones((2, 3))), dict(shard=(2, 4)), dict(shard=(-1, 2)), dict(wrt=("strength",)),
               dict(wrt=()), dict(wrt=("damping", "width"))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.line_param_adjoint(**args)
    with pytest.raises(AssertionError, match="the device was asked for"):  # (a valid call does reach the context)
        ops.line_param_adjoint(**good)
    with pytest.raises(ZeroDivisionError):
        ops.voigt_grad(1.0, 0.0, 1.0, ctx=NoDevice())

    assert LINE_WRT == ("strength",) + ops.LINE_PARAMS
    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.keep_response, syn.n_depth, syn.count, syn.n_lines, syn.instrument = NoDevice(), True, 4, 6, 2, None
    for bad in ("gamma", ("damping", "damping"), (), ("strength", "x")):
        for ask in (lambda: syn.line_sensitivities(wrt=bad), lambda: syn.observed_line_sensitivities(np.zeros(3), wrt=bad),
                    lambda: syn.chi2_line_gradient(np.zeros(3), np.ones(3), wrt=bad)):
            with pytest.raises(ValueError, match="wrt"):
                ask()
    with pytest.raises(ValueError, match="weights"):
        syn.line_sensitivities(np.zeros(5), wrt="damping")
    syn.keep_response = False
    for ask in (lambda: syn.line_sensitivities(wrt="centre"), lambda: syn.microturbulence_sensitivity(1e5), lambda: syn.microturbulence_sensitivity(0.0)):
        with pytest.raises(RuntimeError, match="keep_response=True"):
            ask()


def test_param_adjoint_kernels_do_not_spill(resources):  # noqa: F811
    """no spilled vector registers in the new adjoint kernels; the occupancy the compiler reports is recorded in the output"""
    new = {name: v for name, v in resources.items() if name.startswith("k_line_param_adjoint") or name == "k_voigt_grad"}
    assert set(new) == {"k_line_param_adjoint<4>", "k_line_param_adjoint<64>", "k_line_param_adjoint_tiled", "k_line_param_adjoint_gather", "k_voigt_grad"}, sorted(new)
    for name, v in sorted(new.items()):
        print(f"{name}: {v['vgpr']} VGPRs, {v['spill']} spilled, occupancy {v['occ']} waves / SIMD")
        assert v["spill"] == 0, (name, v)
    # the existing adjoint kernels are still there, under their own names
    assert {"k_line_adjoint<4>", "k_line_adjoint<64>", "k_line_adjoint_tiled", "k_line_adjoint_gather"} <= set(resources)
