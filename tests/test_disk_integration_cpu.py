"""Disk integration with rigid rotation without a GPU: the restatement (tests/disk_integration_reference.py) is the operator
include/stardis_hip.h states — its moments against 40-digit closed forms, its windows normalised, a linear spectrum reproduced, the
limit of many rings Gray's profile —, the entry points are declared, exported and mirrored, and the Python-side validation of
ops.emergent_intensity and ops.disk_integrate raises before any device is asked for.

The Gray limit.  Rings at the Gauss-Legendre nodes of s = sin(theta) in [0, 1] with the weight 2 s ds and I_r = f (1 - eps + eps sqrt(1 -
s^2)), normalised by the quadrature's own sum of w_r (1 - eps + eps mu_r), against rotation_integrated_reference.rotate at the same (V,
eps) on a blended two-line spectrum, V = 30 km/s, eps = 0.6, a jittered grid of 240 points (about 16 points per reach), 40 interior
points: measured with the two restatements alone 8.24e-5 at 20 rings and 7.41e-8 at 256 (8 rings: 1.1e-4, 64 rings: 4.8e-6; the
quadrature of the square-root limb factor in s converges like n_rings^-3).  The comparator is a limit in the number of rings, not a
rounding matter; the bounds are 4 x the measured values, 3.3e-4 and 3.0e-7, the margin for the grid dependence."""
import ctypes
import re

import mpmath
import numpy as np
import pytest

import disk_integration_reference as D
import rotation_integrated_reference as G
from conftest import ROOT
from test_engine_host_cpu import NoDevice

from stardis_amd import _lib, ops

LD = D.LD
needs_extended = pytest.mark.skipif(not D.EXTENDED, reason="no extended-precision long double on this host")
ENTRIES = {"sdx_emergent_intensity_dev": 14, "sdx_emergent_intensity_f64": 11, "sdx_disk_integrate_dev": 12, "sdx_disk_integrate_f64": 11}
GRAY_BOUND = {20: 4 * 8.24e-5, 256: 4 * 7.41e-8}  # 4 x what the two restatements measured (the docstring)


def two_lines(lam):
    return 1.0 - 0.6 * np.exp(-0.5 * ((lam - 6564.6) / 0.12) ** 2) - 0.35 * np.exp(-0.5 * ((lam - 6565.3) / 0.2) ** 2)


def jittered_grid(n, seed=7):
    rng = np.random.default_rng(seed)
    return np.sort(6560.0 + 10.0 * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n)


def cells():
    """(ya, yb): widths 1e-7 .. 2, anywhere in [-1, 1], touching +-1, spanning 0 (symmetric and not)"""
    out = []
    for width in (1e-7, 1e-5, 1e-3, 0.03, 0.4, 1.0):
        for left in (-1.0, -0.9, -0.5, -width, -0.3 * width, -0.5 * width, 0.0, 0.2, 0.7, 1.0 - width):
            if -1.0 <= left and left + width <= 1.0:
                out.append((left, left + width))
    return out + [(-1.0, 1.0), (-1.0, 0.0), (0.0, 1.0), (-0.25, 1.0), (-1.5, 0.3), (0.4, 2.0)]


@needs_extended
def test_moments_against_closed_forms():
    """relative 1e-17 (1 + 1 / width): the difference of antiderivatives loses the cell's width.  M1 of a cell that spans 0 is a
    difference of its halves' moments and is held on the scale of their sum, int |y| over the cell."""
    exact = lambda v: mpmath.mpf(float(v)) + mpmath.mpf(float(v - LD(float(v))))  # noqa: E731  (a longdouble as the sum of two doubles)
    worst = 0.0
    with mpmath.workdps(40):
        for ya, yb in cells():
            m0, m1 = (v[()] for v in D.moments(ya, yb))
            t0, t1 = D.mp_moments(ya, yb)
            a, b = max(ya, -1.0), min(yb, 1.0)
            tol = 1e-17 * (1.0 + 1.0 / (b - a))
            scale1 = abs(t1) if a >= 0 or b <= 0 else D.mp_moments(0.0, b)[1] - D.mp_moments(a, 0.0)[1]
            e0, e1 = abs(exact(m0) - t0) / t0, abs(exact(m1) - t1) / scale1
            worst = max(worst, float(e0 / tol), float(e1 / tol))
            assert e0 <= tol and e1 <= tol, (ya, yb, float(e0), float(e1), tol)
    print(f"moments against 40 digits: worst error / allowance = {worst:.3f}")


@needs_extended
def test_windows_are_normalised_and_linear_spectra_reproduced():
    lam = jittered_grid(120)
    lam_ld = lam.astype(LD)
    line = 3.0 - 0.25 * (lam - 6565.0)
    # the definition divides by the fp64 constant pi: a complete window sums to pi / fl(pi) = 1 + 3.9e-17, which the quotient removes
    one = np.arccos(LD(-1)) / D.pi64()
    for V, scale in ((30.0, 1.0), (30.0, 0.31), (2.0, 1.0), (0.05, 0.5)):
        reach = D.reaches(lam, V, scale)
        worst_norm = worst_line = 0.0
        for i in range(lam.size):
            row = D.row(lam_ld, i, reach[i])
            if row.truncated:
                continue
            worst_norm = max(worst_norm, abs(float(row.den - one)))
            worst_line = max(worst_line, abs(float((row.W * line[row.j0:row.j0 + row.W.size].astype(LD)).sum() / row.den - line[i])))
        print(f"V={V} scale={scale}: |sum M0 - 1| <= {worst_norm:.2e}, linear spectrum to {worst_line:.2e}")
        assert worst_norm <= 1e-17 and worst_line <= 3.0 * 1e-16  # a few longdouble roundings of O(1) and of the spectrum's scale
    # a node exactly on the ring's edge closes a cell of zero length: nothing beyond it is weighted
    lam = np.array([2.0, 3.0, 4.0, 5.0, 6.0]) * 1000.0
    V = D.C_KMS / 4.0  # beta = 0.25 exactly: the reach at lam = 4000 is 1000, the neighbours sit on the edge
    assert D.reaches(lam, V, 1.0)[2] == 1000.0
    row = D.row(lam.astype(LD), 2, D.reaches(lam, V, 1.0)[2])
    assert row.W[0] == 0 and row.W[-1] == 0 and abs(float(row.den - one)) <= 1e-18


@needs_extended
def test_v_zero_and_continuity():
    lam = jittered_grid(60)
    rng = np.random.default_rng(3)
    s, w, limb = D.gray_rings(5, 0.6)
    I = limb[:, None] * two_lines(lam)[None, :] * rng.uniform(0.9, 1.1, (5, 1))
    flat, _ = D.disk_integrate(lam, I, s, w, 0.0)
    assert np.max(np.abs(flat - D.flux_order_sum(I, w).astype(LD))) <= 4e-16 * float(np.abs(I).max() * w.sum())
    # V -> 0: the window is under one spacing and still has three weights; the distance from the flux sum shrinks with V
    gaps = [float(np.max(np.abs(D.disk_integrate(lam, I, s, w, V)[0] - flat))) for V in (1e-1, 1e-2, 1e-3)]
    print("V -> 0:", gaps)
    assert gaps[0] > gaps[1] > gaps[2] > 0 and gaps[2] <= 2e-2 * gaps[0]  # (linear in V under one spacing)
    row = D.row(lam.astype(LD), 30, D.reaches(lam, 1e-3, 1.0)[30])
    assert row.W.size == 3 and np.all(row.W > 0)


@needs_extended
@pytest.mark.parametrize("n_rings", [20, 256])
def test_gray_limit(n_rings):
    """the bound: 4 x the distance measured with the two restatements alone (module docstring): 3.3e-4 at 20 rings, 3.0e-7 at 256"""
    V, eps = 30.0, 0.6
    lam = jittered_grid(240)
    f = two_lines(lam)
    points = list(range(40, 200, 4))
    ref = G.rotate(lam, f, V, eps)["out"][points]
    s, w, limb = D.gray_rings(n_rings, eps)
    out, _ = D.disk_integrate(lam, limb[:, None] * f[None, :], s, w, V, points)
    gap = float(np.max(np.abs(out / np.sum(w * limb) - ref)))
    print(f"{n_rings} rings against Gray's profile: {gap:.3e} (bound {GRAY_BOUND[n_rings]:.1e})")
    assert gap <= GRAY_BOUND[n_rings]


def test_entries_are_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/stardis_hip.h").read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    doc = open(f"{ROOT}/include/stardis_hip.h").read()
    for stage in ('"k_emergent_intensity"', '"k_disk_integrate"'):
        assert stage in doc


def test_emergent_intensity_validates_on_the_host():
    nus, t = np.linspace(7e14, 4e14, 6), np.linspace(4000.0, 9000.0, 4)
    good = dict(tracing_nus=nus, temperatures=t, ray_distances=np.ones((3, 5)), total_alphas=np.ones((4, 6)), ctx=NoDevice())
    for kw in (dict(ray_distances=np.ones((4, 5))), dict(ray_distances=np.ones(15)), dict(ray_distances=np.ones((3, 65))),
               dict(total_alphas=np.ones((4, 5))), dict(total_alphas=np.ones((3, 6))), dict(source=np.ones((4, 5))),
               dict(temperatures=np.array([5000.0]), ray_distances=np.ones((0, 5)))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.emergent_intensity(**args)
    with pytest.raises(AssertionError, match="the device was asked for"):  # (a valid call does reach the context)
        ops.emergent_intensity(**good)


def test_disk_integrate_validates_on_the_host():
    lam = np.linspace(5000.0, 5001.0, 8)
    good = dict(lambdas=lam, intensities=np.ones((3, 8)), ring_scale=[0.0, 0.5, 1.0], ring_weights=np.ones(3), v_rot=10.0, ctx=NoDevice())
    for kw in (dict(lambdas=lam[::-1]), dict(lambdas=lam[:1], intensities=np.ones((3, 1))), dict(intensities=np.ones((3, 7))),
               dict(intensities=np.ones((2, 8))), dict(intensities=np.ones(24)), dict(ring_scale=[0.0, 0.5, 1.5]), dict(ring_scale=[-0.1, 0.5, 1.0]),
               dict(ring_scale=[]), dict(ring_scale=np.linspace(0, 1, 65), ring_weights=np.ones(65), intensities=np.ones((65, 8))),
               dict(ring_weights=np.ones(4)), dict(v_rot=-1.0), dict(v_rot=np.nan), dict(v_rot=3000.0), dict(reference=np.ones((3, 7)))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.disk_integrate(**args)
    with pytest.raises(AssertionError, match="the device was asked for"):
        ops.disk_integrate(**good)


def test_engine_options_without_a_device():
    from stardis_amd.engine import SpectralSynthesizer

    syn = object.__new__(SpectralSynthesizer)
    assert syn.keep_intensities is False  # the class's default: a bare synthesizer launches what it launched
    syn.ctx = NoDevice()
    with pytest.raises(RuntimeError, match="keep_intensities=True"):
        syn.emergent_intensities
    with pytest.raises(RuntimeError, match="keep_intensities=True"):
        syn.disk_integrated(10.0)
    syn.keep_intensities, syn.d_I, syn.begin, syn.count, syn.n_nu = True, object(), 2, 4, 8
    with pytest.raises(ValueError, match="whole spectrum"):
        syn.disk_integrated(10.0)
    syn.begin, syn.count = 0, 8
    with pytest.raises(ValueError, match="v_rot"):
        syn.disk_integrated(-3.0)
    syn.instrument = None
    with pytest.raises(RuntimeError, match="instrument"):
        syn.observed_disk_integrated(10.0)
    syn.instrument = type("I", (), {"rotates": True})()
    with pytest.raises(ValueError, match="rotation twice"):
        syn.observed_disk_integrated(10.0)
    syn.keep_contribution = syn.keep_response = False
    syn.scattering, syn._keep_total = None, True
    with pytest.raises(ValueError, match="keep_intensities"):
        syn.keep_total = False
