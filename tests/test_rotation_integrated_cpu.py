"""The cell-integrated rotation profile at build time and on the host: the six entry points are declared, exported and mirrored; the
new kernels compile for gfx950 without spilled vector registers and without LDS; a null context is refused; the names of
parameter_tangents are validated without a device; the restatement (tests/rotation_integrated_reference.py) against 50-digit mpmath
quadrature and by its own properties; and what tests/test_gpu_rotation_integrated.py relies on — its grids, the velocity at which every
window of the log-uniform grid gains a node, and the steps of its difference quotients with the restatement's own gap for each."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import rotation_integrated_reference as iref
import rotation_reference as rref
from conftest import ROOT
from rotation_integrated_reference import LD
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)
from test_observe_tangent_cpu import IRREGULAR, LAM, TWO_DENSITY

from stardis_amd import _lib
from stardis_amd import constants as K

ENTRIES = {"sdx_rotate_integrated_dev": 12, "sdx_rotate_integrated_adjoint_dev": 9, "sdx_rotate_integrated_f64": 13,
           "sdx_rotate_integrated_adjoint_f64": 10, "sdx_rotate_moments_dev": 7, "sdx_rotate_moments_f64": 7}

SLICE = np.ascontiguousarray(LAM[3000:4500])  # an S-c2 slice: 1500 log-uniform points, 0.013 A = 0.6 km/s apart
RATIO = float(np.median(SLICE[1:] / SLICE[:-1]))
V_STAR = float((RATIO ** 17 - 1.0) * K.C_KMS)  # lam_i (1 + V / c) = lam_{i+17}: every window gains its 17th node on the red side here
EDGE_GRID = 4096.0 * (1.0 + 2.0 ** -8) ** np.arange(7)  # test_gpu_rotation's: lam_{i+m} sits exactly on the profile's edge of point i
EDGE_V = tuple(float(((1.0 + 2.0 ** -8) ** m - 1.0) * K.C_KMS) for m in (1, 2))
SUB_SPACING_V = (0.599, 0.3, 0.03)  # reach / spacing = 0.999, 0.5, 0.05 on the slice
# the Richardson quotient of d / d ln V takes the forward at V e^(+-h) and V e^(+-h / 2).  The step is coarse on purpose: the device's
# forward carries a few 1e-16 of |F|, 1e-13 in the quotient at this h, and the restatement's own gap (1e-10 and more: the cases' test below
# prints it) must dominate that for twice the gap to be an allowance
LNV_STEP = 8.0e-3
# (grid name, V): the quotient cases of the GPU file; the flux is flux_of(grid)
QUOTIENT_CASES = (("slice", 2.0), ("slice", 10.0), ("slice", V_STAR), ("irregular", 10.0))
QUOTIENT_GRIDS = {"slice": SLICE, "irregular": np.ascontiguousarray(IRREGULAR[1000:1700])}


def flux_of(lam, seed=11):
    """a spectrum with lines a few points wide on a smooth continuum: what a quotient in V can see"""
    rng = np.random.default_rng(seed)
    centres, depth = rng.uniform(lam[0], lam[-1], 40), rng.uniform(0.1, 0.8, 40)
    return 1.0 + 0.02 * np.sin(lam / 0.7) - np.sum(depth[:, None] * np.exp(-0.5 * ((lam[None, :] - centres[:, None]) / 0.04) ** 2), axis=0)


def mp_of(v):
    """a longdouble as an mpf, exactly (its two fp64 halves)"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - LD(hi)))


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
    # v sin i and eps by value in the host-buffer twins; the device entries read the pair from device memory
    for name in ("sdx_rotate_integrated", "sdx_rotate_integrated_adjoint"):
        at = 5 if name.endswith("integrated") else 3
        assert _lib.PROTOTYPES[name + "_f64"][1][at:at + 2] == [ctypes.c_double] * 2 and _lib.PROTOTYPES[name + "_dev"][1][at] is ctypes.c_void_p


def test_integrated_kernels_do_not_spill_and_the_sampled_ones_keep_their_registers(resources):  # noqa: F811
    """the bounds are what the build gives (printed): the cell's moments carry atan2 of the device library, two square roots and four
    divisions — 112 vector registers without the derivatives, 124 with them, 98 and 126 in the adjoint's two kernels: four waves per SIMD
    where k_rotate has eight; no spill, no LDS.  k_rotate and k_rotate_tangent keep the registers test_observe_tangent_cpu pins."""
    bounds = (("k_rotate_integrated<false>", 112, 4), ("k_rotate_integrated<true>", 128, 4), ("k_rotate_integrated_adjoint_den", 104, 4),
              ("k_rotate_integrated_adjoint", 128, 4), ("k_rotate_moments", 48, 8), ("k_rotate", 52, 8), ("k_rotate_tangent", 64, 8))
    for name, vgpr, occ in bounds:
        found = [v for k, v in resources.items() if k == name]
        assert len(found) == 1, sorted(resources)
        print(name, found[0])
        assert found[0]["spill"] == 0 and found[0]["lds"] == 0 and found[0]["occ"] >= occ and found[0]["vgpr"] <= vgpr, (name, found[0])


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    none = [None] * 10
    assert lib.sdx_rotate_integrated_dev(None, 4, *none) == -1
    assert b"rotate_integrated: null context" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_rotate_integrated_f64(None, 4, None, None, None, 10.0, 0.6, *none[:6]) == -1
    assert lib.sdx_rotate_integrated_adjoint_dev(None, 4, *none[:7]) == -1 and b"rotate_integrated_adjoint" in lib.sdx_last_error_string()
    assert lib.sdx_rotate_integrated_adjoint_f64(None, 4, None, 10.0, 0.6, *none[:5]) == -1
    assert lib.sdx_rotate_moments_dev(None, 4, *none[:5]) == -1 and b"rotate_moments" in lib.sdx_last_error_string()
    assert lib.sdx_rotate_moments_f64(None, 4, *none[:5]) == -1


def test_validation_needs_no_device():
    from stardis_amd import ops
    from stardis_amd.instrument import Instrument

    class Host(Instrument):  # the name checks are plain Python: an instrument without a device
        def __init__(self, v_rot=None, v_mac=None, rotation=None):
            self.rotates, self.macroturbulent, self.v_rot, self.v_mac = v_rot is not None, v_mac is not None, v_rot, v_mac
            if rotation is not None:
                self.rotation = rotation

    for inst in (Host(v_rot=10.0), Host(v_rot=10.0, rotation="sampled")):
        with pytest.raises(ValueError, match='rotation="integrated"'):
            inst._wrt("v_rot")
        with pytest.raises(ValueError, match='rotation="integrated"'):
            inst._wrt(("v_rad", "v_rot"))
        assert inst._wrt(None) == ("v_rad", "lsf", "limb_darkening")
    assert Host(v_rot=10.0, v_mac=3.0)._wrt(None) == Instrument.PARAMETERS == ("v_rad", "lsf", "v_mac", "limb_darkening")
    assert Instrument.INTEGRATED_PARAMETERS == ("v_rot",)
    integrated = Host(v_rot=10.0, v_mac=3.0, rotation="integrated")
    assert integrated._wrt(None) == Instrument.PARAMETERS + ("v_rot",) and integrated._wrt("v_rot") == ("v_rot",)
    assert Host(v_rot=10.0, rotation="integrated")._wrt(None) == ("v_rad", "lsf", "limb_darkening", "v_rot")
    assert Host(v_rot=0.0, rotation="integrated")._wrt(None) == ("v_rad", "lsf") and Host(rotation="integrated")._wrt(None) == ("v_rad", "lsf")
    with pytest.raises(ValueError, match="v_rad, lsf, v_mac, limb_darkening"):
        integrated._wrt(("v_rot", "v_sin_i"))
    with pytest.raises(RuntimeError, match="no rotation"):
        Host(v_mac=3.0, rotation="integrated")._wrt("v_rot")
    with pytest.raises(ValueError, match="v_rot > 0"):
        Host(v_rot=0.0, rotation="integrated")._wrt("v_rot")
    with pytest.raises(ValueError, match="sampled, integrated"):
        Instrument(np.linspace(6562.0, 6568.0, 11), resolving_power=5.0e4, v_rot=10.0, rotation="exact")
    lam = np.linspace(6560.0, 6570.0, 50)
    for call in (lambda: ops.rotate_integrated(lam[::-1], np.ones(50), 10.0), lambda: ops.rotate_integrated(lam, np.ones(49), 10.0),
                 lambda: ops.rotate_integrated(lam, np.ones(50), -1.0), lambda: ops.rotate_integrated(lam, np.ones(50), 10.0, limb_darkening=1.5),
                 lambda: ops.rotate_integrated(lam, np.ones(50), 10.0, reference=np.ones(3)), lambda: ops.rotate_integrated(lam[:1], np.ones(1), 10.0),
                 lambda: ops.rotate_integrated_adjoint(lam, np.ones(49), 10.0), lambda: ops.rotate_integrated_adjoint(lam, np.ones(50), 3000.0),
                 lambda: ops.rotate_integrated_adjoint(lam, np.ones(50), 10.0, nus=np.ones(2))):
        with pytest.raises(ValueError):
            call()
    if _lib.load().sdx_device_count() == 0:  # valid arguments: then, and only then, the device is asked for (no CPU fallback)
        with pytest.raises(RuntimeError):
            ops.rotate_integrated(lam, np.ones(50), 10.0)
        with pytest.raises(RuntimeError):
            ops.rotate_integrated_adjoint(lam, np.ones(50), 10.0)
        with pytest.raises(RuntimeError):
            ops.rotate_moments(-0.5, 0.5)


# ---- the restatement against quadrature -------------------------------------------------------------------------------------------------
def test_the_restatement_against_50_digit_quadrature_of_K_phi():
    """every weight W_ij of a few rows — interior, truncated, a window narrower than a cell, a node on the edge — against mpmath's
    quadrature of K(y) phi_j(y), phi_j node j's hat function: to 1e-15 of den_i (5e-17 was measured when the operator was proposed)"""
    mpmath.mp.dps = 50
    worst = 0.0
    cases = [(IRREGULAR[:400], 10.0, 0.6, (0, 3, 200, 399)), (SLICE[:300], 2.0, 0.0, (0, 150, 299)), (SLICE[:300], 0.3, 1.0, (0, 150)),
             (EDGE_GRID, EDGE_V[0], 0.6, (0, 3, 6)), (TWO_DENSITY[480:560], 10.0, 0.6, (18, 20, 22))]
    for lam, V, eps, points in cases:
        got = {r.i: r for r in iref.rows(lam, V, eps) if r.i in points}
        x = [mpmath.mpf(float(v)) for v in lam]
        e, hp, fp64_reach = mpmath.mpf(eps), mpmath.mpf(float(np.pi / 2)), iref.reaches(lam, V)
        for i in points:
            reach = mpmath.mpf(float(fp64_reach[i]))  # (the row's parameter, as the definition rounds it)
            Kf = lambda y: 2 * (1 - e) * mpmath.sqrt(max(1 - y * y, 0)) + hp * e * (1 - y * y)  # noqa: E731
            row, exact = got[i], []
            for k in range(row.W.size):
                j, total = row.j0 + k, mpmath.mpf(0)
                for a, b, rising in ((j - 1, j, True), (j, j + 1, False)):  # the two cells of node j's hat
                    if a < 0 or b >= lam.size:
                        continue
                    ya, yb = (x[a] - x[i]) / reach, (x[b] - x[i]) / reach
                    lo, hi = max(ya, -1), min(yb, 1)
                    if hi > lo:
                        phi = (lambda y: (y - ya) / (yb - ya)) if rising else (lambda y: (yb - y) / (yb - ya))  # noqa: E731
                        pts = sorted({lo, hi} | {mpmath.mpf(0)} if lo < 0 < hi else {lo, hi})
                        total += mpmath.quad(lambda y: Kf(y) * phi(y), pts)
                exact.append(total)
            den = sum(exact)
            worst = max([worst] + [float(abs(mp_of(w) - t) / den) for w, t in zip(row.W, exact)])
            assert float(abs(mp_of(row.den) - den) / den) <= 1e-15
    print(f"worst |W_ij - 50-digit quadrature| / den_i = {worst:.3e}, allowed 1e-15")
    assert 0 < worst <= 1e-15


def test_the_moments_of_the_restatement_against_mpmath():
    """the antiderivative differences in longdouble on the GPU file's cells: what the device's moments are NOT formed from, so the two
    agree only if both are right; here to 1e-15 of the cell's own M0 for cells 1e-3 wide and wider"""
    mpmath.mp.dps = 50
    ya, yb = moment_cells()
    keep = yb - ya >= 1e-3
    S0, Q0, S1, Q1 = iref.moments(ya[keep], yb[keep])
    for eps in (0.0, 0.6, 1.0):
        m0, m1 = 2 * (1 - LD(eps)) * S0 + iref.half_pi() * LD(eps) * Q0, 2 * (1 - LD(eps)) * S1 + iref.half_pi() * LD(eps) * Q1
        for a, b, v0, v1 in zip(ya[keep], yb[keep], m0, m1):
            e0, e1 = iref.mp_moments(a, b, eps)
            assert abs(mp_of(v0) - e0) <= 1e-15 * e0 and abs(mp_of(v1) - e1) <= 1e-15 * e0, (a, b, eps)


def moment_cells():
    """-> (ya, yb): the cells of the moments' checks — 1e-6 to 2 wide, touching -1 and +1, both ends in one half, spanning 0, reaching
    past the clamp"""
    ya, yb = [], []
    for width in (1e-6, 1e-4, 1e-2, 0.1, 0.5):
        start = np.r_[-1.0, -0.9, -0.5 - width, -width, 0.0, 0.3, 0.7, 1.0 - width]
        start = np.r_[start, -width / 3, 0.5 - width / 2]  # spanning 0; around 1/2
        ya += [start]
        yb += [start + width]
    ya += [np.array([-1.0, -1.0, 0.0, -1.0, -0.25, -50.0, 0.99, -3.0])]
    yb += [np.array([1.0, 0.0, 1.0, 0.75, 1.0, -0.99, 70.0, 3.0])]
    ya, yb = np.concatenate(ya), np.concatenate(yb)
    yb[np.isclose(yb, 1.0, rtol=0, atol=1e-15)] = 1.0
    return ya, yb


# ---- the restatement by its own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,V", [("irregular", 10.0), ("two-density", 23.7), ("slice", 2.0), ("slice", 0.3), ("edge", EDGE_V[1])])
def test_row_sums_and_the_reproduction_of_linear_flux(grid, V):
    lam = {"irregular": IRREGULAR[:600], "two-density": TWO_DENSITY[300:800], "slice": SLICE[:400], "edge": EDGE_GRID}[grid]
    fl = 3 - LD(0.002) * (lam.astype(LD) - lam[0])  # linear in longdouble from the fp64 nodes
    f = fl.astype(np.float64)
    interior = 0
    for row in iref.rows(lam, V, 0.6):
        assert abs(row.W.sum() - row.den) <= 1e-18 * row.den and row.den > 0 and np.all(row.W >= -1e-18 * row.den)
        assert abs(row.T.sum() - row.tsum) <= 1e-17 * np.abs(row.T).sum() + 1e-30
        if not row.truncated:
            interior += 1
            assert row.tsum == 0 and row.e0 == 0 and row.e1 == 0
            # sum_j W_ij lam_j = lam_i den_i: the profile is even, the hats reproduce a linear function
            assert abs((row.W * fl[row.j0:row.j0 + row.W.size]).sum() / row.den - fl[row.i]) <= 1e-17 * abs(fl[row.i]), (grid, row.i)
            assert abs((row.T * fl[row.j0:row.j0 + row.T.size]).sum()) <= 1e-16 * row.den  # ... for every V: no derivative
    assert interior > (0 if grid == "edge" else 100)
    if grid in ("irregular", "two-density"):
        sampled = rref.rotate(lam, f, V, 0.6)[0]
        inner = ~np.array([r.truncated for r in iref.rows(lam, V, 0.6)])
        assert np.max(np.abs(sampled - f)[inner]) > 1e-9  # the sampled sum has no such property where the spacing varies
    elif grid == "edge":
        assert not rref.clear_of_profile_edge(lam, V, 1e-8)  # no exemption is needed here


def test_the_operator_tends_to_the_identity_continuously():
    """reach / spacing = 0.999, 0.5, 0.05: a window narrower than one spacing still has three weights, and out_i -> f_i"""
    f = flux_of(SLICE)
    gaps = []
    for V in SUB_SPACING_V:
        ratio = V / K.C_KMS * SLICE[750] / (SLICE[751] - SLICE[750])
        r = iref.rotate(SLICE, f, V, 0.6)
        row = next(x for x in iref.rows(SLICE, V, 0.6) if x.i == 750)
        assert row.W.size == 3 and np.all(row.W > 0)
        gaps.append(float(np.max(np.abs(r["out"] - f))))
        print(f"V = {V}: reach / spacing {ratio:.3f}, max |out - f| = {gaps[-1]:.3e}, the neighbours' share {float((row.W[0] + row.W[2]) / row.den):.3e}")
        assert abs(ratio - {0.599: 0.999, 0.3: 0.5, 0.03: 0.05}[V]) < 2e-3
    assert gaps[0] > gaps[1] > gaps[2] > 0 and gaps[2] < 0.06 * gaps[0]  # the neighbours' share is (4 / (3 pi)) reach / spacing: linear in V


@pytest.mark.parametrize("grid,V", QUOTIENT_CASES + (("slice-end", 40.0),))
def test_the_derivative_against_richardson_quotients_of_the_restatement(grid, V):
    """T, end terms included, against the Richardson value of the restatement's own forward at the GPU file's step: interior points
    and ("slice-end") a short grid on which every window is truncated.  d out / dV is continuous but only Hoelder-1/2 where a node crosses
    a profile edge, so the gap does not fall like h^4; what it is here is what the device's quotient is allowed twice of."""
    lam = SLICE[:120] if grid == "slice-end" else QUOTIENT_GRIDS[grid]
    f = flux_of(lam)
    gap, size = iref.quotient_gap(lam, f, V, 0.6, LNV_STEP)
    exact = iref.rotate(lam, f, V, 0.6)["dlnv"]
    fine = float(np.max(np.abs(iref.richardson(lambda v: iref.rotate(lam, f, float(v), 0.6)["out"], V, LNV_STEP / 4) - exact)))
    print(f"{grid}, V = {V:.6f}: largest |d out / d ln V| {size:.3e}, gap of the Richardson value at h = {LNV_STEP}: {gap:.3e}, at h / 4: {fine:.3e}")
    if grid == "slice-end":
        assert all(r.truncated for r in iref.rows(lam, V, 0.6)) and any(r.e0 != 0 and r.e1 != 0 for r in iref.rows(lam, V, 0.6))
    # the analytic derivative and the quotient agree to the quotient's own error, which falls with the step
    assert 1e-11 < gap <= 1e-2 * size and fine < gap and fine <= 1e-3 * size and size > 1e-3


def test_v_star_is_where_every_window_gains_a_node():
    below, above = rref.window_lengths(SLICE, V_STAR * (1 - 1e-9)), rref.window_lengths(SLICE, V_STAR * (1 + 1e-9))
    inner = slice(40, -40)
    print(f"V* = {V_STAR!r}: windows of {below[inner].min()} .. {below[inner].max()} points just below, {above[inner].min()} .. {above[inner].max()} just above")
    assert np.all(above[inner] - below[inner] >= 1) and 9.0 < V_STAR < 11.0
