"""Radial-tangential macroturbulence as include/stardis_hip.h defines it (sdx_macroturbulence_dev, sdx_macroturbulence_adjoint_dev)
restated in numpy, one window slice per point: what tests/test_gpu_macroturbulence.py holds the device against and
tests/test_macroturbulence_cpu.py pins by its own properties.  Same definition: windows, u, K = exp(-u^2) - sqrt(pi) u erfc(u) and
s = sqrt(pi) u erfc(u) in fp64 with scipy.special.erfc, in the header's order of operations; the trapezoid weights, the products and
the window sums in np.longdouble.

MACRO_TOL = 1e-12 of max |F| over the window, device against this restatement: the fp64 formula for K is within 6e-17 of its 40-digit
value at every u in [0, 7] (test_macroturbulence_cpu.py holds it to 1e-15); a device erfc or exp off by up to 16 ulp moves a weight by
less than 1e-15 of the peak; a lane-ordered fp64 sum over at most 701 terms adds less than 1e-13.  The profile has no edge: a point
within rounding of the window's end carries K(6) = 3e-18 of the peak, so no inclusion matters.
The derivative outputs are held to MACRO_TOL of max |F| times max(1, sum_j v_ij / den_i): dout = (sum v f - out sum v) / den is a
difference of two sums of size max |F| sum v / den, each carrying the relative error above (the ratio is 1 for a whole window, since
the integrals of s and K are both sqrt(pi) / 4)."""
import numpy as np
from scipy.special import erfc

from observe_reference import SUM_TOL  # noqa: F401  (identities between reordered sums: 1e-12 of the sum of the absolute terms)

MACRO_TOL = 1e-12  # of max |F| over the window, device against this restatement
C_KMS = 299792.458
REACH = 6.0  # the window: |u| <= 6
SQRT_PI = 1.7724538509055159  # np.sqrt(np.pi), the device's constant
LD = np.longdouble


def profile(u):
    """-> (K, s) in fp64 for u >= 0: K = max(exp(-(u u)) - s, 0), s = (sqrt(pi) u) erfc(u) = dK / d ln zeta"""
    u = np.asarray(u, dtype=np.float64)
    s = (SQRT_PI * u) * erfc(u)
    return np.maximum(np.exp(-(u * u)) - s, 0.0), s


def trapezoid_weights(lam):
    h = np.empty_like(lam)
    h[1:-1] = (lam[2:] - lam[:-2]) / 2
    h[0] = (lam[1] - lam[0]) / 2
    h[-1] = (lam[-1] - lam[-2]) / 2
    return h


def windows(lambdas, zeta):
    """-> (lam, beta, i0, i1) in fp64, the header's roundings: the points with lo_i <= lam_j <= hi_i are lam[i0[i]:i1[i]]"""
    lam = np.ascontiguousarray(lambdas, dtype=np.float64)
    beta = np.float64(zeta) / C_KMS
    reach = lam * (REACH * beta)
    return lam, beta, np.searchsorted(lam, lam - reach, "left"), np.searchsorted(lam, lam + reach, "right")


def point_rows(lambdas, zeta):
    """yields (i, j, w, v): the indices j point i includes, w_ij = K_ij h_j and v_ij = s_ij h_j over them (longdouble)"""
    lam, beta, i0, i1 = windows(lambdas, zeta)
    h = trapezoid_weights(lam.astype(LD))
    for i in range(lam.size):
        j = np.arange(min(i0[i], i), max(i1[i], i + 1))  # (i includes itself)
        K, s = profile(np.abs(lam[j] - lam[i]) / (lam[i] * beta))
        K[j == i], s[j == i] = 1.0, 0.0
        yield i, j, K.astype(LD) * h[j], s.astype(LD) * h[j]


def macroturbulence(lambdas, flux, zeta, reference=None, rows=None):
    """-> dict(out, dout, scale, dscale[, out_reference, dout_reference, scale_reference, dscale_reference]) in longdouble: the
    broadened flux, d / d ln zeta of it at fixed windows, max |F| over the included points and that times max(1, sum v / den) — what
    MACRO_TOL is taken against.  !(zeta > 0): a copy, the derivative 0."""
    given = {"": np.asarray(flux, dtype=np.float64).astype(LD)}
    if reference is not None:
        given["_reference"] = np.asarray(reference, dtype=np.float64).astype(LD)
    res = {}
    for tag, f in given.items():
        on = zeta > 0
        res["out" + tag], res["dout" + tag] = (np.empty_like(f), np.empty_like(f)) if on else (f.copy(), np.zeros_like(f))
        res["scale" + tag], res["dscale" + tag] = (np.empty_like(f), np.empty_like(f)) if on else (np.abs(f), np.abs(f))
    if not zeta > 0:
        return res
    for i, j, w, v in rows if rows is not None else point_rows(lambdas, zeta):
        den, vden = w.sum(), v.sum()
        for tag, f in given.items():
            out = (w * f[j]).sum() / den
            res["out" + tag][i], res["dout" + tag][i] = out, ((v * f[j]).sum() - out * vden) / den
            res["scale" + tag][i] = np.abs(f[j]).max()
            res["dscale" + tag][i] = res["scale" + tag][i] * max(LD(1), vden / den)
    return res


def adjoint(lambdas, u, zeta, u_reference=None, nus=None, rows=None):
    """-> (w, w_reference, scale, scale_reference) in longdouble: the transpose applied to u (and u_reference) and, per point j,
    sum_i h_j |a_i| over the i that include j (the peak term of each i, K = 1) — what MACRO_TOL is taken against: u is signed, the
    sums cancel, and a_i of the neighbours may be anything."""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    us = [np.asarray(a, dtype=np.float64).astype(LD) for a in (u, u_reference) if a is not None]
    ws, scales = [np.zeros_like(lam) for _ in us], [np.zeros_like(lam) for _ in us]
    if not zeta > 0:
        ws, scales = [a.copy() for a in us], [np.abs(a) for a in us]
    else:
        peak = trapezoid_weights(lam)
        for i, j, w, _ in rows if rows is not None else point_rows(lambdas, zeta):
            den = w.sum()
            for a, out, scale in zip(us, ws, scales):
                out[j] += w * (a[i] / den)
                scale[j] += peak[j] * np.abs(a[i] / den)
    if nus is not None:
        k = np.asarray(nus, dtype=np.float64).astype(LD) / lam
        ws, scales = [a * k for a in ws], [a * np.abs(k) for a in scales]
    return ws[0], ws[1] if len(us) > 1 else None, scales[0], scales[1] if len(us) > 1 else None


def dot_terms(lambdas, u, flux, zeta, rows=None):
    """sum_ij |u_i w_ij f_j / den_i|: what a bound on <macroturbulence(f), u> - <f, adjoint(u)> is taken against"""
    u, f = (np.asarray(a, dtype=np.float64).astype(LD) for a in (u, flux))
    if not zeta > 0:
        return float(np.sum(np.abs(u * f)))
    return float(sum(np.sum(np.abs(u[i] * w * f[j] / w.sum())) for i, j, w, _ in (rows if rows is not None else point_rows(lambdas, zeta))))


def window_lengths(lambdas, zeta):
    _, _, i0, i1 = windows(lambdas, zeta)
    return i1 - i0


def mapping_estimate(lambdas, zeta):
    """the expected window length the kernels' mapping tests against 32: 2 (6 beta) lam_i (n - 1) / (lam_{n-1} - lam_0)"""
    lam, beta, _, _ = windows(lambdas, zeta)
    return 2.0 * (REACH * beta) * lam * float(lam.size - 1) / (lam[-1] - lam[0])
