"""Rotational broadening as include/stardis_hip.h defines it (sdx_rotate_dev, sdx_rotate_adjoint_dev) restated in numpy, in
np.longdouble from the fp64 inputs, one window slice per point: what tests/test_gpu_rotation.py holds the device against and
tests/test_rotation_cpu.py pins by its own properties.  Same definition; the roundings are those of the longer format and the sums
numpy's.

The profile has a square-root edge: where a point j sits within a few ulp of lo_i or hi_i, q_ij is a few ulp, its term is
sqrt(few ulp) ~ 2e-8 of the profile's peak, and whether it is included hinges on one rounding.  clear_of_profile_edge(lam, V, margin)
says that no pair of a window has |1 - |y_ij|| < margin.  With margin = 1e-8 the device's q (a few roundings, dq <~ 1e-15) moves an edge
term by at most dq / (2 sqrt(2e-8)) ~ 3e-12 of the peak and every other term by a few ulp, hence ROT_TOL."""
import numpy as np

from observe_reference import SUM_TOL  # noqa: F401  (identities between reordered sums: 1e-12 of the sum of the absolute terms)

ROT_TOL = 1e-11  # of max |F| over the window, device against this restatement
C_KMS = 299792.458
LD = np.longdouble


def trapezoid_weights(lam):
    h = np.empty_like(lam)
    h[1:-1] = (lam[2:] - lam[:-2]) / 2
    h[0] = (lam[1] - lam[0]) / 2
    h[-1] = (lam[-1] - lam[-2]) / 2
    return h


def windows(lambdas, V):
    """-> (lam, reach, i0, i1) in longdouble: the points with lo_i <= lam_j <= hi_i are lam[i0[i]:i1[i]] (obs_windows with D = 1)"""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    reach = lam * (LD(V) / LD(C_KMS))
    return lam, reach, np.searchsorted(lam, lam - reach, "left"), np.searchsorted(lam, lam + reach, "right")


def point_rows(lambdas, V, eps):
    """yields (i, j, w): the indices j point i includes and w_ij = K_ij h_j over them"""
    lam, reach, i0, i1 = windows(lambdas, V)
    h = trapezoid_weights(lam)
    c_sqrt, c_q = 2 * (1 - LD(eps)), LD(np.float64(np.pi / 2)) * LD(eps)  # (pi / 2: the fp64 constant, as the device has it)
    for i in range(lam.size):
        j = np.arange(i0[i], i1[i])
        y = (lam[j] - lam[i]) / reach[i]
        q = 1 - y * y
        keep = (q > 0) | (j == i)
        j, q = j[keep], np.where(j == i, LD(1), q)[keep]
        yield i, j, (c_sqrt * np.sqrt(q) + c_q * q) * h[j]


def rotate(lambdas, flux, V, eps, reference=None):
    """-> (out, out_reference, scale, scale_reference) in longdouble: the broadened flux and reference (None without one) and, per
    point, max |F| over the included points — what ROT_TOL is taken against.  !(V > 0): a copy."""
    f = np.asarray(flux, dtype=np.float64).astype(LD)
    g = None if reference is None else np.asarray(reference, dtype=np.float64).astype(LD)
    if not V > 0:
        return f.copy(), None if g is None else g.copy(), np.abs(f), None if g is None else np.abs(g)
    out, scale = np.empty_like(f), np.empty_like(f)
    out_ref, scale_ref = (None, None) if g is None else (np.empty_like(f), np.empty_like(f))
    for i, j, w in point_rows(lambdas, V, eps):
        den = w.sum()
        out[i], scale[i] = (w * f[j]).sum() / den, np.abs(f[j]).max()
        if g is not None:
            out_ref[i], scale_ref[i] = (w * g[j]).sum() / den, np.abs(g[j]).max()
    return out, out_ref, scale, scale_ref


def adjoint(lambdas, u, V, eps, u_reference=None, nus=None):
    """-> (w, w_reference, scale, scale_reference) in longdouble: the transpose applied to u (and u_reference) and, per point j,
    sum_i K_peak h_j |a_i| over the i that include j, K_peak = K at q = 1 — what ROT_TOL is taken against: the device's term for an
    (i, j) near the profile's edge is off by up to 3e-12 of the PEAK term of that i, not of its own small value (u is signed, the sums
    cancel, and a_i of the neighbours may be anything)."""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    us = [np.asarray(a, dtype=np.float64).astype(LD) for a in (u, u_reference) if a is not None]
    ws, scales = [np.zeros_like(lam) for _ in us], [np.zeros_like(lam) for _ in us]
    if not V > 0:
        ws, scales = [a.copy() for a in us], [np.abs(a) for a in us]
    else:
        peak = (2 * (1 - LD(eps)) + LD(np.float64(np.pi / 2)) * LD(eps)) * trapezoid_weights(lam)
        for i, j, w in point_rows(lambdas, V, eps):
            den = w.sum()
            for a, out, scale in zip(us, ws, scales):
                out[j] += w * (a[i] / den)
                scale[j] += peak[j] * np.abs(a[i] / den)
    if nus is not None:
        k = np.asarray(nus, dtype=np.float64).astype(LD) / lam
        ws, scales = [a * k for a in ws], [a * np.abs(k) for a in scales]
    return ws[0], ws[1] if len(us) > 1 else None, scales[0], scales[1] if len(us) > 1 else None


def dot_terms(lambdas, u, flux, V, eps):
    """sum_ij |u_i w_ij f_j / den_i|: what a bound on <rotate(f), u> - <f, adjoint(u)> is taken against"""
    u, f = (np.asarray(a, dtype=np.float64).astype(LD) for a in (u, flux))
    if not V > 0:
        return float(np.sum(np.abs(u * f)))
    return float(sum(np.sum(np.abs(u[i] * w * f[j] / w.sum())) for i, j, w in point_rows(lambdas, V, eps)))


def window_lengths(lambdas, V):
    _, _, i0, i1 = windows(lambdas, V)
    return i1 - i0


def profile_edge_margin(lambdas, V):
    """the smallest |1 - |y_ij|| over the pairs inside the windows and the nearest points outside them (j != i)"""
    lam, reach, i0, i1 = windows(lambdas, V)
    worst = np.inf
    for i in range(lam.size):
        j = np.arange(max(i0[i] - 1, 0), min(i1[i] + 1, lam.size))
        j = j[j != i]
        if j.size:
            worst = min(worst, float(np.min(np.abs(1 - np.abs((lam[j] - lam[i]) / reach[i])))))
    return worst


def clear_of_profile_edge(lambdas, V, margin):
    """no pair (i, j) of a window, or just outside one, with |1 - |y_ij|| < margin: no inclusion hinges on one rounding, and no
    included term is the square root of a few ulp"""
    return profile_edge_margin(lambdas, V) >= margin
