"""The instrument model of include/stardis_hip.h (sdx_observe_dev) restated in numpy, one window slice per pixel, with
scipy.special.erf / erfc: what tests/test_gpu_observe.py holds the device against and tests/test_observe_cpu.py pins by its own
properties.  Same definition, same operations per point; only the order of the sums (numpy's pairwise sum) differs."""
import math

import numpy as np
from scipy.special import erf, erfc

FLUX_TOL = 1e-10  # of |ref|, device against this restatement
SUM_TOL = 1e-12   # identities between reordered sums
C_KMS = 299792.458
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


def doppler_factor(v_kms):
    beta = v_kms / C_KMS
    return math.sqrt((1.0 + beta) / (1.0 - beta))


def sigma_of_R(edges, R):
    edges = np.asarray(edges, dtype=np.float64)
    return (edges[:-1] + edges[1:]) / 2 / (np.asarray(R, dtype=np.float64) * FWHM_PER_SIGMA)


def trapezoid_weights(x):
    h = np.empty_like(x)
    h[1:-1] = (x[2:] - x[:-2]) / 2
    h[0] = (x[1] - x[0]) / 2
    h[-1] = (x[-1] - x[-2]) / 2
    return h


def response(e0, e1, x, sigma):
    """the Gaussian of width sigma around each x integrated from e0 to e1"""
    s2 = sigma * np.sqrt(2.0)
    a, b = (e0 - x) / s2, (e1 - x) / s2
    r = np.empty_like(x)
    up = a > 0
    dn = ~up & (b < 0)
    mid = ~up & ~dn
    r[up] = 0.5 * (erfc(a[up]) - erfc(b[up]))
    r[dn] = 0.5 * (erfc(-b[dn]) - erfc(-a[dn]))
    r[mid] = 0.5 * (erf(b[mid]) - erf(a[mid]))
    return r


def windows(x, edges, sigma):
    """-> (i0, i1, covered) per pixel: the points with lo <= x <= hi are x[i0:i1]"""
    lo, hi = edges[:-1] - 8 * sigma, edges[1:] + 8 * sigma
    covered = (lo >= x[0]) & (hi <= x[-1])
    return np.searchsorted(x, lo, "left"), np.searchsorted(x, hi, "right"), covered


def observe(lambdas, flux, edges, sigma, doppler=1.0, reference=None, truncated=True):
    """-> out (n_pix,).  truncated=False: every pixel sums over the whole grid (the NaN rule stays the window's)."""
    lam, f = np.asarray(lambdas, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (edges.size - 1,))
    g = None if reference is None else np.asarray(reference, dtype=np.float64)
    x = lam * doppler
    h = trapezoid_weights(x)
    i0, i1, covered = windows(x, edges, sigma)
    out = np.full(edges.size - 1, np.nan)
    for j in np.flatnonzero(covered):
        sl = slice(i0[j], i1[j]) if truncated else slice(0, x.size)
        w = response(edges[j], edges[j + 1], x[sl], sigma[j]) * h[sl]
        den = w.sum() if g is None else (w * g[sl]).sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            out[j] = (w * f[sl]).sum() / den
    return out


def window_lengths(lambdas, edges, sigma, doppler=1.0):
    x = np.asarray(lambdas, dtype=np.float64) * doppler
    i0, i1, covered = windows(x, np.asarray(edges, dtype=np.float64), np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(edges) - 1,)))
    return np.where(covered, i1 - i0, 0)


def clear_of_grid_ends(lambdas, edges, sigma, doppler=1.0, margin=1e-9):
    """no lo_j or hi_j within `margin` Angstrom of a grid end: the NaN pattern cannot hinge on one rounding"""
    x0, x1 = lambdas[0] * doppler, lambdas[-1] * doppler
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(edges) - 1,))
    lo, hi = np.asarray(edges)[:-1] - 8 * sigma, np.asarray(edges)[1:] + 8 * sigma
    return bool(np.all(np.abs(lo - x0) > margin) and np.all(np.abs(hi - x1) > margin))
