"""The tangent of the instrument model (include/stardis_hip.h, sdx_observe_tangent_dev, sdx_rotate_tangent_dev) restated in numpy:
observe_reference's own windows and weights (fp64, scipy's erf / erfc), the two partials of the pixel response from their closed forms
in np.longdouble, every sum in np.longdouble.  What tests/test_gpu_observe_tangent.py holds the device against and
tests/test_observe_tangent_cpu.py pins against 50-digit mpmath and by difference quotients of observe_reference itself.

The closed forms, with a' = (e0 - x) / sigma, b' = (e1 - x) / sigma and phi the unit normal density:
    dr/dx = (phi(a') - phi(b')) / sigma,      dr/d ln sigma = a' phi(a') - b' phi(b').
phi(a') - phi(b') is formed from the nearer edge and expm1 of -(|a'^2 - b'^2|) / 2, a'^2 - b'^2 = (a' - b')(a' + b'), and
dr/d ln sigma = near (phi(a') - phi(b')) + (a' - b') phi(far): the product rule over the two differences, each of which keeps its
relative accuracy for a pixel much narrower than sigma and with both edges in one tail.  Their sum cancels only at the genuine zero of
dr/d ln sigma (t phi(t) is stationary at |t| = 1, so a narrow pixel around |t| = 1 has none), where the condition number of the
derivative itself is unbounded; PRODUCT_RULE_SCALE is therefore what an error of dr/d ln sigma is taken against."""
import mpmath
import numpy as np

import observe_reference as oref
import rotation_reference as rref
from observe_reference import C_KMS, FLUX_TOL, SUM_TOL  # noqa: F401

LD = np.longdouble
RESTATEMENT_TOL = 1e-17  # the longdouble closed forms against 50 digits: exponents up to 32 at an epsilon of 5.4e-20, a few roundings


def _pi_ld():
    return LD(4) * np.arctan(LD(1))


def response_grad(e0, e1, x, sigma):
    """-> (dr/dx, dr/d ln sigma) in longdouble for arrays of (e0, e1, x, sigma)"""
    e0, e1, x, sigma = (np.asarray(v, dtype=np.float64).astype(LD) for v in np.broadcast_arrays(e0, e1, x, sigma))
    a, b = (e0 - x) / sigma, (e1 - x) / sigma
    m, p = (e0 - e1) / sigma, ((e0 - x) + (e1 - x)) / sigma  # a' - b', a' + b'
    first = p >= 0  # |a'| <= |b'|
    near, far = np.where(first, a, b), np.where(first, b, a)
    norm = np.sqrt(2 * _pi_ld())
    phi_near, phi_far = np.exp(-near * near / 2) / norm, np.exp(-far * far / 2) / norm
    g = phi_near * np.expm1(-np.abs(m * p) / 2)  # phi(far) - phi(near)
    G = np.where(first, -g, g)                   # phi(a') - phi(b')
    return G / sigma, near * G + m * phi_far


def mp_phi(t):
    return mpmath.exp(-t * t / 2) / mpmath.sqrt(2 * mpmath.pi)


def mp_response(a, b):
    """(r, sigma dr/dx, dr/d ln sigma, PRODUCT_RULE_SCALE) at 50 digits for the edges a', b' (floats) of a unit Gaussian around 0"""
    a, b = mpmath.mpf(float(a)), mpmath.mpf(float(b))
    r = (mpmath.erfc(a / mpmath.sqrt(2)) - mpmath.erfc(b / mpmath.sqrt(2))) / 2 if a > 0 else (
        (mpmath.erfc(-b / mpmath.sqrt(2)) - mpmath.erfc(-a / mpmath.sqrt(2))) / 2 if b < 0 else (mpmath.erf(b / mpmath.sqrt(2)) - mpmath.erf(a / mpmath.sqrt(2))) / 2)
    G = mp_phi(a) - mp_phi(b)
    near, far = (a, b) if a + b >= 0 else (b, a)
    return r, G, a * mp_phi(a) - b * mp_phi(b), abs(near * G) + abs((a - b) * mp_phi(far))


def response_grad_points():
    """-> (a', b'): the points of the response-gradient checks — both tails out to +-8, pixels from 1e-4 sigma to 1e3 sigma wide, x
    exactly on an edge (a' = 0 or b' = 0: the grid holds 0) and at the pixel's centre (a' = -b')"""
    t = np.linspace(-8.0, 8.0, 65)  # (steps of 0.25: 0 and +-1 are on it)
    a, b = [], []
    for width in (1e-4, 1e-2, 0.3, 1.0, 3.0, 10.0, 1e3):
        a += [t, t - width, -np.full(1, width / 2)]
        b += [t + width, t, np.full(1, width / 2)]
    a, b = np.concatenate(a), np.concatenate(b)
    return a, b


def velocity_factor(doppler):
    """d ln D / dv per km/s for D = sqrt((1 + beta) / (1 - beta)): (D^2 + 1)^2 / (4 D^2 c)"""
    D2 = LD(doppler) * LD(doppler)
    return (D2 + 1) ** 2 / (4 * D2 * LD(C_KMS))


def observe_tangent(lambdas, flux, edges, sigma, doppler=1.0, reference=None, dflux=None, dreference=None):
    """-> dict of (n_pix,) longdouble arrays, NaN where the grid does not cover the pixel's window:
         out, v_rad (per km/s), lsf (per ln kappa), flux (with dflux),
         and for each of the last three `<name>_terms`: the sum of the ABSOLUTE terms of its quotient,
         (sum |d w F| + |out| sum |d w g|) / |den| — what a tolerance is taken against, so that cancellation is not charged."""
    lam, f = np.asarray(lambdas, dtype=np.float64), np.asarray(flux, dtype=np.float64).astype(LD)
    edges = np.asarray(edges, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (edges.size - 1,))
    g = None if reference is None else np.asarray(reference, dtype=np.float64).astype(LD)
    df = None if dflux is None else np.asarray(dflux, dtype=np.float64).astype(LD)
    dg = None if dreference is None else np.asarray(dreference, dtype=np.float64).astype(LD)
    x = lam * doppler
    h = oref.trapezoid_weights(x)
    i0, i1, covered = oref.windows(x, edges, sigma)
    n_pix = edges.size - 1
    names = ("out", "v_rad", "lsf", "flux", "v_rad_terms", "lsf_terms", "flux_terms")
    res = {k: np.full(n_pix, np.nan, dtype=LD) for k in names}
    per_kms = velocity_factor(doppler)
    for j in np.flatnonzero(covered):
        sl = slice(i0[j], i1[j])
        r = oref.response(edges[j], edges[j + 1], x[sl], sigma[j])
        w = (r * h[sl]).astype(LD)  # observe_reference's own weights
        rx, rs = response_grad(edges[j], edges[j + 1], x[sl], sigma[j])
        wD, wS = (x[sl].astype(LD) * rx + r.astype(LD)) * h[sl].astype(LD), rs * h[sl].astype(LD)
        gj = np.ones(w.size, dtype=LD) if g is None else g[sl]
        den = (w * gj).sum()
        out = (w * f[sl]).sum() / den
        res["out"][j] = out
        for name, dw, scale in (("v_rad", wD, per_kms), ("lsf", wS, LD(1))):
            res[name][j] = ((dw * f[sl]).sum() - out * (dw * gj).sum()) / den * scale
            res[name + "_terms"][j] = (np.abs(dw * f[sl]).sum() + abs(out) * np.abs(dw * gj).sum()) / abs(den) * scale
        if df is not None:
            second = LD(0) if dg is None else (w * dg[sl]).sum()
            res["flux"][j] = ((w * df[sl]).sum() - out * second) / den
            res["flux_terms"][j] = (np.abs(w * df[sl]).sum() + abs(out) * (LD(0) if dg is None else np.abs(w * dg[sl]).sum())) / abs(den)
    if df is None:
        del res["flux"], res["flux_terms"]
    return res


def rotate_eps_rows(lambdas, V, eps):
    """yields (i, j, w, dw) over rotation_reference's rows: w_ij as point_rows gives it and dw_ij = (-2 sqrt(q) + (pi / 2) q) h_j"""
    lam, reach, i0, i1 = rref.windows(lambdas, V)
    h = rref.trapezoid_weights(lam)
    c_sqrt, c_q, half_pi = 2 * (1 - LD(eps)), LD(np.float64(np.pi / 2)) * LD(eps), LD(np.float64(np.pi / 2))
    for i in range(lam.size):
        j = np.arange(i0[i], i1[i])
        y = (lam[j] - lam[i]) / reach[i]
        q = 1 - y * y
        keep = (q > 0) | (j == i)
        j, q = j[keep], np.where(j == i, LD(1), q)[keep]
        root = np.sqrt(q)
        yield i, j, (c_sqrt * root + c_q * q) * h[j], (-2 * root + half_pi * q) * h[j]


def rotate_tangent(lambdas, flux, V, eps, reference=None):
    """-> (dout_eps, dout_eps_reference, scale, scale_reference) in longdouble: d rotate / d eps and, per point, max |F| over the
    included points (rotation_reference's ROT_TOL is taken against it).  !(V > 0): zeros."""
    f = np.asarray(flux, dtype=np.float64).astype(LD)
    g = None if reference is None else np.asarray(reference, dtype=np.float64).astype(LD)
    if not V > 0:
        return np.zeros_like(f), None if g is None else np.zeros_like(f), np.abs(f), None if g is None else np.abs(g)
    d, scale = np.empty_like(f), np.empty_like(f)
    d_ref, scale_ref = (None, None) if g is None else (np.empty_like(f), np.empty_like(f))
    for i, j, w, dw in rotate_eps_rows(lambdas, V, eps):
        den, dden = w.sum(), dw.sum()
        d[i], scale[i] = ((dw * f[j]).sum() - (w * f[j]).sum() / den * dden) / den, np.abs(f[j]).max()
        if g is not None:
            d_ref[i], scale_ref[i] = ((dw * g[j]).sum() - (w * g[j]).sum() / den * dden) / den, np.abs(g[j]).max()
    return d, d_ref, scale, scale_ref
