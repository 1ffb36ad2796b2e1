"""The adjoint of the instrument model of include/stardis_hip.h (sdx_observe_adjoint_dev) restated in numpy on top of
tests/observe_reference.py (windows, response, trapezoid_weights), one window slice per pixel: what tests/test_gpu_observe_adjoint.py
holds the device against and tests/test_observe_adjoint_cpu.py pins by its own properties.  Same definition, same operations per term;
only the order of the sums differs."""
import numpy as np

import observe_reference as oref


def pixel_rows(lambdas, edges, sigma, doppler=1.0):
    """-> x, [(j, slice, w_ij over the slice) for every COVERED pixel j]"""
    lam, edges = np.asarray(lambdas, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (edges.size - 1,))
    x = lam * doppler
    h = oref.trapezoid_weights(x)
    i0, i1, covered = oref.windows(x, edges, sigma)
    return x, [(j, slice(i0[j], i1[j]), oref.response(edges[j], edges[j + 1], x[i0[j]:i1[j]], sigma[j]) * h[i0[j]:i1[j]]) for j in np.flatnonzero(covered)]


def adjoint(lambdas, c, edges, sigma, doppler=1.0, flux=None, reference=None, nus=None):
    """-> (w_flux, w_ref, scale, scale_ref): the two outputs and, per point, the sums of the absolute values of their terms — what a
    bound on an error is taken against (c is signed; the sums cancel).  w_ref and scale_ref are None without a reference."""
    lam, c = np.asarray(lambdas, dtype=np.float64), np.asarray(c, dtype=np.float64)
    g = None if reference is None else np.asarray(reference, dtype=np.float64)
    f = None if flux is None else np.asarray(flux, dtype=np.float64)
    _, rows = pixel_rows(lam, edges, sigma, doppler)
    w_flux, scale = np.zeros(lam.size), np.zeros(lam.size)
    w_ref = None if g is None else np.zeros(lam.size)
    scale_ref = None if g is None else np.zeros(lam.size)
    for j, sl, w in rows:
        den = w.sum() if g is None else (w * g[sl]).sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            a = c[j] / den
        w_flux[sl] += w * a
        scale[sl] += np.abs(w * a)
        if g is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                b = -((w * f[sl]).sum() / den) * a
            w_ref[sl] += w * b
            scale_ref[sl] += np.abs(w * b)
    if nus is not None:
        k = np.asarray(nus, dtype=np.float64) / lam
        w_flux, scale = w_flux * k, scale * np.abs(k)
        if g is not None:
            w_ref, scale_ref = w_ref * k, scale_ref * np.abs(k)
    return w_flux, w_ref, scale, scale_ref


def pixel_sets(lambdas, edges, sigma, doppler=1.0):
    """-> member (n_pix, n) bool: covered pixel j holds point i — for the tests' own assertions about their inputs"""
    lam = np.asarray(lambdas, dtype=np.float64)
    x, rows = pixel_rows(lam, edges, sigma, doppler)
    member = np.zeros((len(edges) - 1, lam.size), dtype=bool)
    for j, sl, _ in rows:
        member[j, sl] = True
    return member


def noncontiguous_points(member):
    """how many points lie in a set of pixels that is not one run of consecutive pixels"""
    count = 0
    for i in range(member.shape[1]):
        js = np.flatnonzero(member[:, i])
        count += bool(js.size and js[-1] - js[0] + 1 != js.size)
    return count


def dot_terms(lambdas, c, flux, edges, sigma, doppler=1.0, reference=None):
    """sum_ij |c_j w_ij f_i / den_j| over the covered pixels: what a bound on <observe(f), c> - <f, adjoint(c)> is taken against"""
    lam, c, f = (np.asarray(a, dtype=np.float64) for a in (lambdas, c, flux))
    g = None if reference is None else np.asarray(reference, dtype=np.float64)
    total = 0.0
    for j, sl, w in pixel_rows(lam, edges, sigma, doppler)[1]:
        den = w.sum() if g is None else (w * g[sl]).sum()
        total += float(np.sum(np.abs(c[j] * w * f[sl] / den)))
    return total


def nonmonotone_input():
    """600 irregular points on 6500 - 6600 A, 37 random pixels in 6520 - 6580 A whose sigma varies by two orders of magnitude from pixel to
    pixel, v = 30 km/s: lo_j and hi_j both fail to ascend, and some points lie in a set of pixels with gaps."""
    rng = np.random.default_rng(0)
    lam = np.sort(rng.uniform(6500.0, 6600.0, 600))
    edges = np.sort(rng.uniform(6520.0, 6580.0, 38))
    sigma = np.clip(0.05 * np.exp(2.5 * rng.standard_normal(37)), 0.02, 2.0)
    return lam, edges, sigma, 30.0
