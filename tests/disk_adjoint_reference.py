"""The transpose and the V-derivative of the disk integration as include/stardis_hip.h defines them (sdx_disk_integrate_adjoint_dev,
sdx_disk_integrate_deriv_dev) restated in numpy, in np.longdouble from the fp64 inputs, on tests/disk_integration_reference.row: what
tests/test_gpu_disk_adjoint.py holds the device against, pinned by tests/test_disk_adjoint_cpu.py (Richardson quotients of the
restatement's own forward, the dot identity).

Same definition, other arithmetic (disk_integration_reference's notes apply): reach = lam_i ((V / c) scale) is the PARAMETER of a
(point, ring) and is taken as the definition rounds it, in fp64; everything behind it is longdouble.

The derivative, for ring r, point i, reach > 0, over the cells g = [j, j + 1] of the row:
    dnum = sum_g (M1_g / Delta_g) (I[j+1] - I[j]) - e_hi I[n-1] + e_lo I[0],     dden = -e_hi + e_lo,
    e_hi = y_hi K(y_hi) where lam_i + reach > lam[n-1] (y_hi = (lam[n-1] - lam_i) / reach), e_lo = y_lo K(y_lo) where lam_i - reach < lam[0],
    K(y) = 1 / (pi sqrt((1 - y)(1 + y))),     dA = (dnum - A dden) / den,     dout = sum_r w_r dA_r.
"""
import numpy as np

import disk_integration_reference as D

LD = D.LD


def end_terms(lam, i, reach):
    """-> (e_lo, e_hi, margin): y K(y) at the two ends of the grid seen from point i, 0 where the window does not reach the end;
    margin = the smallest 1 - |y_end| over the ends that are reached (inf: none), what the derivative's contract is stated in"""
    reach = LD(reach)
    e, margin = [LD(0), LD(0)], np.inf
    for k, end in enumerate((0, lam.size - 1)):
        if end == i:
            continue
        dl = lam[end] - lam[i]
        u = (reach - abs(dl)) / reach
        if not u > 0:
            continue
        y = dl / reach
        e[k] = y / (D.pi64() * np.sqrt(u * (1 + abs(y))))
        margin = min(margin, float(u))
    return e[0], e[1], margin


def reaches(lambdas, V, scale, exact=False):
    """reach[i] as the definition rounds it (fp64, disk_integration_reference.reaches), or with `exact` unrounded in longdouble from a
    longdouble V: the operator as a smooth function of V, which is what a difference quotient in V needs (the fp64 rounding of the
    reach moves the forward result by 1e-16 relative, 1e-13 of a quotient at a step of 1e-3)"""
    if not exact:
        return D.reaches(lambdas, V, scale)
    return np.asarray(lambdas, dtype=np.float64).astype(LD) * ((LD(V) / LD(np.float64(D.C_KMS))) * LD(np.float64(scale)))


def ring_forward(lambdas, spectrum, V, scale, points=None, exact=False):
    """A_r over `points` in longdouble, as disk_integration_reference.ring_average, with the reach of reaches(..., exact)"""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    f = np.asarray(spectrum, dtype=np.float64).astype(LD)
    points = range(lam.size) if points is None else points
    reach = reaches(lambdas, V, scale, exact)
    A = np.empty(len(points), dtype=LD)
    for k, i in enumerate(points):
        if not reach[i] > 0:
            A[k] = f[i]
            continue
        w = D.row(lam, i, reach[i])
        A[k] = (w.W * f[w.j0:w.j0 + w.W.size]).sum() / w.den
    return A


def disk_forward(lambdas, intensities, ring_scale, ring_weights, V, points=None, exact=False):
    I = np.asarray(intensities, dtype=np.float64)
    return sum(LD(np.float64(w)) * ring_forward(lambdas, I[r], V, s, points, exact)
               for r, (s, w) in enumerate(zip(np.asarray(ring_scale, dtype=np.float64), np.asarray(ring_weights, dtype=np.float64))))


def ring_derivative(lambdas, spectrum, V, scale, points=None, exact=False):
    """-> (dA, terms, margin) over `points` (default: all), longdouble: dA_r[i] = d A_r[i] / d ln V; terms[i] = the sum of the absolute
    terms of dA (what a tolerance is taken against); margin[i] = 1 - |y_end| of the nearest truncated end (inf: not truncated)"""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    f = np.asarray(spectrum, dtype=np.float64).astype(LD)
    points = range(lam.size) if points is None else points
    reach = reaches(lambdas, V, scale, exact)
    dA, T, margin = np.zeros(len(points), dtype=LD), np.zeros(len(points), dtype=LD), np.full(len(points), np.inf)
    for k, i in enumerate(points):
        if not reach[i] > 0:
            continue
        w = D.row(lam, i, reach[i])
        j0, m = w.j0, w.W.size
        y = (lam[j0:j0 + m] - lam[i]) / LD(reach[i])
        y[i - j0] = 0
        c = np.clip(y, -1, 1)
        _, M1 = D.cell_moments(c[:-1], c[1:])
        delta = (lam[j0 + 1:j0 + m] - lam[j0:j0 + m - 1]) / LD(reach[i])
        fj = f[j0:j0 + m]
        t = M1 / delta * (fj[1:] - fj[:-1])
        e_lo, e_hi, margin[k] = end_terms(lam, i, reach[i])
        A = (w.W * fj).sum() / w.den
        dnum = t.sum() - e_hi * f[-1] + e_lo * f[0]
        dden = e_lo - e_hi
        dA[k] = (dnum - A * dden) / w.den
        T[k] = (np.abs(t).sum() + abs(e_hi * f[-1]) + abs(e_lo * f[0]) + abs(A) * (abs(e_lo) + abs(e_hi))) / w.den
    return dA, T, margin


def disk_derivative(lambdas, intensities, ring_scale, ring_weights, V, points=None, exact=False):
    """-> (dout_lnv, terms, margin) in longdouble over `points`: sum_r w_r dA_r[i], the sum of its absolute terms, and the smallest
    1 - |y_end| over the truncated (point, ring) pairs per point"""
    I = np.asarray(intensities, dtype=np.float64)
    n = np.asarray(lambdas).size if points is None else len(points)
    out, terms, margin = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.full(n, np.inf)
    for r, (s, w) in enumerate(zip(np.asarray(ring_scale, dtype=np.float64), np.asarray(ring_weights, dtype=np.float64))):
        dA, T, mg = ring_derivative(lambdas, I[r], V, s, points, exact)
        out += LD(w) * dA
        terms += abs(LD(w)) * T
        margin = np.minimum(margin, mg)
    return out, terms, margin


def adjoint_rows(lambdas, u, ring_scale, ring_weights, V, nus=None, points=None):
    """-> (W, terms) in longdouble, each (n_rings, n): W[r][j] = w_r sum_i (u_i / den_r(i)) (weight of node j in point i's row for ring
    r), times nus[j] / lam[j] with nus; terms: the same sum of absolute values (what a tolerance is taken against).  A (point, ring)
    whose reach is not positive passes w_r u_i through.  points: the i at which u is not zero (default: all are visited)."""
    lam64 = np.asarray(lambdas, dtype=np.float64)
    lam, uu = lam64.astype(LD), np.asarray(u, dtype=np.float64).astype(LD)
    scale, wts = np.asarray(ring_scale, dtype=np.float64), np.asarray(ring_weights, dtype=np.float64)
    W, T = np.zeros((scale.size, lam.size), dtype=LD), np.zeros((scale.size, lam.size), dtype=LD)
    for r in range(scale.size):
        reach = D.reaches(lam64, V, scale[r])
        for i in (range(lam.size) if points is None else points):
            if not reach[i] > 0:
                W[r, i] += uu[i]
                T[r, i] += abs(uu[i])
                continue
            w = D.row(lam, i, reach[i])
            W[r, w.j0:w.j0 + w.W.size] += uu[i] / w.den * w.W
            T[r, w.j0:w.j0 + w.W.size] += abs(uu[i] / w.den) * np.abs(w.W)
        W[r] *= LD(wts[r])
        T[r] *= abs(LD(wts[r]))
    if nus is not None:
        factor = np.asarray(nus, dtype=np.float64).astype(LD) / lam
        W, T = W * factor, T * np.abs(factor)
    return W, T


def richardson_lnv(forward, V, h=2.0 ** -10):
    """d forward / d ln V = V d forward / dV at V from the central quotients in V at the steps V h, V h / 2 and V h / 4, extrapolated once
    (error h^4 where forward is smooth) -> (value, unsure): the value from the two finer steps and its distance from the one of the two
    coarser steps, which errs 16 times as much where forward is smooth and which shows a kink inside the steps where it is not: the
    value's own uncertainty.  Choose V and h so that V (1 +- h / 4) is exact in the format forward takes."""
    def quotient(step):
        d = V * step
        return (forward(V + d) - forward(V - d)) / (2 * LD(d)) * LD(V)

    q1, q2, q3 = quotient(h), quotient(h / 2), quotient(h / 4)
    coarse, fine = (4 * q2 - q1) / 3, (4 * q3 - q2) / 3
    return fine, np.abs(fine - coarse)
