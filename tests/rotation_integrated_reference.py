"""The cell-integrated rotation profile as include/stardis_hip.h defines it (sdx_rotate_integrated_dev, sdx_rotate_integrated_adjoint_dev)
restated in numpy, in np.longdouble from the fp64 inputs, one row per point: what tests/test_gpu_rotation_integrated.py holds the device
against and tests/test_rotation_integrated_cpu.py pins against 50-digit mpmath quadrature and by its own properties.

Same definition, other arithmetic: the moments of a cell are plain differences of the antiderivatives
    int sqrt(q) = (y sqrt(q) + asin y) / 2,   int q = y - y^3 / 3,   int y sqrt(q) = -q^(3/2) / 3,   int y q = y^2 / 2 - y^4 / 4,   q = 1 - y^2,
which lose |y| / d of a cell d wide — harmless at the longer format's 5.4e-20 for the cells a window holds (the device, in fp64, forms
them without differences).  There is no profile edge to stay clear of: a node on the edge closes a cell of zero length.

beta = V / c and reach_i = lam_i beta are the row's PARAMETERS and are taken as the definition rounds them, in fp64 (reaches()), like the
constant pi / 2; everything behind them is longdouble.  It matters in one place: the end term y K(y) of a truncated window ends in
sqrt(1 - |y|), so where an END node of the grid sits on the profile's edge, a reach that differs by an ulp would move it by sqrt(ulp) =
1e-8.  1 - |y| is formed as (reach - |lam_end - lam_i|) / reach, as the device forms it."""
import functools

import mpmath
import numpy as np

from observe_reference import SUM_TOL  # noqa: F401  (identities between reordered sums: 1e-12 of the sum of the absolute terms)
from rotation_reference import C_KMS, LD, ROT_TOL  # noqa: F401

DERIV_TOL = 1e-10  # of the sum of the absolute terms: the project's tolerance for the tangents (observe_reference.FLUX_TOL)
# sdx_rotate_moments against 50 digits, relative to |M|: observe_tangent_reference's RESTATEMENT_TOL convention — a closed form of a few
# roundings against mpmath, 1e-17 at the longdouble epsilon 2^-64 — carried to the device's format: the same count of roundings at 2^-53.
MOMENT_TOL = 1e-17 * 2.0 ** 11


def half_pi():
    return LD(np.float64(np.pi / 2))  # (the fp64 constant, as the device has it)


def reaches(lambdas, V):
    """-> reach_i = lam_i (V / c) as the definition rounds it: two fp64 operations"""
    return np.asarray(lambdas, dtype=np.float64) * (np.float64(V) / np.float64(C_KMS))


def antiderivatives(y):
    """-> (S0, Q0, S1, Q1) at y in [-1, 1], longdouble"""
    q = np.maximum(1 - y * y, 0)
    root = np.sqrt(q)
    return (y * root + np.arcsin(y)) / 2, y - y ** 3 / 3, -q * root / 3, y * y / 2 - y ** 4 / 4


def moments(ya, yb):
    """-> (S0, Q0, S1, Q1): the four integrals over [ya, yb] clamped to [-1, 1], longdouble (zeros for an empty cell)"""
    a, b = (np.clip(np.asarray(v, dtype=np.float64).astype(LD), -1, 1) for v in (ya, yb))
    lo, hi = antiderivatives(a), antiderivatives(b)
    return tuple(np.where(b > a, above - below, 0) for below, above in zip(lo, hi))


def mp_moments(ya, yb, eps):
    """(M0, M1) at 50 digits by quadrature of K and y K over [ya, yb] clamped, K = 2 (1 - eps) sqrt(q) + (pi / 2) eps q with the fp64 pi / 2"""
    a, b = (mpmath.mpf(min(max(float(v), -1.0), 1.0)) for v in (ya, yb))
    if not b > a:
        return mpmath.mpf(0), mpmath.mpf(0)
    e, hp = mpmath.mpf(float(eps)), mpmath.mpf(float(np.pi / 2))
    K = lambda y: 2 * (1 - e) * mpmath.sqrt(max(1 - y * y, 0)) + hp * e * (1 - y * y)  # noqa: E731
    pts = sorted({a, b} | {mpmath.mpf(t) for t in (-1, 0, 1) if a < t < b})
    return mpmath.quad(K, pts), mpmath.quad(lambda y: y * K(y), pts)


class Row:
    """point i's row: nodes j0 .. j0 + W.size - 1 with the weights W (forward), dW (d / d eps), T (d / d ln V, end terms included); den =
    sum W, dden = sum dW, tsum = sum T; t: M1 / Delta per cell (the cells that count: first .. first + t.size - 1); e0, e1 the end terms"""


def rows(lambdas, V, eps):
    """yields a Row per point, in longdouble (V > 0)"""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    n = lam.size
    all_reaches = reaches(lambdas, V).astype(LD)
    c_sqrt, c_q = 2 * (1 - LD(eps)), half_pi() * LD(eps)
    for i in range(n):
        reach = all_reaches[i]
        g0 = max(int(np.searchsorted(lam, lam[i] - reach, "left")) - 1, 0)
        g1 = min(int(np.searchsorted(lam, lam[i] + reach, "right")), n - 1)
        y = (lam[g0:g1 + 1] - lam[i]) / reach
        y[i - g0] = 0
        c = np.clip(y, -1, 1)
        S0, Q0, S1, Q1 = (hi - lo for lo, hi in zip(antiderivatives(c[:-1]), antiderivatives(c[1:])))
        counts = c[1:] > c[:-1]
        delta = (lam[g0 + 1:g1 + 1] - lam[g0:g1]) / reach
        row = Row()
        row.i, row.j0 = i, g0
        for name, a, b in (("W", c_sqrt, c_q), ("dW", LD(-2), half_pi())):
            M0, M1 = np.where(counts, a * S0 + b * Q0, 0), np.where(counts, a * S1 + b * Q1, 0)
            r = (M1 - y[:-1] * M0) / delta
            w = np.zeros(y.size, dtype=LD)
            w[1:] += r
            w[:-1] += M0 - r
            setattr(row, name, w)
            if name == "W":
                row.t = M1 / delta
        row.T = np.zeros(y.size, dtype=LD)
        row.T[1:] += row.t
        row.T[:-1] -= row.t

        def end_term(lam_end):
            u = (reach - abs(lam_end - lam[i])) / reach  # 1 - |y|
            if not u > 0:
                return LD(0)
            q = u * (1 + abs(lam_end - lam[i]) / reach)
            return (lam_end - lam[i]) / reach * (c_sqrt * np.sqrt(q) + c_q * q)

        row.e0 = end_term(lam[0]) if i != 0 else LD(0)
        row.e1 = end_term(lam[n - 1]) if i != n - 1 else LD(0)
        row.ends = (g0 == 0 and row.e0 != 0, g1 == n - 1 and row.e1 != 0)
        if row.e0 != 0:
            row.T[0] += row.e0  # (then g0 = 0: the window reaches the grid's first node)
        if row.e1 != 0:
            row.T[-1] -= row.e1
        row.den, row.dden, row.tsum = row.W.sum(), row.dW.sum(), row.e0 - row.e1
        row.truncated = bool(lam[i] - reach < lam[0] or lam[i] + reach > lam[n - 1])
        yield row


def rotate(lambdas, flux, V, eps, reference=None):
    """-> dict of longdouble arrays over the points, for `flux` and (keys ending in _reference) for `reference`:
         out, dlnv (d out / d ln V), deps (d out / d eps), scale (max |F| over the row's nodes: what ROT_TOL is taken against),
         dlnv_terms, deps_terms (the sums of the absolute terms of the two quotients as the operator forms them: what DERIV_TOL is
         taken against).  !(V > 0): a copy, zeros, and terms of |F| so that an allowance stays positive."""
    series = {"": np.asarray(flux, dtype=np.float64).astype(LD)}
    if reference is not None:
        series["_reference"] = np.asarray(reference, dtype=np.float64).astype(LD)
    names = ("out", "dlnv", "deps", "scale", "dlnv_terms", "deps_terms")
    res = {k + tag: np.zeros_like(f) for tag, f in series.items() for k in names}
    if not V > 0:
        for tag, f in series.items():
            res["out" + tag] = f.copy()
            for k in ("scale", "dlnv_terms", "deps_terms"):
                res[k + tag] = np.abs(f)
        return res
    for row in rows(lambdas, V, eps):
        i, sl = row.i, slice(row.j0, row.j0 + row.W.size)
        for tag, f in series.items():
            fj = f[sl]
            out = (row.W * fj).sum() / row.den
            res["out" + tag][i], res["scale" + tag][i] = out, np.abs(fj).max()
            res["dlnv" + tag][i] = ((row.T * fj).sum() - out * row.tsum) / row.den
            res["deps" + tag][i] = ((row.dW * fj).sum() - out * row.dden) / row.den
            cells = np.abs(row.t * np.diff(fj)).sum() + abs(row.e0 * f[0]) + abs(row.e1 * f[-1])
            res["dlnv_terms" + tag][i] = (cells + abs(out) * (abs(row.e0) + abs(row.e1))) / row.den
            res["deps_terms" + tag][i] = (np.abs(row.dW * fj).sum() + abs(out) * np.abs(row.dW).sum()) / row.den
    return res


def adjoint(lambdas, u, V, eps, u_reference=None, nus=None):
    """-> (w, w_reference, scale, scale_reference) in longdouble: the transpose applied to u (and u_reference) and, per node j, the sum
    of its peak terms K(0) h_j / reach_i |a_i| over the rows that hold j (h_j: half the two cells around j) — what ROT_TOL is taken
    against, as rotation_reference.adjoint's scale is."""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    us = [np.asarray(a, dtype=np.float64).astype(LD) for a in (u, u_reference) if a is not None]
    ws, scales = [np.zeros_like(lam) for _ in us], [np.zeros_like(lam) for _ in us]
    if not V > 0:
        ws, scales = [a.copy() for a in us], [np.abs(a) for a in us]
    else:
        h = np.empty_like(lam)
        h[1:-1], h[0], h[-1] = (lam[2:] - lam[:-2]) / 2, (lam[1] - lam[0]) / 2, (lam[-1] - lam[-2]) / 2
        peak = 2 * (1 - LD(eps)) + half_pi() * LD(eps)
        reach = reaches(lambdas, V).astype(LD)
        for row in rows(lambdas, V, eps):
            sl = slice(row.j0, row.j0 + row.W.size)
            for a, out, scale in zip(us, ws, scales):
                out[sl] += row.W * (a[row.i] / row.den)
                scale[sl] += peak * h[sl] / reach[row.i] * np.abs(a[row.i] / row.den)
    if nus is not None:
        k = np.asarray(nus, dtype=np.float64).astype(LD) / lam
        ws, scales = [a * k for a in ws], [a * np.abs(k) for a in scales]
    return ws[0], ws[1] if len(us) > 1 else None, scales[0], scales[1] if len(us) > 1 else None


def dot_terms(lambdas, u, flux, V, eps):
    """sum_ij |u_i W_ij f_j / den_i|: what a bound on <rotate(f), u> - <f, adjoint(u)> is taken against"""
    u, f = (np.asarray(a, dtype=np.float64).astype(LD) for a in (u, flux))
    if not V > 0:
        return float(np.sum(np.abs(u * f)))
    return float(sum(np.sum(np.abs(u[r.i] * r.W * f[r.j0:r.j0 + r.W.size] / r.den)) for r in rows(lambdas, V, eps)))


def richardson(forward, V, h):
    """the Richardson value (4 Q(h / 2) - Q(h)) / 3 of the central quotients Q(s) = (F(V e^s) - F(V e^-s)) / (2 s) of d F / d ln V"""
    Q = lambda s: (forward(V * np.exp(s)) - forward(V * np.exp(-s))) / (2 * s)  # noqa: E731
    return (4 * Q(h / 2) - Q(h)) / 3


@functools.lru_cache(maxsize=None)
def _gap(lam_bytes, flux_bytes, V, eps, h):
    lam, f = np.frombuffer(lam_bytes), np.frombuffer(flux_bytes)
    exact = rotate(lam, f, V, eps)["dlnv"]
    quotient = richardson(lambda v: rotate(lam, f, float(v), eps)["out"], V, h)
    return float(np.max(np.abs(quotient - exact))), float(np.max(np.abs(exact)))


def quotient_gap(lambdas, flux, V, eps, h):
    """-> (gap, largest |d out / d ln V|): the restatement's own largest distance, over the points, between the Richardson value at step
    h of its forward and its analytic derivative.  d out / dV is continuous but only Hoelder-1/2 where a node crosses a profile edge, so a
    quotient does not converge like h^4 there; this gap is the yardstick for the same quotient of the device's forward."""
    lam, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (lambdas, flux))
    return _gap(lam.tobytes(), f.tobytes(), float(V), float(eps), float(h))
