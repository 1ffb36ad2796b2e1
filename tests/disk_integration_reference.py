"""Disk integration with rigid rotation as include/stardis_hip.h defines it (sdx_disk_integrate_dev) restated in numpy, in np.longdouble
from the fp64 inputs, one (point, ring) at a time: what tests/test_gpu_disk_integration.py holds the device against and
tests/test_disk_integration_cpu.py pins against 40-digit mpmath closed forms and by its own properties.

Same definition, other arithmetic: M0 of a cell is the plain difference of the antiderivative asin(y) / pi, which loses 1 / d of a
cell d wide — harmless at the longer format's 5.4e-20 for the cells a window holds (the device, in fp64, forms it from one atan2 of the
angle difference).  M1 = (sqrt(q_a) - sqrt(q_b)) / pi, q = 1 - y^2, is NOT taken as that difference: around y = 0 it would lose 1 / (d |y|),
the whole value for a narrow cell at the line centre; it is (b - a)(b + a) / (pi (sqrt(q_a) + sqrt(q_b))), every factor exact or a sum of
non-negative terms.  A node on a ring's edge closes a cell of zero length.

beta = V / c, beta_r = beta ring_scale[r] and reach = lam_i beta_r are the PARAMETERS of a (point, ring) and are taken as the definition
rounds them, in fp64 (reaches()), like the constant pi; everything behind them is longdouble."""
import mpmath
import numpy as np

from rotation_reference import C_KMS, LD, ROT_TOL  # noqa: F401  (ROT_TOL: 1e-11 of the window's scale, the project's tolerance for k_rotate_integrated)

EXTENDED = bool(np.finfo(LD).eps <= 1e-18)  # a host without an extended long double has no restatement to offer: the tests skip


def pi64():
    return LD(np.float64(np.pi))  # (the fp64 constant, as the device has it)


def reaches(lambdas, V, scale):
    """-> reach[i] = lam_i ((V / c) scale) as the definition rounds it: three fp64 operations"""
    return np.asarray(lambdas, dtype=np.float64) * ((np.float64(V) / np.float64(C_KMS)) * np.float64(scale))


def cell_moments(a, b):
    """-> (M0, M1) over [a, b], -1 <= a, b <= 1 in longdouble (zeros where not b > a)"""
    root = lambda y: np.sqrt(np.maximum((1 - y) * (1 + y), 0))  # noqa: E731
    counts = b > a
    m0 = (np.arcsin(b) - np.arcsin(a)) / pi64()
    roots = root(a) + root(b)  # (0 only for the whole interval [-1, 1], whose M1 is 0)
    m1 = (b - a) * (b + a) / (pi64() * np.where(roots > 0, roots, 1))
    return np.where(counts, m0, 0), np.where(counts, m1, 0)


def moments(ya, yb):
    """-> (M0, M1): the two integrals over [ya, yb] clamped to [-1, 1], longdouble (zeros for an empty cell)"""
    a, b = (np.clip(np.asarray(v, dtype=np.float64).astype(LD), -1, 1) for v in (ya, yb))
    return cell_moments(a, b)


def mp_moments(ya, yb):
    """(M0, M1) at 40 digits from the closed forms over [ya, yb] clamped, with the fp64 pi"""
    with mpmath.workdps(40):
        a, b = (mpmath.mpf(min(max(float(v), -1.0), 1.0)) for v in (ya, yb))
        if not b > a:
            return mpmath.mpf(0), mpmath.mpf(0)
        p = mpmath.mpf(float(np.pi))
        return (mpmath.asin(b) - mpmath.asin(a)) / p, (mpmath.sqrt(1 - a * a) - mpmath.sqrt(1 - b * b)) / p


class Row:
    """point i's row for one ring: nodes j0 .. j0 + W.size - 1 with the weights W; den = sum of M0 over the cells that count; m0 the M0 of
    the cells j0 .. j0 + W.size - 2; truncated: the window reaches past an end of the grid"""


def row(lam, i, reach):
    """lam: the grid in longdouble; reach: fp64 as reaches() gives it, > 0"""
    n = lam.size
    reach = LD(reach)
    g0 = max(int(np.searchsorted(lam, lam[i] - reach, "left")) - 1, 0)
    g1 = min(int(np.searchsorted(lam, lam[i] + reach, "right")), n - 1)
    y = (lam[g0:g1 + 1] - lam[i]) / reach
    y[i - g0] = 0
    c = np.clip(y, -1, 1)
    M0, M1 = cell_moments(c[:-1], c[1:])
    delta = (lam[g0 + 1:g1 + 1] - lam[g0:g1]) / reach
    r = (M1 - y[:-1] * M0) / delta
    out = Row()
    out.i, out.j0 = i, g0
    out.W = np.zeros(y.size, dtype=LD)
    out.W[1:] += r
    out.W[:-1] += M0 - r
    out.m0, out.den = M0, M0.sum()
    out.truncated = bool(lam[i] - reach < lam[0] or lam[i] + reach > lam[n - 1])
    return out


def ring_average(lambdas, spectrum, V, scale, points=None):
    """-> (A, window_scale) in longdouble over `points` (default: all): the ring's average A_r[i] and max |I_r| over the row's nodes"""
    lam = np.asarray(lambdas, dtype=np.float64).astype(LD)
    f = np.asarray(spectrum, dtype=np.float64).astype(LD)
    points = range(lam.size) if points is None else points
    reach = reaches(lambdas, V, scale)
    A, S = np.empty(len(points), dtype=LD), np.empty(len(points), dtype=LD)
    for k, i in enumerate(points):
        if not reach[i] > 0:
            A[k], S[k] = f[i], abs(f[i])
            continue
        w = row(lam, i, reach[i])
        fj = f[w.j0:w.j0 + w.W.size]
        A[k], S[k] = (w.W * fj).sum() / w.den, np.abs(fj).max()
    return A, S


def disk_integrate(lambdas, intensities, ring_scale, ring_weights, V, points=None):
    """-> (out, scale) in longdouble over `points`: out[i] = sum_r w_r A_r[i]; scale[i] = sum_r |w_r| max_window |I_r|, what ROT_TOL is
    taken against"""
    I = np.asarray(intensities, dtype=np.float64)
    n = np.asarray(lambdas).size if points is None else len(points)
    out, scale = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for r, (s, w) in enumerate(zip(np.asarray(ring_scale, dtype=np.float64), np.asarray(ring_weights, dtype=np.float64))):
        A, S = ring_average(lambdas, I[r], V, s, points)
        out += LD(w) * A
        scale += abs(LD(w)) * S
    return out, scale


def flux_order_sum(intensities, ring_weights):
    """sum_r w_r I_r in fp64 in the flux's order: two ascending halves over r, each from 0.0, the lower added to the upper"""
    I, w = np.asarray(intensities, dtype=np.float64), np.asarray(ring_weights, dtype=np.float64)
    half = (w.size + 1) // 2
    lower, upper = np.zeros(I.shape[1]), np.zeros(I.shape[1])
    for r in range(w.size):
        if r < half:
            lower = lower + I[r] * w[r]
        else:
            upper = upper + I[r] * w[r]
    return lower + upper


def gray_rings(n_rings, eps):
    """Gauss-Legendre rings in s = sin(theta) in [0, 1] -> (ring_scale, weights 2 s ds, limb factors 1 - eps + eps sqrt(1 - s^2))"""
    x, w = np.polynomial.legendre.leggauss(n_rings)
    s, ds = 0.5 * (x + 1.0), 0.5 * w
    return s, 2.0 * s * ds, 1.0 - eps + eps * np.sqrt((1.0 - s) * (1.0 + s))
