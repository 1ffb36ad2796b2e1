"""The response functions (include/stardis_hip.h, sdx_response_dev) restated in numpy, on the columns of tests/formal_solution_truth.py.

response(..., dtype=longdouble) is the truth: the definitions evaluated with a 64-bit mantissa.  response(..., dtype=float64) is the
restatement: the same lines in double precision, which plays the oracle's role — a kernel is held to be no further from the truth
than formal_solution_truth.bound(the restatement's own distance, N_d).  Both form the mean opacity of a gap as the reference does,
exp((log a + log a') / 2); the kernels' sqrt(a) sqrt(a') is what the per-gap term of bound() is for.

The four classes at the ends of the double range (tiny, underflow, huge, overflow) are outside the contract the header states: the
derivative divides by t0^3 and (t0 + t1)^2.  Used by tests/test_response_cpu.py and tests/test_gpu_response.py.
"""
import numpy as np

import formal_solution_truth as T
from stardis_amd import constants as K

L = T.L
CLASSES = ("thin", "straddle_small", "moderate", "straddle_50", "thick", "everything", "ramp", "leading_transparent",
           "interior_transparent", "surface_transparent", "transparent", "spike")
OPAQUE = tuple(name for name in CLASSES if "transparent" not in name)  # every row has alpha > 0: ln alpha can be perturbed
EXCLUDED_AT_MOST = 1.0 / 8  # of a class's columns: near a threshold of the weights, or nowhere finite in the restatement


def planck(nus, temps, dtype):
    nus, temps = np.asarray(nus).astype(dtype), np.asarray(temps).astype(dtype)
    pre = (2 * dtype(K.H_CGS) * nus ** 3) / (dtype(K.C_CGS) ** 2)
    return pre[None, :] / (np.exp((dtype(K.H_CGS) * nus)[None, :] / (dtype(K.K_B_CGS) * temps[:, None])) - 1)


def theta_sum(terms, weights):
    """sum over the last axis of terms * weights in the flux's order: two ascending halves, the lower added to the upper"""
    x = terms * weights
    n = x.shape[-1]
    half = (n + 1) >> 1
    lo, hi = np.zeros(x.shape[:-1], dtype=x.dtype), np.zeros(x.shape[:-1], dtype=x.dtype)
    for j in range(half):
        lo = lo + x[..., j]
    for j in range(half, n):
        hi = hi + x[..., j]
    return lo + hi


def response(nus, temps, ray, weights, alphas, source=None, dtype=L):
    """-> dict(Ra, Rs, F, S): R_alpha (N_d, N_nu), R_source (N_d, N_nu), the emergent flux (N_nu,) and the source plane, in `dtype`.
    ray: the (N_d - 1, N_theta) table of ray lengths, formed in double by the caller."""
    f = dtype
    alphas = np.asarray(alphas).astype(f)
    nd, nn = alphas.shape
    rd = np.asarray(ray, dtype=np.float64).astype(f)
    nt = rd.shape[1]
    wts = np.asarray(weights).astype(f)
    S = planck(nus, temps, f) if source is None else np.asarray(source).astype(f).reshape(nd, nn)
    ng = nd - 1
    with np.errstate(all="ignore"):
        mean = np.exp((np.log(alphas[1:]) + np.log(alphas[:-1])) * f(0.5))
        t = mean[:, :, None] * rd[:, None, :]  # (N_g, N_nu, N_theta)
        E = np.exp(-t)
        small, mid = t < T.TAU_SMALL, t < T.TAU_BIG
        w0 = np.where(small, t * (1 - t / 2), np.where(mid, 1 - E, f(1)))
        w1 = np.where(small, t ** 2 * (f(0.5) - t / 3), np.where(mid, (1 - E) - t * E, f(1)))
        w2 = np.where(small, t ** 3 * (f(1) / 3 - t / 4), np.where(mid, 2 * ((1 - E) - t * E) - t ** 2 * E, f(2)))
        p0 = np.where(small, 1 - t, np.where(mid, E, f(0)))
        p1 = np.where(small, t - t ** 2, np.where(mid, t * E, f(0)))
        p2 = np.where(small, t ** 2 - t ** 3, np.where(mid, t ** 2 * E, f(0)))
        zero = t == 0
        c = np.where(zero, f(1), 1 - w0)
        e, de0, de1, a, q, r = (np.zeros_like(t) for _ in range(6))
        for g in range(ng - 1):
            t0, t1, s = t[g], t[g + 1], t[g] + t[g + 1]
            S0, S1, S2 = S[g][:, None], S[g + 1][:, None], S[g + 2][:, None]
            d10, d21 = S0 - S1, S2 - S1
            A = d10 * t1 / t0 - d21 * t0 / t1
            B = d10 / t0 + d21 / t1
            e[g] = w0[g] * S1 + (w1[g] * A + w2[g] * B) / s
            de0[g] = (p0[g] * S1 + (p1[g] * A + p2[g] * B) / s + w1[g] * ((-d21 / t1 - d10 * t1 / t0 ** 2) / s - A / s ** 2)
                      + w2[g] * ((-d10 / t0 ** 2) / s - B / s ** 2))
            de1[g] = w1[g] * ((d10 / t0 + d21 * t0 / t1 ** 2) / s - A / s ** 2) + w2[g] * ((-d21 / t1 ** 2) / s - B / s ** 2)
            a[g] = (w1[g] * t1 / t0 + w2[g] / t0) / s
            r[g] = (-w1[g] * t0 / t1 + w2[g] / t1) / s
            q[g] = w0[g] - a[g] - r[g]
        g = ng - 1
        t0, S1, d10 = t[g], S[g + 1][:, None], S[g][:, None] - S[g + 1][:, None]
        e[g] = w0[g] * S1 + w2[g] * d10 / t0 ** 2
        de0[g] = p0[g] * S1 + p2[g] * d10 / t0 ** 2 - 2 * w2[g] * d10 / t0 ** 3
        a[g] = w2[g] / t0 ** 2
        q[g] = w0[g] - a[g]
        for x in (e, de0, de1, a, q, r):  # the (1, 0) step: no derivative, no coefficient
            x[zero] = 0
        p0 = np.where(zero, f(0), p0)
        I = np.zeros((nd, nn, nt), dtype=f)
        for g in range(ng):
            I[g + 1] = np.where(zero[g], I[g], c[g] * I[g] + e[g])
        Tr = np.ones((nd, nn, nt), dtype=f)
        for k in range(nd - 2, -1, -1):
            Tr[k] = Tr[k + 1] * c[k]
        G = Tr[1:] * (-p0 * I[:-1] + de0)  # G[j], j = 0 .. N_g - 1
        G[1:] = G[1:] + Tr[1:-1] * de1[:-1]
        tG = t * G
        ra = np.zeros((nd, nn, nt), dtype=f)
        ra[1:] = tG
        ra[1:-1] = ra[1:-1] + tG[1:]
        ra[0] = tG[0]
        rs = np.zeros((nd, nn, nt), dtype=f)
        rs[:-1] = Tr[1:] * a
        rs[1:] = rs[1:] + Tr[1:] * q
        if nd > 2:
            rs[2:] = rs[2:] + Tr[1:-1] * r[:-1]
        return dict(Ra=theta_sum(ra * f(0.5), wts), Rs=theta_sum(rs, wts), F=theta_sum(I[-1], wts), S=S)


class Responses:
    """truth and restatement of one Case, computed once and left unchanged; `source`: None (Planck) or a plane"""

    def __init__(self, c, source=None):
        self.case, self.source = c, source
        self.truth = response(c.nus, c.temps, c.ray, c.weights, c.alphas, source, L)
        self.restated = response(c.nus, c.temps, c.ray, c.weights, c.alphas, source, np.float64)
        for d in (self.truth, self.restated):
            for v in d.values():
                v.setflags(write=False)
        self.keep = ~T.near_threshold(c.alphas, c.ray)

    def excluded(self, key):
        """per column: flagged by near_threshold, or the restatement is finite nowhere in it"""
        return ~self.keep | ~np.isfinite(self.restated[key]).any(axis=0)


_responses = {}


def responses(n_depth, n_theta, per_class, order="grouped", source_seed=None):
    """cached per shape; source_seed: a caller's source plane drawn from that seed instead of the Planck function"""
    key = (n_depth, n_theta, per_class, order, source_seed)
    if key not in _responses:
        c = T.case(n_depth, n_theta, per_class, order, CLASSES)
        source = None
        if source_seed is not None:  # rough, positive, of the Planck function's size
            rng = np.random.default_rng(source_seed)
            source = planck(c.nus, c.temps, np.float64) * rng.uniform(0.3, 3.0, (n_depth, c.n_nu))
        _responses[key] = Responses(c, source)
    return _responses[key]


def source_plane(nus, temps):
    return planck(nus, temps, np.float64)
