"""Flux contribution function and formation mean restated in numpy, for the sizes and shards no reference run exists for.

Built from the source function and the weights of the short-characteristic step (van Noort 2002 eq. 14 as the reference
writes it, radiation_field_solvers/base.py:22-45 and :200-266) — NOT from a traced intensity: per ray and gap the step is
I[g+1] = c[g] I[g] + e[g] with

    c = 1 - w0
    e = w0 S1 + w1 [(S1-S2) t0/t1 - (S1-S0) t1/t0] / (t0+t1) + w2 [(S2-S1)/t1 + (S0-S1)/t0] / (t0+t1)     (g < N_d-2)
    e = w0 S1 + w2 (S0-S1) / t0^2                                                                          (last gap)

and (c, e) = (1, 0) where t0 == 0 (:203-206, :253-254).  T[N_d-1] = 1, T[k] = T[k+1] c[k];  C[0] = 0,
C[k] = sum_theta w_theta (T[k] e[k-1]), theta in two ascending halves with the lower added to the upper.
"""
import decimal
import math

import numpy as np

H_CGS, C_CGS, K_B_CGS = 6.62607015e-27, 29979245800.0, 1.380649e-16


# ---- exp and log as correctly rounded functions -------------------------------------------------------------------------------
# np.exp and np.log are properties of the numpy build and of the CPU it dispatches on: two builds differ in the last bit of a few
# per cent of the values.  The scheme amplifies that bit: log(alpha) ~ -30 turns one ulp of the logarithm into 7e-15 of the mean
# opacity, and in a thin gap (tau just above 5e-4) w2 = 2 w1 - tau^2 exp(-tau) cancels six digits, so that the rounding pattern of the
# weights — and with it C at the 1e-11 level — belongs to the library, not to the scheme.  The correctly rounded value of either
# function is unique, so a golden made with them (tests/golden/make_golden_contribution.py) can be reproduced anywhere: 40-digit
# decimal arithmetic of the standard library, rounded once to the nearest double.
_CONTEXT = decimal.Context(prec=40)


def _exact(fn, fallback):
    def scalar(v):
        v = float(v)
        if not math.isfinite(v) or (fn == "ln" and v <= 0.0):
            return float(fallback(v))  # zeros, infinities, NaN, negative arguments: IEEE special values, the same everywhere
        return float(getattr(_CONTEXT.create_decimal_from_float(v), fn)(context=_CONTEXT))

    table = np.frompyfunc(scalar, 1, 1)

    def call(x):
        with np.errstate(all="ignore"):
            out = table(x)
        return np.float64(out) if np.ndim(out) == 0 else out.astype(np.float64)

    return call


exact_exp = _exact("exp", np.exp)
exact_log = _exact("ln", np.log)


def planck(nus, temps):
    """B_nu(T) -> (N_d, N_nu), the operations of source_functions/blackbody.py:31-35."""
    nus = np.asarray(nus, dtype=np.float64).reshape(1, -1)
    t = np.asarray(temps, dtype=np.float64).reshape(-1, 1)
    return (2.0 * H_CGS * nus**3 / C_CGS**2) / (np.exp(H_CGS * nus / (K_B_CGS * t)) - 1.0)


def weights(tau, exp=np.exp):
    """w0, w1, w2 of :22-45: the series below 5e-4, the exponential form below 50, (1, 1, 2) otherwise."""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = exp(-tau)
        w0 = 1.0 - e
        w1 = w0 - tau * e
        w2 = 2.0 * w1 - tau * tau * e
        small, big = tau < 5e-4, ~(tau < 50)
        w0 = np.where(small, tau * (1.0 - tau / 2), np.where(big, 1.0, w0))
        w1 = np.where(small, tau * tau * (0.5 - tau / 3), np.where(big, 1.0, w1))
        w2 = np.where(small, tau * tau * tau * (1.0 / 3 - tau / 4), np.where(big, 2.0, w2))
    return w0, w1, w2


def contribution_function(nus, temps, ray_dist, theta_weights, total_alphas, source=None, exact=False):
    """-> C (N_d, N_nu).  ray_dist: (N_d-1, N_theta) = dist[:, None] / cos(thetas); source: optional (N_d, N_nu) plane, default Planck.
    exact: exp and log of the mean opacity and of the weights correctly rounded (above; ~10 us per value) instead of numpy's."""
    exp, log = (exact_exp, exact_log) if exact else (np.exp, np.log)
    temps = np.asarray(temps, dtype=np.float64).reshape(-1)
    alphas = np.asarray(total_alphas, dtype=np.float64)
    ray_dist = np.asarray(ray_dist, dtype=np.float64).reshape(temps.size - 1, -1)
    wts = np.asarray(theta_weights, dtype=np.float64).reshape(-1)
    n_depth, n_nu = alphas.shape
    S = planck(nus, temps) if source is None else np.asarray(source, dtype=np.float64)
    with np.errstate(all="ignore"):
        mean = exp((log(alphas[1:]) + log(alphas[:-1])) * 0.5)  # :121
        terms = []
        for th in range(wts.size):
            tau = mean * ray_dist[:, th:th + 1]  # :123-129
            w0, w1, w2 = weights(tau, exp)
            c = np.where(tau == 0, 1.0, 1.0 - w0)
            e = np.empty_like(tau)
            t0, t1 = tau[:-1], tau[1:]
            d10, d21 = S[:-2] - S[1:-1], S[2:] - S[1:-1]
            e[:-1] = (w0[:-1] * S[1:-1] + w1[:-1] * (-d21 * t0 / t1 + d10 * t1 / t0) / (t0 + t1)
                      + w2[:-1] * (d21 / t1 + d10 / t0) / (t0 + t1))
            e[-1] = w0[-1] * S[-1] + w2[-1] * (S[-2] - S[-1]) / tau[-1] ** 2
            e = np.where(tau == 0, 0.0, e)
            trans = np.ones((n_depth, n_nu))
            for k in range(n_depth - 2, -1, -1):
                trans[k] = trans[k + 1] * c[k]
            terms.append((trans[1:] * e) * wts[th])
        half = (wts.size + 1) >> 1
        lower, upper = np.zeros((n_depth - 1, n_nu)), np.zeros((n_depth - 1, n_nu))
        for t in terms[:half]:
            lower = lower + t
        for t in terms[half:]:
            upper = upper + t
    C = np.zeros((n_depth, n_nu))
    C[1:] = lower + upper
    return C


def formation_mean(C, x):
    """<x> = (sum_{k>=1} C[k] m_k) / (sum_{k>=1} C[k]), m_k = (x[k-1] + x[k]) 0.5: ascending k, one rounding per operation
    (what sdx_formation_mean_dev computes, bit for bit); 0 / 0 -> NaN."""
    C = np.asarray(C, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    num, den = np.zeros(C.shape[1]), np.zeros(C.shape[1])
    for k in range(1, C.shape[0]):
        m = (x[k - 1] + x[k]) * 0.5
        num = num + C[k] * m
        den = den + C[k]
    with np.errstate(all="ignore"):
        return num / den
