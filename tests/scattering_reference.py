"""The mean intensity and the scattering source iteration of include/stardis_hip.h (sdx_mean_intensity_dev, sdx_scatter_source_dev),
restated in numpy: every function takes the number type, np.longdouble (the truth a kernel is judged against, as in
formal_solution_truth) or np.float64 (the plain restatement, whose own distance from the truth sets the tolerance through
formal_solution_truth.bound).

    Operator.sweeps()    U and D of a source plane, per (row, column, angle)
    Operator.J(), .diagonal(), mean_intensity()    J and the diagonal L
    Operator.matrix()    the dense operator, column by column from unit vectors
    direct_solve()       (1 - albedo Lambda) S = (1 - albedo) B by elimination
    iterate()            the Jacobi iteration with the local operator, run to the stopping rule or for a GIVEN number of iterations per column
    spectral_radius()    of the iteration's error propagation, for choosing grids on which it contracts

Used by tests/test_scattering_cpu.py and tests/test_gpu_scattering.py.  The GPU tests skip where formal_solution_truth.EXTENDED is false.
"""
import numpy as np

import formal_solution_truth as T
from stardis_amd import constants as K

L = T.L
EXTENDED = T.EXTENDED
# what the GPU tests measured in this process: (kernel label, quantity, n_depth, n_theta, class, kernel's distance, restatement's distance);
# scripts/scattering_truth_table.py runs the tests and writes these out
RECORD = []


def mean_weights(thetas, theta_weights, dtype=np.float64):
    """m_k = w_k sin(theta_k) / (2 sum_j w_j sin(theta_j)): sum_k 2 m_k = 1"""
    th, w = np.asarray(thetas).astype(dtype), np.asarray(theta_weights).astype(dtype)
    x = w * np.sin(th)
    return x / (2 * x.sum())


def planck(nus, temps, dtype):
    nus, temps = np.asarray(nus).astype(dtype), np.asarray(temps).astype(dtype)
    pre = (2 * dtype(K.H_CGS) * nus ** 3) / (dtype(K.C_CGS) ** 2)
    return pre[None, :] / (np.exp((dtype(K.H_CGS) * nus)[None, :] / (dtype(K.K_B_CGS) * temps[:, None])) - 1)


def optical_depths(alphas, ray_table, dtype):
    """tau[g][i][k] = (sqrt(alpha[g][i]) sqrt(alpha[g+1][i])) ray_table[g][k]; the table is formed in double by the caller"""
    a = np.sqrt(np.asarray(alphas).astype(dtype))
    rd = np.asarray(ray_table, dtype=np.float64).astype(dtype)
    return (a[:-1] * a[1:])[:, :, None] * rd[:, None, :]


def _split(a):
    """Veltkamp: a = hi + lo with 26-bit halves (fp64)"""
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma64(a, b, c):
    """a b + c rounded once, in fp64 arithmetic alone: the product exactly as p + e (Dekker), the sum p + c exactly as s + t (Knuth), then
    s + (t + e).  The fused multiply-add of the device to the last bit except in near-ties of the final sum."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    v = s - p
    t = (p - (s - v)) + (c - v)
    return s + (t + e)


_EXP_P = [float.fromhex(h) for h in ("0x1.ade156a5dcb37p-26", "0x1.28af3fca7ab0cp-22", "0x1.71dee623fde64p-19", "0x1.a01997c89e6b0p-16", "0x1.a01a014761f6ep-13",
                                     "0x1.6c16c1852b7b0p-10", "0x1.1111111122322p-7", "0x1.55555555502a1p-5", "0x1.5555555555511p-3", "0x1.000000000000bp-1")]


def exp_neg64(tau):
    """exp(-tau) as the formal-solution kernels form it (sdx_math.h, exp_neg: the device library's double-precision exp, operation for
    operation) — the definition's sweeps are the kernels' own step, and its exponential is part of that step.  It is faithfully rounded,
    not always libm's value, and in the gaps just above tau = 5e-4 the weights amplify that last bit by 1 / tau^3: a plain restatement
    with libm's exp measures libm's luck there, not the distance of an fp64 evaluation of the definition.  Arguments at or above 64 are
    never read (the weights are constants from tau = 50)."""
    tau = np.minimum(np.asarray(tau, dtype=np.float64), 64.0)
    n = np.rint(tau * float.fromhex("-0x1.71547652b82fep+0"))
    r = fma64(n, float.fromhex("-0x1.62e42fefa39efp-1"), -tau)
    r = fma64(float.fromhex("-0x1.abc9e3b39803fp-56"), n, r)
    p = fma64(r, _EXP_P[0], _EXP_P[1])
    for coef in _EXP_P[2:]:
        p = fma64(r, p, coef)
    p = fma64(r, p, 1.0)
    p = fma64(r, p, 1.0)
    return np.ldexp(p, n.astype(np.int64))


def _weights(tau, dtype):
    ex = exp_neg64(tau) if dtype is np.float64 else np.exp(-tau)
    small, mid = tau < T.TAU_SMALL, tau < T.TAU_BIG
    one = dtype(1)
    w0 = np.where(small, tau * (1 - tau / 2), np.where(mid, 1 - ex, one))
    w1 = np.where(small, tau ** 2 * (dtype(0.5) - tau / 3), np.where(mid, (1 - ex) - tau * ex, one))
    w2 = np.where(small, tau ** 3 * (one / 3 - tau / 4), np.where(mid, 2 * ((1 - ex) - tau * ex) - tau ** 2 * ex, dtype(2)))
    return w0, w1, w2


class Steps:
    """what a sweep over tau [n_gap][n_nu][n_theta] needs per step, formed once: step s arrives at row s + 1 through gap s; the next
    gap is s + 1, the last step has none.  e = w0 S1 + (k1 (S1 - S2) - k2 (S1 - S0)) + (k3 (S2 - S1) + k4 (S0 - S1)) — the reference's
    second-order terms with their factors t0 / t1 / (t0 + t1) ... formed first —, the last step e = w0 S1 + k4 (S0 - S1), k4 = w2 / t0^2.
    q: the coefficient of S1 in e (q = w0 - a - r, a = (w1 t1 / t0 + w2 / t0) / s, r = (w2 / t1 - w1 t0 / t1) / s; last step a = w2 / t0^2, r = 0)."""

    def __init__(self, tau, dtype):
        with np.errstate(all="ignore"):
            n = tau.shape[0]
            w0, w1, w2 = _weights(tau, dtype)
            self.zero = tau == 0
            self.w0, self.c = w0, 1 - w0
            t0 = tau
            t1 = np.concatenate([tau[1:], np.ones_like(tau[:1])])
            s = t0 + t1
            self.k1, self.k2 = w1 * (t0 / t1) / s, w1 * (t1 / t0) / s
            self.k3, self.k4 = w2 / t1 / s, w2 / t0 / s
            a, r = (w1 * (t1 / t0) + w2 / t0) / s, (w2 / t1 - w1 * (t0 / t1)) / s
            self.k4[n - 1] = a[n - 1] = w2[n - 1] / t0[n - 1] ** 2
            r[n - 1] = 0
            self.k1[n - 1] = self.k2[n - 1] = self.k3[n - 1] = 0
            self.q = np.where(self.zero, dtype(0), (w0 - a) - r)
            self.n = n

    def march(self, S, start):
        """S [n_gap + 1][n_nu] in the sweep's own order -> values [n_gap + 1][n_nu][n_theta], row 0 = start"""
        with np.errstate(all="ignore"):
            n = self.n
            out = np.empty((n + 1,) + self.c.shape[1:], dtype=self.c.dtype)
            out[0] = start
            for s in range(n):
                s0, s1 = S[s][:, None], S[s + 1][:, None]
                if s < n - 1:
                    s2 = S[s + 2][:, None]
                    e = self.w0[s] * s1 + (self.k1[s] * (s1 - s2) - self.k2[s] * (s1 - s0)) + (self.k3[s] * (s2 - s1) + self.k4[s] * (s0 - s1))
                else:
                    e = self.w0[s] * s1 + self.k4[s] * (s0 - s1)
                out[s + 1] = np.where(self.zero[s], out[s], self.c[s] * out[s] + e)
            return out


class Operator:
    """the two sweeps on one set of optical depths tau [n_gap][n_nu][n_theta] with mean weights m [n_theta]"""

    def __init__(self, tau, m, dtype):
        self.dtype = dtype
        self.m = np.asarray(m).astype(dtype)
        self.tau = tau
        self.up, self.down = Steps(tau, dtype), Steps(tau[::-1], dtype)
        self.n_depth, self.n_nu, self.n_theta = tau.shape[0] + 1, tau.shape[1], tau.shape[2]

    def theta_sum(self, x):
        """sum_k m_k x[..., k]: two ascending halves, the lower added to the upper"""
        half = (self.n_theta + 1) >> 1
        lo, hi = np.zeros(x.shape[:-1], dtype=self.dtype), np.zeros(x.shape[:-1], dtype=self.dtype)
        with np.errstate(all="ignore"):
            for k in range(half):
                lo = lo + x[..., k] * self.m[k]
            for k in range(half, self.n_theta):
                hi = hi + x[..., k] * self.m[k]
            return lo + hi

    def sweeps(self, S):
        S = np.asarray(S).astype(self.dtype)
        U = self.up.march(S, np.broadcast_to(S[0][:, None], (self.n_nu, self.n_theta)))  # a thermalised lower boundary
        D = self.down.march(S[::-1], self.dtype(0))[::-1]
        return U, D

    def J(self, S):
        U, D = self.sweeps(S)
        with np.errstate(all="ignore"):
            return self.theta_sum(U) + self.theta_sum(D)

    def diagonal(self):
        one, zero = np.ones((1, self.n_nu, self.n_theta), dtype=self.dtype), np.zeros((1, self.n_nu, self.n_theta), dtype=self.dtype)
        qU = np.concatenate([one, self.up.q])
        qD = np.concatenate([zero, self.down.q])[::-1]
        with np.errstate(all="ignore"):
            return self.theta_sum(qU) + self.theta_sum(qD)

    def matrix(self):
        """Lambda [n_depth (row)][n_depth (column)][n_nu]: column j is J of the j-th unit vector (per frequency, all unit vectors in
        one pass over the depths: the frequency's optical depths repeated n_depth times)"""
        out = np.empty((self.n_depth, self.n_depth, self.n_nu), dtype=self.dtype)
        eye = np.eye(self.n_depth, dtype=self.dtype)
        for i in range(self.n_nu):
            out[:, :, i] = Operator(np.repeat(self.tau[:, i:i + 1, :], self.n_depth, axis=1), self.m, self.dtype).J(eye)
        return out


def operator(alphas, ray_table, m, dtype):
    return Operator(optical_depths(alphas, ray_table, dtype), m, dtype)


def mean_intensity(alphas, ray_table, m, source, dtype):
    """-> (J, L), each [n_depth][n_nu]"""
    op = operator(alphas, ray_table, m, dtype)
    return op.J(source), op.diagonal()


def albedo(alpha_scatter, alphas, dtype):
    """alpha_scatter / alpha_total in [0, 1], 0 where alpha_total == 0 (and for NaN); alpha_scatter [n_depth] or [n_depth][n_nu]"""
    a = np.asarray(alphas).astype(dtype)
    sc = np.asarray(alpha_scatter).astype(dtype)
    sc = np.broadcast_to(sc[:, None] if sc.ndim == 1 else sc, a.shape)
    with np.errstate(all="ignore"):
        w = np.where(a == 0, dtype(0), sc / a)
        return np.where(w > 0, np.where(w < 1, w, dtype(1)), dtype(0))


def solve(A, b):
    """A x = b by elimination with partial pivoting, in A's own number type (numpy's solvers know no long double)"""
    if A.dtype == np.float64:
        return np.linalg.solve(A, b)
    A, b = A.copy(), b.copy()
    n = b.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= f[:, None] * A[k]
        b[k + 1:] -= f * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def direct_solve(op, w, B):
    """S [n_depth][n_nu] of (1 - albedo Lambda) S = (1 - albedo) B, column by column"""
    lam = op.matrix()
    B = np.asarray(B).astype(op.dtype)
    S = np.empty_like(B)
    eye = np.eye(op.n_depth, dtype=op.dtype)
    for i in range(op.n_nu):
        S[:, i] = solve(eye - w[:, i][:, None] * lam[:, :, i], (1 - w[:, i]) * B[:, i])
    return S


def clamp01(x, dtype):
    return np.where(x > 0, np.where(x < 1, x, dtype(1)), dtype(0))


def spectral_radius(op, w):
    """per column: the spectral radius of 1 - diag(1 / (1 - albedo Lc)) (1 - albedo Lambda), what one iteration does to the error"""
    lam = op.matrix().astype(np.float64)
    Lc = clamp01(op.diagonal(), op.dtype).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    out = np.empty(op.n_nu)
    eye = np.eye(op.n_depth)
    for i in range(op.n_nu):
        M = eye - (eye - w[:, i][:, None] * lam[:, :, i]) / (1 - w[:, i] * Lc[:, i])[:, None]
        out[i] = np.abs(np.linalg.eigvals(M)).max()
    return out


def iterate(op, w, B, tol=None, max_iter=None, counts=None):
    """The iteration of sdx_scatter_source_dev.  counts [n_nu]: column i takes exactly counts[i] updates (no stopping rule); else the
    stopping rule with tol and max_iter.  -> dict(S, iterations, status, change); a stopped column is frozen."""
    dt = op.dtype
    B, w = np.asarray(B).astype(dt), np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        thermal = (1 - w) * B
        inv = 1 / (1 - w * clamp01(op.diagonal(), dt))
        S = B.copy()
        n_nu = op.n_nu
        live = np.ones(n_nu, dtype=bool)
        iterations, status, change = np.zeros(n_nu, dtype=np.int32), np.ones(n_nu, dtype=np.int32), np.zeros(n_nu, dtype=dt)
        if counts is not None:
            counts = np.asarray(counts)
            live = counts > 0
            status[:] = 0
        n_max = int(counts.max()) if counts is not None else int(max_iter)
        for n in range(1, n_max + 1):
            if not live.any():
                break
            dS = ((thermal + w * op.J(S)) - S) * inv
            new = S + dS
            finite = np.isfinite(dS).all(axis=0)
            cd = np.where(finite, np.abs(dS).max(axis=0), dt(np.inf))
            cs = np.abs(new).max(axis=0)
            iterations[live], change[live] = n, cd[live]
            failed = live & ~finite
            status[failed] = 2
            upd = live & finite
            S[:, upd] = new[:, upd]
            if counts is None:
                done = upd & (cd <= dt(tol) * cs)
                status[done] = 0
                live = upd & ~done
            else:
                live = upd & (counts > n)
    return dict(S=S, iterations=iterations, status=status, change=change)


def alphas_for(dtau, dist):
    """a positive opacity column [n_depth] whose gaps, sqrt(alpha[g] alpha[g+1]) dist[g], have the vertical optical depths dtau [n_depth - 1]"""
    dtau, dist = np.asarray(dtau, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    a = np.empty(dtau.size + 1)
    a[0] = dtau[0] / dist[0]
    for g in range(dtau.size):
        a[g + 1] = (dtau[g] / dist[g]) ** 2 / a[g]
    return a


def log_grid(n, lo, hi):
    """the optical depth scale of n points log-spaced over [lo, hi], row 0 deepest -> (tau_points [n], dtau [n - 1])"""
    t = np.geomspace(hi, lo, n)
    return t, t[:-1] - t[1:]
