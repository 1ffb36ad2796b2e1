"""The adjoint of the mean intensity and of the scattering solve (include/stardis_hip.h, sdx_mean_intensity_adjoint_dev and
sdx_scatter_response_dev) restated in numpy on scattering_reference.Operator: every function takes its number type from the operator,
np.longdouble (the truth) or np.float64 (the plain restatement, whose own distance from the truth sets the tolerance through
formal_solution_truth.bound).

    transposed(op, z)             Lambda^T z, by the walk against each sweep (op.matrix() transposed is the dense truth it is checked against)
    gradient(op, z, S)            G[k] = d(z^T J[S]) / d ln alpha[k] at fixed S
    iterate(op, w, c, ...)        the transposed Jacobi loop, run to the stopping rule or for a GIVEN number of iterations per column
    outputs(op, w, B, S, y, d)    y -> R_thermal, R_absorption, R_scatter (and z, G, J, A, H)
    response(op, w, B, S, c, d)   the three planes from a dense transposed solve: no iteration in the way

Used by tests/test_scattering_adjoint_cpu.py and tests/test_gpu_scattering_adjoint.py.
"""
import numpy as np

import formal_solution_truth as T
import scattering_reference as R

L = T.L
EXTENDED = T.EXTENDED
# what the GPU tests measured in this process: (label, quantity, n_depth, n_theta, class or column, kernel's figure, restatement's figure);
# scripts/scattering_adjoint_truth_table.py runs the tests and writes these out
RECORD = []


class Coefficients:
    """of one sweep over tau [n_gap][n_nu][n_theta] in the sweep's own order, step s through gap s with the next gap s + 1:
    c, a, q, r, p0 [n_gap][n_nu][n_theta] — the formulas of sdx_response_dev, the (1, 0) step where tau == 0 — and derivatives(S)"""

    def __init__(self, tau, dtype):
        f = dtype
        with np.errstate(all="ignore"):
            n = tau.shape[0]
            t = tau
            w0, w1, w2 = R._weights(t, f)
            E = R.exp_neg64(t) if f is np.float64 else np.exp(-t)
            small, mid = t < T.TAU_SMALL, t < T.TAU_BIG
            self.p0 = np.where(small, 1 - t, np.where(mid, E, f(0)))
            self.p1 = np.where(small, t - t ** 2, np.where(mid, t * E, f(0)))
            self.p2 = np.where(small, t ** 2 - t ** 3, np.where(mid, t ** 2 * E, f(0)))
            self.zero = t == 0
            t1 = np.concatenate([t[1:], np.ones_like(t[:1])])
            s = t + t1
            a, r = (w1 * t1 / t + w2 / t) / s, (-w1 * t / t1 + w2 / t1) / s
            a[n - 1], r[n - 1] = w2[n - 1] / t[n - 1] ** 2, 0
            q = w0 - a - r
            self.c = np.where(self.zero, f(1), 1 - w0)
            self.a, self.q, self.r = (np.where(self.zero, f(0), x) for x in (a, q, r))
            self.p0 = np.where(self.zero, f(0), self.p0)
            self.t, self.t1, self.w0, self.w1, self.w2, self.n, self.dtype = t, t1, w0, w1, w2, n, f

    def derivatives(self, S):
        """S [n_gap + 1][n_nu] in the sweep's order -> (de/dt0, de/dt1) [n_gap][n_nu][n_theta]"""
        f, n = self.dtype, self.n
        de0, de1 = np.zeros_like(self.t), np.zeros_like(self.t)
        with np.errstate(all="ignore"):
            for g in range(n - 1):
                t0, t1, s = self.t[g], self.t1[g], self.t[g] + self.t1[g]
                S1 = S[g + 1][:, None]
                d10, d21 = S[g][:, None] - S1, S[g + 2][:, None] - S1
                A = d10 * t1 / t0 - d21 * t0 / t1
                B = d10 / t0 + d21 / t1
                de0[g] = (self.p0[g] * S1 + (self.p1[g] * A + self.p2[g] * B) / s + self.w1[g] * ((-d21 / t1 - d10 * t1 / t0 ** 2) / s - A / s ** 2)
                          + self.w2[g] * ((-d10 / t0 ** 2) / s - B / s ** 2))
                de1[g] = self.w1[g] * ((d10 / t0 + d21 * t0 / t1 ** 2) / s - A / s ** 2) + self.w2[g] * ((-d21 / t1 ** 2) / s - B / s ** 2)
            g = n - 1
            t0, S1, d10 = self.t[g], S[g + 1][:, None], S[g][:, None] - S[g + 1][:, None]
            de0[g] = self.p0[g] * S1 + self.p2[g] * d10 / t0 ** 2 - 2 * self.w2[g] * d10 / t0 ** 3
            de0[self.zero] = 0
            de1[self.zero] = 0
        return de0, de1


def _coefficients(op):
    if not hasattr(op, "_adjoint_coefficients"):
        op._adjoint_coefficients = (Coefficients(op.tau, op.dtype), Coefficients(op.tau[::-1], op.dtype))
    return op._adjoint_coefficients


def _theta_sum(x):
    """sum over the last axis: two ascending halves, the lower added to the upper (the weights are inside the terms)"""
    n = x.shape[-1]
    half = (n + 1) >> 1
    lo, hi = np.zeros(x.shape[:-1], dtype=x.dtype), np.zeros(x.shape[:-1], dtype=x.dtype)
    with np.errstate(all="ignore"):
        for k in range(half):
            lo = lo + x[..., k]
        for k in range(half, n):
            hi = hi + x[..., k]
        return lo + hi


def _vbar(op, k, z):
    """z [n_depth][n_nu] in the sweep's order -> vbar [n_depth][n_nu][n_theta]"""
    n = k.n
    v = np.empty((n + 1, op.n_nu, op.n_theta), dtype=op.dtype)
    with np.errstate(all="ignore"):
        v[n] = op.m * z[n][:, None]
        for s in range(n - 1, -1, -1):
            v[s] = op.m * z[s][:, None] + k.c[s] * v[s + 1]
    return v


def transposed(op, z):
    """Lambda^T z [n_depth][n_nu]"""
    z = np.asarray(z).astype(op.dtype)
    out = None
    with np.errstate(all="ignore"):
        for dir_, k in enumerate(_coefficients(op)):
            zs = z[::-1] if dir_ else z
            v = _vbar(op, k, zs)
            n = k.n
            rows = np.zeros((n + 1, op.n_nu, op.n_theta), dtype=op.dtype)
            rows[:n] = k.a * v[1:]
            rows[1:] = rows[1:] + k.q * v[1:]
            if n > 1:
                rows[2:] = rows[2:] + k.r[:-1] * v[1:-1]
            if dir_ == 0:
                rows[0] = rows[0] + v[0]  # U[0] = S[0]
            summed = _theta_sum(rows)
            out = summed if dir_ == 0 else out + summed[::-1]
    return out


def gradient(op, z, S):
    """G [n_depth][n_nu]: the derivative of z^T J[S] with respect to ln alpha[k] at fixed S"""
    z, S = np.asarray(z).astype(op.dtype), np.asarray(S).astype(op.dtype)
    U, D = op.sweeps(S)
    out = None
    with np.errstate(all="ignore"):
        for dir_, k in enumerate(_coefficients(op)):
            zs, Ss, val = (z[::-1], S[::-1], D[::-1]) if dir_ else (z, S, U)
            v = _vbar(op, k, zs)
            de0, de1 = k.derivatives(Ss)
            n = k.n
            tbar = v[1:] * (de0 - k.p0 * val[:-1])
            tbar[1:] = tbar[1:] + v[1:-1] * de1[:-1]
            tt = k.t * tbar
            rows = np.zeros((n + 1, op.n_nu, op.n_theta), dtype=op.dtype)
            rows[1:] = tt
            rows[:-1] = rows[:-1] + tt
            summed = _theta_sum(rows * op.dtype(0.5))
            out = summed if dir_ == 0 else out + summed[::-1]
    return out


def iterate(op, w, c, tol=None, max_iter=None, counts=None):
    """The iteration of sdx_scatter_response_dev: y^0 = c, y^(n+1) = y^n + (c + Lambda^T (w y^n) - y^n) / (1 - w clamp(L)).  counts
    [n_nu]: column i takes exactly counts[i] updates; else the stopping rule.  -> dict(y, iterations, status, change)"""
    dt = op.dtype
    c, w = np.asarray(c).astype(dt), np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        inv = 1 / (1 - w * R.clamp01(op.diagonal(), dt))
        y = c.copy()
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
            dy = ((c + transposed(op, w * y)) - y) * inv
            new = y + dy
            finite = np.isfinite(dy).all(axis=0)
            cd = np.where(finite, np.abs(dy).max(axis=0), dt(np.inf))
            cs = np.abs(new).max(axis=0)
            iterations[live], change[live] = n, cd[live]
            status[live & ~finite] = 2
            upd = live & finite
            y[:, upd] = new[:, upd]
            if counts is None:
                done = upd & (cd <= dt(tol) * cs)
                status[done] = 0
                live = upd & ~done
            else:
                live = upd & (counts > n)
    return dict(y=y, iterations=iterations, status=status, change=change)


def outputs(op, w, B, S, y, direct=None):
    """-> dict(z, G, J, A, H, R_thermal, R_absorption, R_scatter) from the solved y"""
    dt = op.dtype
    w, B, S, y = (np.asarray(x).astype(dt) for x in (w, B, S, y))
    d = np.zeros_like(y) if direct is None else np.asarray(direct).astype(dt)
    with np.errstate(all="ignore"):
        z = w * y
        G = gradient(op, z, S)
        J = op.J(S)
        A = d + G
        H = y * (J - B)
        return dict(z=z, G=G, J=J, A=A, H=H, R_thermal=(1 - w) * y, R_absorption=A - w * H, R_scatter=w * A + w * (1 - w) * H)


def dense_solve(op, w, c):
    """y of (1 - Lambda^T W) y = c, column by column by elimination"""
    lam = op.matrix()
    c, w = np.asarray(c).astype(op.dtype), np.asarray(w).astype(op.dtype)
    y = np.empty_like(c)
    eye = np.eye(op.n_depth, dtype=op.dtype)
    for i in range(op.n_nu):
        y[:, i] = R.solve(eye - lam[:, :, i].T * w[:, i][None, :], c[:, i])
    return y


def response(op, w, B, S, cotangent, direct=None):
    return outputs(op, w, B, S, dense_solve(op, w, cotangent), direct)


# ---- the emergent flux of the scattering solution against difference quotients ----------------------------------------------------
# On a grid problem p (tests/test_gpu_scattering.py, grid_problem: total opacity p.alphas, albedo p.albedo, thermal plane p.B) the
# functional is the emergent flux Phi = F_nu[N_d-1] of the formal solution with source = S.  Three seeded directions, all RELATIVE so that
# a column without scattering has a direction too:
#     absorption   alpha -> alpha + eps pa (alpha - alpha_scatter)          dPhi/d eps = sum_k R_absorption[k] pa[k] (1 - albedo[k])
#                  (at fixed alpha_scatter; relative to the ABSORBING part: at albedo 0.999 a step relative to the total would
#                  multiply the absorption several times over)
#     scatter      alpha_scatter -> alpha_scatter (1 + eps ps)              dPhi/d eps = sum_k R_scatter[k] ps[k]
#     thermal      B -> B (1 + eps pb)                                      dPhi/d eps = sum_k R_thermal[k] pb[k] B[k]
# and the Richardson quotient (4 D(h/2) - D(h)) / 3 of central differences D.  gap = |prediction - quotient| / (sum_k |R[k] p[k]| + |Phi|):
# eps is a relative change, so the flux itself is the derivative's natural unit — and the quotient's rounding noise is a fraction of Phi,
# not of the derivative (an isothermal column's flux hardly depends on its opacity at all).
QUANTITIES = ("R_absorption", "R_scatter", "R_thermal")
H_DEVICE = 1e-2  # the step of the fp64 quotients (device and fp64 restatement alike): their truncation error, h^4 / 30 of a fifth derivative,
#                  stays above the quotient's rounding noise 1e-16 |Phi| / h, so that the gap is a property of the functional and not of luck
TOL_DEVICE = 1e-13  # where the forward solve of the fp64 quotients stops
H_TRUTH = 1e-4   # the step of the 80-bit quotient: truncation 1e-17 of a fifth derivative, rounding noise 2^-64 / h = 5e-16 of Phi


def directions(p, seed=11):
    rng = np.random.default_rng(seed)
    return {name: rng.uniform(0.5, 1.5, (p.n_depth, p.n_nu)) for name in QUANTITIES}


def perturbed(p, name, direction, eps, dtype):
    """-> (total_alphas, alpha_scatter, B) in dtype, moved by eps along one direction"""
    total, B = p.alphas.astype(dtype), p.B.astype(dtype)
    sc = p.albedo.astype(dtype) * total
    d = direction.astype(dtype) * dtype(eps)
    if name == "R_absorption":
        return total + d * (total - sc), sc, B
    if name == "R_scatter":
        return (total - sc) + sc * (1 + d), sc * (1 + d), B
    return total, sc, B * (1 + d)


def richardson(phi, h):
    """phi(eps) -> the derivative at 0 from central differences at h and h / 2"""
    D = lambda e: (phi(e) - phi(-e)) / (2 * e)  # noqa: E731
    return (4 * D(h / 2) - D(h)) / 3


def gap(prediction, quotient, scale):
    with np.errstate(all="ignore"):
        diff = np.abs(np.asarray(prediction).astype(L) - np.asarray(quotient).astype(L))
        return np.where(diff == 0, L(0), diff / np.asarray(scale).astype(L)).astype(np.float64)


def weighted(name, planes, p, direction):
    """-> (sum_k R[k] p[k], sum_k |R[k] p[k]|) per column"""
    x = planes[name] * direction.astype(planes[name].dtype)
    if name == "R_thermal":
        x = x * p.B.astype(x.dtype)
    if name == "R_absorption":
        x = x * (1 - p.albedo.astype(x.dtype))
    return x.sum(axis=0), np.abs(x).sum(axis=0)


def dense_iterate(op, w, B, tol, max_iter=2000):
    """sdx_scatter_source_dev's iteration and stopping rule with the dense operator in place of the sweeps: what a solve that stops at
    `tol` leaves of the fixed point, at the cost of a matrix-vector product per iteration"""
    lam, dt = op.matrix(), op.dtype
    inv = 1 / (1 - w * R.clamp01(op.diagonal(), dt))
    before, S, after = B.copy(), B.copy(), B.copy()

    def update(x, i):
        return x + (((1 - w[:, i]) * B[:, i] + w[:, i] * (lam[:, :, i] @ x)) - x) * inv[:, i]

    for i in range(op.n_nu):
        for _ in range(max_iter):
            before[:, i], S[:, i] = S[:, i], update(S[:, i], i)
            if np.abs(S[:, i] - before[:, i]).max() <= dt(tol) * np.abs(S[:, i]).max():
                break
        after[:, i] = update(S[:, i], i)
    return before, S, after


def restated_flux(p, total, sc, B, dtype, tol=None):
    """the emergent flux of the scattering solution -> (response_truth.response's dict with F [n_nu], S, op, albedo); the fixed point by
    elimination, or with `tol` by the iteration that stops there — the dict then also holds F_stops, the flux of the iterate one update
    before the stop, at it and one after"""
    import response_truth as RT

    op = R.operator(total, p.ray, p.m, dtype)
    w = R.albedo(sc, total, dtype)
    if tol is None:
        S = R.direct_solve(op, w, B)
        return RT.response(p.nus, p.temps, p.ray, p.weights, total, S, dtype), S, op, w
    before, S, after = dense_iterate(op, w, B, tol)
    out = RT.response(p.nus, p.temps, p.ray, p.weights, total, S, dtype)
    out["F_stops"] = [RT.response(p.nus, p.temps, p.ray, p.weights, total, x, dtype)["F"] for x in (before, after)] + [out["F"]]
    return out, S, op, w


_gaps = {}


def restated_gaps(p, key, dtype, h, seed=11, tol=None):
    """{quantity: gap [n_nu]} of the restatement in dtype against its own Richardson quotient with step h, the fixed point by elimination
    or (tol) by the iteration stopped at tol — as a device that iterates forms it; cached under `key`.
    With tol the gap is the LARGEST over where each of the quotient's four solves may stop: at the restatement's own count, one update
    earlier or one later, independently — the freedom the solve's own test grants a device (its count within one of the restatement's).
    What a solve leaves of the fixed point when it stops is a few times tol; the quotient divides the difference of two such remainders by
    h, and whether they cancel is decided by whether the two counts agree.  For a quantity in which the flux is linear (R_thermal) that
    is all the gap there is: a single sample of it would measure the luck of the counts, not the procedure."""
    import itertools
    if (key, dtype, h, tol) not in _gaps:
        dirs = directions(p, seed)
        total, sc, B = perturbed(p, "R_thermal", dirs["R_thermal"], 0.0, dtype)
        base, S, op, w = restated_flux(p, total, sc, B, dtype, tol)
        planes = response(op, w, B, S, base["Rs"], base["Ra"])
        out = {}
        for name in QUANTITIES:
            value, scale = weighted(name, planes, p, dirs[name])
            if tol is None:
                quotient = richardson(lambda e: restated_flux(p, *perturbed(p, name, dirs[name], e, dtype), dtype)[0]["F"], dtype(h))
                out[name] = gap(value, quotient, scale + np.abs(base["F"]))
                continue
            hh = dtype(h)
            stops = [restated_flux(p, *perturbed(p, name, dirs[name], e, dtype), dtype, tol)[0]["F_stops"] for e in (hh, -hh, hh / 2, -hh / 2)]
            worst = np.zeros(p.n_nu)
            for a, b, c, d in itertools.product(*stops):
                quotient = (4 * (c - d) / hh - (a - b) / (2 * hh)) / 3
                worst = np.maximum(worst, gap(value, quotient, scale + np.abs(base["F"])))
            out[name] = worst
        _gaps[(key, dtype, h, tol)] = out
    return _gaps[(key, dtype, h, tol)]
