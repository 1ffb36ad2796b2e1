"""Ng acceleration of the scattering source iteration (include/stardis_hip.h, sdx_scatter_source_ng_dev, states the definition) and the
same rule applied to the adjoint iteration, which has no device entry ("The scattering adjoint"), restated in numpy on scattering_reference / scattering_adjoint_reference, which
stay as they are.  Both solves are one preconditioned fixed point x <- x + G(x), so one function states the rule for both:

    iterate_ng(G, x0, tol, max_iter, options)   updates, history, extrapolation, safeguard and stopping rule, per column
    forward_G(op, w, B), adjoint_G(op, w, c)     the updates of scattering_reference.iterate and scattering_adjoint_reference.iterate
    dense_forward_G, dense_adjoint_G             the same fixed points with the dense operator (a matrix product per update)
    NG_COLUMNS, problem(), cotangents()          the column set the CPU and the GPU tests share

The number type is x0's: np.float64 or np.longdouble.

The rule, per column (no column reads another's state):
    update         dx = G(x); x <- x + dx.  cd = max |dx|, cs = max |x + dx|; a non-finite dx is refused (status 2, the column freezes);
                   cd <= tol cs ends the column with status 0.  Evaluated on updates only.
    history        the last four iterates since the last extrapolation, the initial iterate and an extrapolated one included.
    extrapolation  after update n, where the column is live and accelerated, start <= n < max_iter (the iterate returned has always been
                   through an update), at least `period` updates since the last extrapolation and four iterates of history x0
                   (newest) .. x3:
                       q1 = (x0 - 2 x1) + x2, q2 = ((x0 - x1) - x2) + x3, q3 = x0 - x1
                       A1 = sum q1 q1, B1 = sum q1 q2, C1 = sum q1 q3, B2 = sum q2 q2, C2 = sum q2 q3   (unweighted, over depth)
                       det = A1 B2 - B1 B1, a = (C1 B2 - C2 B1) / det, b = (C2 A1 - C1 B1) / det
                       x <- (((1 - a) - b) x0 + a x1) + b x2
                   every operation rounded once.  The sums: lane g of `lanes` sums its depths g, g + lanes, ... ascending, then the
                   partials are added in ascending lane order.  A non-finite component (det == 0 included) skips the extrapolation:
                   nothing changes, nothing is counted, the history continues.
    safeguard      a whole period after an extrapolation the change cd of that update is compared with a reference, the change of the
                   update before the extrapolation.  Smaller: the extrapolation counts as a gain, and the next one takes a new
                   reference and a new copy of the iterate it replaces.  Not smaller: a strike; the next extrapolation keeps the
                   reference and the copy.  Two strikes in a row: the column takes the copy back (the iterate before the first of
                   the two extrapolations; the updates since are lost), continues plain for good, and `accelerations` stops counting.
                   No operator application is spent on it, and it reads the column's own numbers alone.
"""
import types

import numpy as np

import scattering_adjoint_reference as A
import scattering_reference as R

L = R.L
DEFAULTS = dict(start=4, period=4, accelerate=True, lanes=1, strikes=2, judge="period")


def _sum(p, lanes):
    """sum over axis 0 of p [n_depth][n_col]: lane g its depths g, g + lanes, ... ascending, then the lanes ascending"""
    total = np.zeros(p.shape[1:], dtype=p.dtype)
    for g in range(min(lanes, p.shape[0])):
        part = np.zeros(p.shape[1:], dtype=p.dtype)
        for d in range(g, p.shape[0], lanes):
            part = part + p[d]
        total = total + part
    return total


def extrapolate(x0, x1, x2, x3, lanes=1):
    """the unweighted second-order Ng step of four iterates [n_depth][n_col], x0 the newest -> (x, a, b); non-finite where it is to be skipped"""
    dt = x0.dtype.type
    with np.errstate(all="ignore"):
        q1 = (x0 - dt(2) * x1) + x2
        q2 = ((x0 - x1) - x2) + x3
        q3 = x0 - x1
        A1, B1, C1, B2, C2 = (_sum(p, lanes) for p in (q1 * q1, q1 * q2, q1 * q3, q2 * q2, q2 * q3))
        det = A1 * B2 - B1 * B1
        a = (C1 * B2 - C2 * B1) / det
        b = (C2 * A1 - C1 * B1) / det
        return (((dt(1) - a) - b) * x0 + a * x1) + b * x2, a, b


def iterate_ng(G, x0, tol=None, max_iter=None, options=None, counts=None):
    """x <- x + G(x) per column of x0 [n_depth][n_col] with the rule above.  G maps the whole plane to the whole plane, column by column
    independently.  options: start, period, accelerate, lanes, strikes (the device has 2; 1 and 0, no safeguard, are the variants of
    profiles/scattering_ng_classes.json) and judge ("period", the device's; "every": at every update of the period, another variant
    of that table).  counts [n_col]: column i takes exactly counts[i] updates (no stopping rule, status 0).  -> dict(x, iterations, status, change, accelerations, switched_off): switched_off is the update at which the
    safeguard sent the column back to the plain iteration, 0 where it never did."""
    o = dict(DEFAULTS)
    o.update(options or {})
    unknown = set(o) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"unknown option {sorted(unknown)}")
    start, period, lanes, strikes = int(o["start"]), int(o["period"]), int(o["lanes"]), int(o["strikes"])
    if o["accelerate"] and (start < 4 or period < 1):
        raise ValueError("start >= 4 and period >= 1")
    x = np.array(x0, copy=True)
    dt = x.dtype.type
    n_col = x.shape[1]
    with np.errstate(all="ignore"):
        live = np.ones(n_col, dtype=bool)
        iterations, status, change = np.zeros(n_col, dtype=np.int32), np.ones(n_col, dtype=np.int32), np.zeros(n_col, dtype=x.dtype)
        if counts is not None:
            counts = np.asarray(counts)
            live = counts > 0
            status[:] = 0
        n_max = int(counts.max()) if counts is not None else int(max_iter)
        ring = np.zeros((3,) + x.shape, dtype=x.dtype)  # the three iterates before the current one; ring[head] is the latest of them
        head = 0
        held = np.ones(n_col, dtype=np.int64)           # iterates of history, the current one included
        since = np.full(n_col, period, dtype=np.int64)  # updates since the last extrapolation
        on = np.full(n_col, bool(o["accelerate"]))
        probation = np.zeros(n_col, dtype=bool)
        reference = np.zeros(n_col, dtype=x.dtype)
        fallback = np.zeros_like(x)
        accelerations, switched_off = np.zeros(n_col, dtype=np.int32), np.zeros(n_col, dtype=np.int32)
        streak = np.zeros(n_col, dtype=np.int64)
        every = o["judge"] == "every"
        for n in range(1, n_max + 1):
            if not live.any():
                break
            dx = G(x)
            new = x + dx
            finite = np.isfinite(dx).all(axis=0)
            cd = np.where(finite, np.abs(dx).max(axis=0), dt(np.inf))
            cs = np.abs(new).max(axis=0)
            iterations[live], change[live] = n, cd[live]
            status[live & ~finite] = 2
            upd = live & finite
            head = (head + 1) % 3
            ring[head][:, upd] = x[:, upd]  # (the ring turns for every column alike; a frozen column's slots are never read again)
            x[:, upd] = new[:, upd]
            held[upd] += 1
            since[upd] += 1
            if counts is None:
                done = upd & (cd <= dt(tol) * cs)
                status[done] = 0
                live = upd & ~done
            else:
                live = upd & (counts > n)
            # the safeguard: judged once per extrapolation, a whole period after it
            judged = live & on & probation & ((since >= period) | every)
            fail = judged & ~(cd < reference)
            streak[judged & ~fail] = 0
            streak[fail] += 1
            back = fail & (streak >= strikes) if strikes > 0 else fail & False
            if back.any():
                x[:, back] = fallback[:, back]
                on[back] = False
                switched_off[back] = n
            probation &= ~(since >= period)
            # the extrapolation
            want = live & on & ~probation & (n >= start) & (n < n_max) & (since >= period) & (held >= 4)
            if want.any():
                e, _, _ = extrapolate(x[:, want], ring[head][:, want], ring[(head + 2) % 3][:, want], ring[(head + 1) % 3][:, want], lanes)
                ok = np.isfinite(e).all(axis=0)
                idx = np.flatnonzero(want)[ok]
                fresh = idx[streak[idx] == 0]
                fallback[:, fresh] = x[:, fresh]
                reference[fresh] = cd[fresh]
                x[:, idx] = e[:, ok]
                held[idx], since[idx], probation[idx] = 1, 0, True
                accelerations[idx] += 1
    return dict(x=x, iterations=iterations, status=status, change=change, accelerations=accelerations, switched_off=switched_off)


# ---- the two fixed points ------------------------------------------------------------------------------------------------------------
def forward_G(op, w, B):
    """scattering_reference.iterate's update, operation for operation -> (G, x0)"""
    dt = op.dtype
    B, w = np.asarray(B).astype(dt), np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        thermal = (1 - w) * B
        inv = 1 / (1 - w * R.clamp01(op.diagonal(), dt))
    return (lambda S: ((thermal + w * op.J(S)) - S) * inv), B.copy()


def adjoint_G(op, w, c):
    """scattering_adjoint_reference.iterate's update, operation for operation -> (G, x0)"""
    dt = op.dtype
    c, w = np.asarray(c).astype(dt), np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        inv = 1 / (1 - w * R.clamp01(op.diagonal(), dt))
    return (lambda y: ((c + A.transposed(op, w * y)) - y) * inv), c.copy()


def dense_forward_G(lam, diagonal, w, B):
    """the forward fixed point with the dense operator lam [row][column] of ONE grid shared by all columns -> (G, x0)"""
    dt = lam.dtype.type
    B, w = np.asarray(B).astype(dt), np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        thermal = (1 - w) * B
        inv = 1 / (1 - w * R.clamp01(diagonal, dt))
    return (lambda S: ((thermal + w * (lam @ S)) - S) * inv), B.copy()


def dense_adjoint_G(lam, diagonal, w, c):
    dt = lam.dtype.type
    c, w = np.asarray(c).astype(dt), np.asarray(w).astype(dt)
    lamT = np.ascontiguousarray(lam.T)
    with np.errstate(all="ignore"):
        inv = 1 / (1 - w * R.clamp01(diagonal, dt))
    return (lambda y: ((c + lamT @ (w * y)) - y) * inv), c.copy()


def scatter_source_ng(op, w, B, tol=None, max_iter=None, options=None, counts=None):
    G, x0 = forward_G(op, w, B)
    out = iterate_ng(G, x0, tol, max_iter, options, counts)
    out["S"] = out["x"]
    return out


def scatter_response_ng(op, w, c, tol=None, max_iter=None, options=None, counts=None):
    G, x0 = adjoint_G(op, w, c)
    out = iterate_ng(G, x0, tol, max_iter, options, counts)
    out["y"] = out["x"]
    return out


# ---- the column set --------------------------------------------------------------------------------------------------------------------
NG_GRIDS = [(57, 1e-4, 1e3), (57, 1e-6, 1e2), (20, 1e-3, 1e2), (9, 1e-2, 1e2), (4, 0.1, 10.0)]  # (points, tau range)
NG_ANGLES = (3, 20)
NG_UNIFORM = (0.5, 0.9, 0.99, 0.999, 0.9999, 0.99999)
NG_ALBEDOS = tuple(f"{a:g}" for a in NG_UNIFORM) + ("rising", "random", "random high")
NG_SOURCES = ("flat", "planck-like")
# (albedo, source) per column of every grid: 18 columns
NG_COLUMNS = [(a, s) for s in NG_SOURCES for a in NG_ALBEDOS]
TOL, MAX_ITER = 1e-12, 4000


def albedo_column(name, n, seed=3):
    """row 0 is the deepest point; x runs from 0 there to 1 at the surface"""
    x = np.arange(n) / (n - 1.0)
    if name == "rising":
        return 0.05 + 0.949 * x ** 2
    if name == "random":
        return np.random.default_rng(seed).uniform(0.0, 0.9999, n)
    if name == "random high":
        return np.random.default_rng(seed + 1).uniform(0.9, 0.9999, n)
    return np.full(n, float(name))


def source_column(name, n):
    x = np.arange(n) / (n - 1.0)
    return np.ones(n) if name == "flat" else 10.0 ** (4.0 * (1.0 - x))


def problem(n, lo, hi, n_theta, columns=None):
    """the columns of one grid as a device problem (alpha = 1: the gaps' lengths are their optical depths), in the shape of
    test_gpu_scattering.grid_problem"""
    from stardis_amd import ops, synth

    columns = NG_COLUMNS if columns is None else columns
    tau, dtau = R.log_grid(n, lo, hi)
    thetas, weights = synth.thetas_and_weights(n_theta)
    w = np.stack([albedo_column(a, n) for a, _ in columns], axis=1)
    B = np.stack([source_column(s, n) for _, s in columns], axis=1)
    n_nu = len(columns)
    return types.SimpleNamespace(n_depth=n, n_theta=n_theta, n_nu=n_nu, tau=tau, thetas=thetas, weights=weights, m=ops.mean_weights(thetas, weights),
                                 ray=dtau.reshape(-1, 1) / np.cos(thetas), alphas=np.ones((n, n_nu)), albedo=np.ascontiguousarray(w),
                                 B=np.ascontiguousarray(B), nus=np.linspace(7.5e14, 3.0e14, n_nu), temps=np.linspace(9500.0, 3900.0, n),
                                 columns=list(columns))


def cotangents(n, n_col, seed=17):
    """cotangents over three decades"""
    return 10.0 ** np.random.default_rng(seed).uniform(-1.5, 1.5, (n, n_col))
