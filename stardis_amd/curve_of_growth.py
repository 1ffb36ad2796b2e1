"""Curve-of-growth inversion: from measured equivalent widths to offsets in log gf (or in the abundance of a species that has the line
alone).  Pure host code over a callable; SpectralSynthesizer.fit_equivalent_widths is solve() over
SpectralSynthesizer.equivalent_widths, where one evaluation of `points` trial strengths for every line is one device call.

The isolated-line equivalent width W(s) of a line whose strength is scaled by s grows with s — linearly while the line is weak, as the
square root of ln s on the flat part, as sqrt(s) once the damping wings carry it.  No derivative is used: the reference's line windows
make W a function of s with small steps (the window's half-width is an integer), and a bracket does not care."""
import collections

import numpy as np

LN10 = float(np.log(10.0))

Solution = collections.namedtuple("Solution", "delta_log_gf bracket W converged")
Solution.__doc__ = """delta_log_gf (n,): the offset in dex at which W equals W_obs, interpolated linearly in (ln s, ln W) between the ends of
the final bracket (NaN where W_obs was not bracketed by the initial span); bracket (n, 2): that bracket in dex, lower end first; W (n,):
the equivalent width the evaluator gives at delta_log_gf; converged (n,): the bracket is narrower than tol, and every pass found its
samples monotone and W_obs between two of them."""


def solve(evaluate, W_obs, span=2.0, points=5, tol=1e-3, max_iter=8):
    """evaluate(ln_strength (n, K)) -> W (n, K): the equivalent widths of n lines at K natural-log strength offsets each.
    W_obs (n,): the measured widths, in the evaluator's unit.  Each pass evaluates `points` strengths per line, equally spaced in dex
    across the line's current bracket (at first [-span, +span] dex), and keeps the sub-interval whose ends' widths bracket W_obs; it
    stops when every bracket of a line still in play is below `tol` dex, or after max_iter passes.  A line whose W_obs lies outside the
    widths of the initial span, or whose samples are not strictly increasing, leaves the iteration with converged = False."""
    W_obs = np.ascontiguousarray(W_obs, dtype=np.float64).reshape(-1)
    n, points = W_obs.size, int(points)
    if points < 2 or not span > 0 or not tol > 0 or max_iter < 1:
        raise ValueError("solve: need points >= 2, span > 0, tol > 0 and max_iter >= 1")
    lo, hi = np.full(n, -float(span)), np.full(n, float(span))
    W_lo, W_hi = np.full(n, np.nan), np.full(n, np.nan)
    ok = np.ones(n, dtype=bool)  # still bracketed and monotone
    frac = np.linspace(0.0, 1.0, points)
    rows = np.arange(n)
    for _ in range(int(max_iter)):
        grid = lo[:, None] + (hi - lo)[:, None] * frac[None, :]  # dex
        grid[:, -1] = hi  # (the ends exactly: a bracket never grows by rounding)
        W = np.asarray(evaluate(np.ascontiguousarray(grid * LN10)), dtype=np.float64).reshape(n, points)
        monotone = (np.diff(W, axis=1) > 0).all(axis=1)
        inside = (W[:, 0] <= W_obs) & (W_obs <= W[:, -1])
        ok &= monotone & inside
        # the sub-interval [k, k + 1] with W[k] <= W_obs <= W[k + 1] (the last such k)
        k = np.clip((W <= W_obs[:, None]).sum(axis=1) - 1, 0, points - 2)
        new_lo, new_hi = grid[rows, k], grid[rows, k + 1]
        lo, hi = np.where(ok, new_lo, lo), np.where(ok, new_hi, hi)
        W_lo, W_hi = np.where(ok, W[rows, k], W_lo), np.where(ok, W[rows, k + 1], W_hi)
        if not ok.any() or ((hi - lo)[ok] < tol).all():
            break
    with np.errstate(all="ignore"):
        t = (np.log(W_obs) - np.log(W_lo)) / (np.log(W_hi) - np.log(W_lo))
    t = np.where(np.isfinite(t), np.clip(t, 0.0, 1.0), 0.5)
    delta = np.where(np.isfinite(W_lo), lo + (hi - lo) * t, np.nan)
    delta = np.minimum(np.maximum(delta, lo), hi)  # (NaN stays NaN)
    at = np.where(np.isfinite(delta), delta, 0.0)
    W_at = np.asarray(evaluate(np.ascontiguousarray((at * LN10)[:, None])), dtype=np.float64).reshape(n)
    W_at = np.where(np.isfinite(delta), W_at, np.nan)
    return Solution(delta, np.stack([lo, hi], axis=1), W_at, ok & ((hi - lo) < tol))
