"""The instrument model (include/stardis_hip.h, sdx_observe_dev and sdx_observe_adjoint_dev) judged against an extended-precision
evaluation of its own definition, on inputs chosen to hurt.

truth() and adjoint_truth() evaluate the definition with mpmath (DPS digits).  What the header defines as single fp64 operations —
x_i = lambdas[i] D, the trapezoid weights h_i, lo_j, hi_j, covered_j and the membership lo_j <= x_i <= hi_j — is formed in fp64,
correctly rounded on both sides, so membership is exact even for a point on a window's edge; a, b, the three branches of r, the
products and both sums are extended.  The fp64 restatement stays observe_reference.observe / observe_adjoint_reference.adjoint.

A kernel is judged class by class: no further from the truth than
    allowance_j = FACTOR d_ref(class) + (U Lambda_j / A_j + T_j + 8) 2^-53
of A_j, the sum of the absolute terms of the quotient (cancellation is not charged).  d_ref is the restatement's own distance (the
definition's accuracy in fp64: for a pixel much narrower than sigma the difference of two erfc cancels and an argument's rounding is
amplified by 2 p^2), Lambda_j what one unit of 2^-53 |value| in every erf / erfc does to the quotient, U the measured error of the
special functions in that unit, T_j the depth of the sum and 8 the roundings of x, h, w, the product and the quotient.
The adjoint is judged per grid point by the same formula against the point's own absolute terms: T_i the depth of the point's sum,
Lambda_i the effect of a unit in erf / erfc through w_ij, den_j and (for w_reference) out_j.
hostile() draws the inputs; ulp_arguments() / ulp_figure() measure U.

Used by tests/test_observe_truth_cpu.py (the judge can fail; the restatement alone passes), tests/test_gpu_observe_truth.py,
tests/test_gpu_observe_tangent.py (the bound on obs_response) and scripts/observe_truth_table.py.  No GPU work here."""
import functools
import json
import math
import os
import types
import zlib

import mpmath
import numpy as np

import formal_solution_truth as FT
import observe_adjoint_reference as aref
import observe_reference as oref

FACTOR = FT.FACTOR
PER_CLASS = 16  # pixels per case: a class's figure is the largest over them, so one lucky rounding is not what gets measured
EPS = 2.0 ** -53
DPS = 32
ROUNDINGS = 8  # x, h, a, b, the difference, w, the product, the quotient
M = mpmath.mp.clone()  # a context of its own: other tests set mpmath.mp.dps
M.dps = DPS
NS = types.SimpleNamespace
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "observe_truth_classes.json")

RECORD = []  # what the GPU tests measured in this process: dicts, see judge(); scripts/observe_truth_table.py writes them out


# ---- the definition in extended precision ------------------------------------------------------------------------------------------
def mp_response(e0, e1, x, sigma):
    """-> (r, (|E1| + |E2|) / 2): the header's three branches at the context's precision from fp64 e0, e1, x, sigma, and the mean
    magnitude of the two erf / erfc values the branch subtracts"""
    s2 = M.mpf(float(sigma)) * M.sqrt(2)
    x = M.mpf(float(x))
    a, b = (M.mpf(float(e0)) - x) / s2, (M.mpf(float(e1)) - x) / s2
    if a > 0:
        E1, E2 = M.erfc(a), M.erfc(b)
    elif b < 0:
        E1, E2 = M.erfc(-b), M.erfc(-a)
    else:
        E1, E2 = M.erf(b), M.erf(a)
    return (E1 - E2) / 2, (abs(E1) + abs(E2)) / 2


def header_weights(x):
    """h_i of the header, each one rounded fp64 subtraction and an exact halving: (x[i+1] - x[i-1]) / 2, at the ends (x[1] - x[0]) / 2 and
    (x[n-1] - x[n-2]) / 2.  Written from the header, not taken from observe_reference: the truth shares no code with the restatement."""
    n = x.size
    return np.array([(x[min(i + 1, n - 1)] - x[max(i - 1, 0)]) / 2 for i in range(n)])


def header_windows(x, edges, sigma):
    """-> (i0, i1, covered) of the header: lo_j = edges[j] - 8 sigma[j], hi_j = edges[j+1] + 8 sigma[j] in fp64, covered_j = lo_j >= x_0 and
    hi_j <= x_{n-1}, and the members lo_j <= x_i <= hi_j by the comparison itself (one run x[i0:i1] on an ascending grid; an empty window
    has i0 == i1)"""
    i0, i1, covered = (np.zeros(sigma.size, dtype=np.int64) for _ in range(3))
    for j in range(sigma.size):
        reach = 8.0 * sigma[j]
        lo, hi = edges[j] - reach, edges[j + 1] + reach
        covered[j] = lo >= x[0] and hi <= x[-1]
        member = np.flatnonzero((lo <= x) & (x <= hi))
        if member.size:
            assert member[-1] - member[0] + 1 == member.size
            i0[j], i1[j] = member[0], member[-1] + 1
    return i0, i1, covered.astype(bool)


def forward_lanes(x, edges, sigma):
    """-> W per pixel (8 or 64; 0: the estimate is too close to its threshold to call): the lanes k_observe gives a pixel, from the
    windows' expected lengths at the grid's mean spacing, by groups of eight pixels (sdx_kernels.h)"""
    expected = (edges[1:] - edges[:-1] + 16.0 * sigma) * float(x.size - 1) / (x[-1] - x[0])
    W = np.empty(expected.size, dtype=np.int64)
    for first in range(0, expected.size, 8):
        e = expected[first:first + 8]
        W[first:first + 8] = 0 if np.any(np.abs(e / 32.0 - 1.0) < 1e-9) else (64 if np.any(e > 32.0) else 8)
    return W


def depth(count, W):
    """ceil(count / W) + log2 W: serial per lane, then a butterfly; W = 0: the larger of the two mappings'"""
    d = {w: np.ceil(np.asarray(count) / w) + math.log2(w) for w in (8, 64)}
    return np.where(np.asarray(W) == 8, d[8], np.where(np.asarray(W) == 64, d[64], np.maximum(d[8], d[64])))


def rows(lambdas, edges, sigma, doppler=1.0):
    """-> NS(x, h, i0, i1, covered, w, eh): per covered pixel the extended weights w_ij = r_ij h_i over its window x[i0:i1] and
    eh_ij = (|E1| + |E2|) / 2 h_i (None for an uncovered pixel).  x, h and the windows are fp64, as the header defines them."""
    lam, edges = np.asarray(lambdas, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (edges.size - 1,)))
    x = lam * float(doppler)
    h = header_weights(x)
    i0, i1, covered = header_windows(x, edges, sigma)
    w, eh = [None] * sigma.size, [None] * sigma.size
    for j in np.flatnonzero(covered):
        pairs = [mp_response(edges[j], edges[j + 1], x[i], sigma[j]) for i in range(i0[j], i1[j])]
        hh = [M.mpf(float(v)) for v in h[i0[j]:i1[j]]]
        w[j] = [p[0] * v for p, v in zip(pairs, hh)]
        eh[j] = [p[1] * v for p, v in zip(pairs, hh)]
    return NS(x=x, h=h, i0=i0, i1=i1, covered=covered, w=w, eh=eh, edges=edges, sigma=sigma, lanes=forward_lanes(x, edges, sigma))


def _mpv(a):
    return [M.mpf(float(v)) for v in a]


def truth(lambdas, flux, edges, sigma, doppler=1.0, reference=None, rows_=None):
    """-> NS with, per pixel (NaN where the grid does not cover the window):
         out      the definition's value (mpf; out64 its fp64 rounding),
         A        (sum_i |w_ij f_i| + |out_j| sum_i |w_ij g_i|) / |den_j|: what every distance is taken against,
         Lam      (sum_i eh_ij (|f_i| + |out_j| |g_i|)) / |den_j|: the error of out_j per unit of 2^-53 |value| in erf and erfc,
         T        the depth of the kernel's sum;  den, kappa = sum |w g| / |den|, Lam_den = sum eh |g| / |den|  (for the adjoint)"""
    R = rows_ if rows_ is not None else rows(lambdas, edges, sigma, doppler)
    f = np.asarray(flux, dtype=np.float64)
    g = None if reference is None else np.asarray(reference, dtype=np.float64)
    n_pix = R.sigma.size
    nan = M.mpf("nan")
    t = NS(rows=R, out=[nan] * n_pix, den=[nan] * n_pix, A=[nan] * n_pix, Lam=[nan] * n_pix, kappa=[nan] * n_pix, Lam_den=[nan] * n_pix,
           n_window=np.where(R.covered, R.i1 - R.i0, 0))
    for j in np.flatnonzero(R.covered):
        w, eh = R.w[j], R.eh[j]
        fj = _mpv(f[R.i0[j]:R.i1[j]])
        gj = [M.mpf(1)] * len(w) if g is None else _mpv(g[R.i0[j]:R.i1[j]])
        den = M.fdot(w, gj)
        out = M.fdot(w, fj) / den
        abs_g = M.fsum(abs(a * b) for a, b in zip(w, gj))
        t.out[j], t.den[j] = out, den
        t.A[j] = (M.fsum(abs(a * b) for a, b in zip(w, fj)) + abs(out) * abs_g) / abs(den)
        t.Lam[j] = M.fsum(e * (abs(a) + abs(out) * abs(b)) for e, a, b in zip(eh, fj, gj)) / abs(den)
        t.kappa[j] = abs_g / abs(den)
        t.Lam_den[j] = M.fsum(e * abs(b) for e, b in zip(eh, gj)) / abs(den)
    t.out64 = np.array([float(v) for v in t.out])
    t.T = depth(t.n_window, R.lanes)
    t.ratio = np.array([float(l / a) if a == a and a != 0 else np.nan for l, a in zip(t.Lam, t.A)])
    return t


ADJOINT_DEPTH = 7.0  # at most PER_CLASS pixels per point: ceil(16 / 8) + 3 = 5 with eight lanes, ceil(16 / 64) + 6 = 7 with a wave


def adjoint_truth(lambdas, c, edges, sigma, doppler=1.0, flux=None, reference=None, nus=None, rows_=None):
    """-> NS(w_flux, scale, ratio, T[, w_ref, scale_ref, ratio_ref, T_ref]) per grid point, lists of mpf / fp64 arrays:
         w_flux, w_ref   the definition's two outputs (w_ref only with a reference),
         scale, ...      the sums of the absolute values of the point's terms, as observe_adjoint_reference.adjoint returns them,
         ratio, ...      Lambda_i / scale_i, Lambda_i the error per unit of 2^-53 |value| in erf and erfc: through w_ij itself, through
                         den_j and, for w_ref, through out_j (the forward's Lambda_j: the cancellation inside out_j is not charged),
         T, ...          the depth of the point's own sum (two more roundings with nus).
    A point whose scale is 0 has no term: the kernel's value there is exactly 0."""
    lam = np.asarray(lambdas, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    n = lam.size
    R = rows_ if rows_ is not None else rows(lam, edges, sigma, doppler)
    normal = reference is not None
    fw = truth(lam, flux if flux is not None else np.ones(n), edges, sigma, doppler, reference=reference, rows_=R)
    zero = M.mpf(0)
    acc = {k: [zero] * n for k in ("wf", "sf", "lf", "wr", "sr", "lr")}
    for j in np.flatnonzero(R.covered):
        a = M.mpf(float(c[j])) / fw.den[j]
        b = -fw.out[j] * a
        for k, i in enumerate(range(R.i0[j], R.i1[j])):
            w, eh = R.w[j][k], R.eh[j][k]
            t = w * a
            acc["wf"][i] += t
            acc["sf"][i] += abs(t)
            acc["lf"][i] += abs(a) * (eh + abs(w) * fw.Lam_den[j])
            if normal:
                u = w * b
                acc["wr"][i] += u
                acc["sr"][i] += abs(u)
                acc["lr"][i] += abs(b) * (eh + abs(w) * fw.Lam_den[j]) + abs(t) * fw.Lam[j]
    own = ADJOINT_DEPTH + (2.0 if nus is not None else 0.0)
    k = [M.mpf(1)] * n if nus is None else [M.mpf(float(v)) / M.mpf(float(l)) for v, l in zip(np.asarray(nus, dtype=np.float64), lam)]

    def finish(w, s, l):
        scale = np.array([float(a * abs(b)) for a, b in zip(s, k)])
        ratio = np.array([float(a / b) if b != 0 else 0.0 for a, b in zip(l, s)])
        return [a * b for a, b in zip(w, k)], scale, ratio, np.full(n, own)

    res = NS(forward=fw)
    res.w_flux, res.scale, res.ratio, res.T = finish(acc["wf"], acc["sf"], acc["lf"])
    if normal:
        res.w_ref, res.scale_ref, res.ratio_ref, res.T_ref = finish(acc["wr"], acc["sr"], acc["lr"])
    return res


def distance(got, exact, scale):
    """|got - exact| / scale per element, the difference formed at the context's precision; where scale is 0 the element has no term:
    0 where got is 0 too, inf otherwise"""
    got, scale = np.asarray(got, dtype=np.float64), np.asarray([float(s) for s in scale])
    out = np.empty(got.size)
    for i in range(got.size):
        if not np.isfinite(got[i]):
            out[i] = np.inf
        elif scale[i] == 0:
            out[i] = 0.0 if got[i] == 0 else np.inf
        else:
            out[i] = float(abs(M.mpf(float(got[i])) - exact[i]) / M.mpf(float(scale[i])))
    return out


def allowance(d_ref, ratio, T, U):
    """what a kernel's distance may be: FACTOR d_ref(class) + (U Lambda / A + T + 8) 2^-53, per pixel (or point)"""
    return FACTOR * float(d_ref) + (float(U) * np.asarray(ratio) + np.asarray(T) + ROUNDINGS) * EPS


def judge(case, quantity, got, exact, scale, ratio, T, restated, U, label="kernel", record=RECORD, d_ref=None):
    """print, record, then assert: every element of `got` within its allowance; `restated` is the fp64 restatement's value of the
    same quantity, whose largest distance over the case is d_ref (d_ref given: taken from elsewhere, e.g. another seed).
    -> (the kernel's distances, the restatement's)"""
    d_got, d_res = distance(got, exact, scale), distance(restated, exact, scale)
    d_ref = float(np.max(d_res)) if d_ref is None else float(d_ref)
    assert np.isfinite(d_ref) and np.all(np.isfinite(d_res)), (case, quantity, "the restatement itself left the range")
    allow = allowance(d_ref, ratio, T, U)
    worst = int(np.argmax(d_got / allow))
    print(f"{case}, {quantity}: {label} {float(np.max(d_got)):.3e}, restatement {float(np.max(d_res)):.3e} (d_ref {d_ref:.3e}), allowance "
          f"{float(allow.min()):.3e} .. {float(allow.max()):.3e}, worst {label} / allowance {float(d_got[worst] / allow[worst]):.3e} at {worst}")
    if record is not None:
        record.append(dict(case=case, quantity=quantity, label=label, kernel=float(np.max(d_got)), restatement=float(np.max(d_res)),
                           allowance=float(allow[worst]), worst_ratio=float(d_got[worst] / allow[worst])))
    assert np.all(d_got <= allow), (case, quantity, worst, float(d_got[worst]), float(allow[worst]))
    return d_got, d_res


def within(got, exact, scale, ratio, T, d_ref, U):
    """the judge's verdict without the assert (for the mutants)"""
    return bool(np.all(distance(got, exact, scale) <= allowance(d_ref, ratio, T, U)))


# ---- the error of erf and erfc, in units of 2^-53 |value| -------------------------------------------------------------------------------
def ulp_arguments():
    """-> (p, a_erfc, b_erfc, a_erf, b_erf): the fp64 arguments p = fl(a' / fl(sqrt 2)) at which the response routine evaluates the
    special functions for a' = fl(k / 64 sqrt 2), k = 0 .. 544 (p from 0 to 8.5), and the edges to pass with x = 0, sigma = 1:
    (a', a' + 40) gives r = erfc(p) / 2 (the far erfc is exactly 0), (0, a') gives r = erf(p) / 2."""
    a = np.arange(0, 545) / 64.0 * np.sqrt(2.0)
    p = a / np.sqrt(2.0)
    return p, a, a + 40.0, np.zeros(a.size), a


def ulp_figure(p, erfc_values, erf_values):
    """-> (worst, where): the largest |value - exact| / (2^-53 |exact|) over both functions at the fp64 arguments p, against 50 digits"""
    worst, where = 0.0, ""
    with mpmath.workdps(50):
        for name, fn, values in (("erfc", mpmath.erfc, erfc_values), ("erf", mpmath.erf, erf_values)):
            for x, v in zip(p, values):
                exact = fn(mpmath.mpf(float(x)))
                if exact == 0:
                    assert v == 0, (name, x, v)
                    continue
                u = float(abs(mpmath.mpf(float(v)) - exact) / (abs(exact) * mpmath.mpf(2) ** -53))
                if u > worst:
                    worst, where = u, f"{name}({float(x)!r})"
    return worst, where


def chosen_U(worst):
    """the worst figure rounded up to the next integer, plus 1: one unlucky argument outside the sample is not a kernel failure"""
    return int(math.ceil(worst)) + 1


U_OVERRIDE = None  # scripts/observe_truth_table.py sets it to what it has just measured, before it runs the tests


def device_U():
    """the U recorded for the device's erf / erfc in profiles/observe_truth_classes.json (scripts/observe_truth_table.py)"""
    if U_OVERRIDE is not None:
        return int(U_OVERRIDE)
    with open(TABLE) as f:
        return int(json.load(f)["U"])


# ---- hostile inputs ------------------------------------------------------------------------------------------------------------------
SIGMA = 0.05
CENTRE = 6550.0
BASES = ("benign", "tail_spike", "deep_core", "narrow_1e-2", "narrow_1e-4", "narrow_1e-6", "narrow_1e-2_spike", "narrow_1e-4_spike",
         "narrow_1e-6_spike", "wide_30", "wide_1e3", "wide_1e4", "on_edge", "signed", "range_up", "range_down", "spacing", "spacing_ends",
         "far_912_red3000", "far_912_blue30000", "far_1e5_blue3000", "far_1e5_red30000")
CASES = tuple(b + s for b in BASES for s in ("", "+ref"))


def _edges(widths, sigma, centre):
    widths = np.asarray(widths, dtype=np.float64) * sigma
    return centre - widths.sum() / 2 + np.r_[0.0, np.cumsum(widths)]


def _grid(rng, edges, sigma, n, extra=()):
    """n distinct observed wavelengths, irregular, that reach 2.5 sigma past every window; `extra` are among them"""
    lo, hi = edges[0] - 10.5 * sigma, edges[-1] + 10.5 * sigma
    return np.unique(np.r_[lo, hi, rng.uniform(lo, hi, n - 2 - len(extra)), np.asarray(extra, dtype=np.float64)])


def _noise(rng, n):
    return 1.0 + 0.1 * rng.standard_normal(n)


def _benign(rng, sigma=SIGMA, centre=CENTRE, widths=None, n=300):
    edges = _edges(np.ones(PER_CLASS) if widths is None else widths, sigma, centre)
    x = _grid(rng, edges, sigma, n)
    return x, _noise(rng, x.size), edges, np.full(PER_CLASS, sigma)


def _tail_spike(rng):
    """pixels 15 sigma wide; every odd pixel holds one point of 1e12 .. 1e14 that lies 7.0 .. 7.98 sigma above the even pixel below it and
    as far below the even pixel above it: both erfc branches, and beyond 7.9 sigma on either side"""
    edges = _edges(np.full(PER_CLASS, 15.0), SIGMA, CENTRE)
    u = rng.uniform(7.1, 7.9, PER_CLASS // 2)
    u[0], u[1] = 7.95, 7.05
    spikes = edges[1::2][:PER_CLASS // 2] + u * SIGMA
    x = _grid(rng, edges, SIGMA, 600, spikes)
    f = _noise(rng, x.size)
    f[np.searchsorted(x, spikes)] = 10.0 ** rng.uniform(12.0, 14.0, spikes.size)
    return x, f, edges, np.full(PER_CLASS, SIGMA)


DEEP_CORE_HALF_WIDTHS = (2.0, 4.0, 6.0, 7.0)


def _deep_core(rng):
    """pixels one sigma wide between fillers of 12: 1e-12 over every narrow pixel and d sigma to either side, near 1 elsewhere, d cycling
    through DEEP_CORE_HALF_WIDTHS.  With d = 2 the numerator is carried by weights of 1e-2, which an erf difference still gives to
    1e-14 (tests/test_observe_truth_cpu.py measures a wrong response at a quarter of the allowance there); with d = 6 and 7 it rests
    on weights of 1e-9 .. 1e-15, which only the erfc branches give to their relative accuracy."""
    edges = _edges(np.tile([1.0, 12.0], PER_CLASS // 2), SIGMA, CENTRE)
    x = _grid(rng, edges, SIGMA, 600)
    f = _noise(rng, x.size)
    for k, j in enumerate(range(0, PER_CLASS, 2)):
        d = DEEP_CORE_HALF_WIDTHS[k % len(DEEP_CORE_HALF_WIDTHS)] * SIGMA
        f[(x >= edges[j] - d) & (x <= edges[j + 1] + d)] = 1e-12
    return x, f, edges, np.full(PER_CLASS, SIGMA)


def _narrow(rng, ratio, spike):
    """nine pixels `ratio` sigma wide between fillers of three; with `spike`, a point of 1e12 .. 1e14 at 7.0 .. 7.9 sigma below the
    first pixel, above the last and above the ninth"""
    edges = _edges([ratio, 3.0] * 7 + [ratio, ratio], SIGMA, CENTRE)
    spikes = np.array([edges[0] - rng.uniform(7.0, 7.9) * SIGMA, edges[-1] + rng.uniform(7.0, 7.9) * SIGMA, edges[9] + rng.uniform(7.0, 7.9) * SIGMA])
    x = _grid(rng, edges, SIGMA, 300, spikes if spike else ())
    f = _noise(rng, x.size)
    if spike:
        f[np.searchsorted(x, spikes)] = 10.0 ** rng.uniform(12.0, 14.0, 3)
    return x, f, edges, np.full(PER_CLASS, SIGMA)


def _wide(rng, ratio):
    """pixels `ratio` sigma wide: 18 points within 8.5 sigma of every edge, 14 inside every pixel"""
    edges = _edges(np.full(PER_CLASS, ratio), SIGMA, CENTRE)
    near = np.concatenate([e + rng.uniform(-8.5, 8.5, 18) * SIGMA for e in edges])
    inside = np.concatenate([rng.uniform(a + 8.5 * SIGMA, b - 8.5 * SIGMA, 14) for a, b in zip(edges[:-1], edges[1:])])
    x = np.unique(np.r_[edges[0] - 10.5 * SIGMA, edges[-1] + 10.5 * SIGMA, near, inside])
    return x, _noise(rng, x.size), edges, np.full(PER_CLASS, SIGMA)


ON_EDGE_WIDTH = 17.0  # pixel width in sigma: wider than 16, so no window reaches the end of the next pixel but one's


def _on_edge(rng):
    """grid points exactly on every pixel edge (a == 0, b == 0) and one ulp to either side; and, for every SECOND pixel, grid points exactly
    on its lo_j and hi_j and one ulp to either side that carry 1e16 .. 1e17 times (the typical weight / their own).  The pixels are 17
    sigma wide, so an even pixel's window holds its own six end points and no other pixel's: the two members of either end carry a
    share of A_j that compares with the rest of the window, and the point one ulp outside would, were it taken for a member.  (The odd
    pixels hold those points in their cores; the adjoint's pixel vector `even` leaves them out, so that a point on lo_j has pixel j's
    term alone and the point one ulp below it none: an exact 0.)"""
    edges = _edges(np.full(PER_CLASS, ON_EDGE_WIDTH), SIGMA, CENTRE)
    sigma = np.full(PER_CLASS, SIGMA)
    ends = np.r_[(edges[:-1] - 8 * sigma)[::2], (edges[1:] + 8 * sigma)[::2]]  # lo_j, hi_j of the even pixels as the header rounds them
    triple = lambda v: np.r_[np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]  # noqa: E731
    x = _grid(rng, edges, SIGMA, 400 + 3 * (edges.size + ends.size), np.r_[triple(edges), triple(ends)])
    f = _noise(rng, x.size)
    h = header_weights(x)
    at = np.searchsorted(x, triple(ends))
    f[at] = 10.0 ** rng.uniform(16.0, 17.0, at.size) * (np.median(h) / h[at])
    for v in np.r_[edges, ends]:
        k = int(np.searchsorted(x, v))
        assert x[k] == v and x[k - 1] == np.nextafter(v, -np.inf) and x[k + 1] == np.nextafter(v, np.inf)
    i0, i1, _ = header_windows(x, edges, sigma)
    for j in range(0, PER_CLASS, 2):  # an even window: its own two members at either end, nobody else's end points
        inside = np.sort(at[(at >= i0[j]) & (at < i1[j])])
        assert inside.tolist() == [i0[j], i0[j] + 1, i1[j] - 2, i1[j] - 1] and x[i0[j]] == edges[j] - 8 * sigma[j] and x[i1[j] - 1] == edges[j + 1] + 8 * sigma[j]
    return x, f, edges, sigma


def _signed(rng):
    """flux of both signs, moved by the smallest change that leaves every pixel's numerator at 1e-6 of sum |w f|"""
    x, _, edges, sigma = _benign(rng, widths=np.full(PER_CLASS, 3.0))
    f = _noise(rng, x.size) * rng.choice([-1.0, 1.0], x.size)
    h = oref.trapezoid_weights(x)
    i0, i1, _ = oref.windows(x, edges, sigma)
    Wm = np.zeros((PER_CLASS, x.size), dtype=np.longdouble)
    for j in range(PER_CLASS):
        Wm[j, i0[j]:i1[j]] = oref.response(edges[j], edges[j + 1], x[i0[j]:i1[j]], sigma[j]) * h[i0[j]:i1[j]]
    sign = rng.choice([-1.0, 1.0], PER_CLASS)
    for _ in range(4):
        target = 1e-6 * sign * (np.abs(Wm) @ np.abs(f).astype(np.longdouble)).astype(np.float64)
        f = f + np.linalg.lstsq(Wm.astype(np.float64), target - (Wm @ f.astype(np.longdouble)).astype(np.float64), rcond=None)[0]
    cancel = np.abs(Wm @ f.astype(np.longdouble)) / (np.abs(Wm) @ np.abs(f).astype(np.longdouble))
    assert np.all((cancel > 0.5e-6) & (cancel < 2e-6)) and (f > 0).any() and (f < 0).any(), cancel
    return x, f, edges, sigma


def _window_count(x, e0, e1, s):
    return int(np.searchsorted(x, e1 + 8 * s, "right") - np.searchsorted(x, e0 - 8 * s, "left"))


SPACING_COUNTS = np.array([1, 2, 8, 9, 1, 2, 8, 9, 64, 65, 64, 65, 8, 9, 64, 65])


def _spacing(rng, ends):
    """spacings log-uniform over 3.5 decades (1e3 : 1 and more inside one window), two neighbours 4 ulp apart, pixels 1e-3 A wide whose sigma gives windows of exactly
    SPACING_COUNTS points: the first group eight lanes per pixel, the second a wave per pixel.  ends: the grid is cut to the union of
    the windows, with a point exactly on its lowest lo_j and one on its highest hi_j that carry 1e14 .. 1e15."""
    for _ in range(200):
        steps = 10.0 ** rng.uniform(0.0, 3.5, 499)
        x = CENTRE - 2.0 + np.r_[0.0, np.cumsum(steps)] * (4.0 / steps.sum())
        edges = CENTRE + rng.uniform(-0.3, 0.3) + 1e-3 * np.arange(PER_CLASS + 1)
        k = int(np.searchsorted(x, edges[-1])) + 5
        x = np.unique(np.r_[x, x[k] + 4 * np.spacing(x[k])])
        sigma = np.zeros(PER_CLASS)
        for j, want in enumerate(SPACING_COUNTS):
            a, b = 1e-7, 1.0
            for _ in range(200):
                s = math.sqrt(a * b)
                got = _window_count(x, edges[j], edges[j + 1], s)
                if got == want:
                    sigma[j] = s
                    break
                a, b = (s, b) if got < want else (a, s)
        if np.any(sigma == 0) or not np.array_equal(forward_lanes(x, edges, sigma), np.repeat([8, 64], 8)):
            continue
        i0, i1, _ = oref.windows(x, edges, sigma)
        if not any(np.diff(x[a:b]).max() >= 1e3 * np.sort(np.diff(x[a:b]))[1] for a, b in zip(i0, i1) if b - a >= 64):
            continue
        if not ends:
            assert np.array_equal(i1 - i0, SPACING_COUNTS) and np.min(np.diff(x)) == 4 * np.spacing(x[k])
            return x, _noise(rng, x.size), edges, sigma
        lo, hi = (edges[:-1] - 8 * sigma).min(), (edges[1:] + 8 * sigma).max()
        x = np.r_[lo, x[(x > lo) & (x < hi)], hi]
        f = _noise(rng, x.size)
        f[0], f[-1] = 10.0 ** rng.uniform(14.0, 15.0, 2)
        return x, f, edges, sigma
    raise AssertionError("no grid with the windows the spacing class asks for")


def _far(rng, centre, v):
    x, f, edges, sigma = _benign(rng, sigma=0.01, centre=centre, n=400)
    return x, f, edges, sigma, oref.doppler_factor(v)


_BUILDERS = {
    "benign": _benign, "tail_spike": _tail_spike, "deep_core": _deep_core, "on_edge": _on_edge, "signed": _signed,
    "range_up": _benign, "range_down": _benign, "spacing": lambda r: _spacing(r, False), "spacing_ends": lambda r: _spacing(r, True),
    "wide_30": lambda r: _wide(r, 30.0), "wide_1e3": lambda r: _wide(r, 1e3), "wide_1e4": lambda r: _wide(r, 1e4),
    "far_912_red3000": lambda r: _far(r, 912.0, 3000.0), "far_912_blue30000": lambda r: _far(r, 912.0, -30000.0),
    "far_1e5_blue3000": lambda r: _far(r, 1e5, -3000.0), "far_1e5_red30000": lambda r: _far(r, 1e5, 30000.0),
}
for _r in ("1e-2", "1e-4", "1e-6"):
    _BUILDERS[f"narrow_{_r}"] = functools.partial(_narrow, ratio=float(_r), spike=False)
    _BUILDERS[f"narrow_{_r}_spike"] = functools.partial(_narrow, ratio=float(_r), spike=True)


@functools.lru_cache(maxsize=None)
def hostile(name, seed=0):
    """-> (lambdas, flux, reference or None, edges, sigma, D) of the case `name` (one of CASES; `+ref`: the same grid, flux and detector
    with a positive reference), 16 pixels on a grid of at most 600 points.  The arrays are shared between callers: read-only."""
    base, _, ref = name.partition("+")
    rng = np.random.default_rng([seed, zlib.crc32(base.encode())])
    made = _BUILDERS[base](rng)
    x, f, edges, sigma = made[:4]
    D = made[4] if len(made) > 4 else 1.0
    lam = x / D
    g = 2.0 + 0.5 * np.sin(7.0 * lam) if ref else None
    if base.startswith("range"):
        f = f * (1e150 if base == "range_up" else 1e-150)
        g = None if g is None else g * 1e-150
    assert lam.size <= 600 and edges.size == PER_CLASS + 1 and np.all(np.diff(lam) > 0) and np.all(np.diff(lam * D) > 0) and np.all(np.diff(edges) > 0)
    # on the CPU, in fp64: every pixel covered, no denominator that cancels
    xs, h = lam * D, header_weights(lam * D)
    i0, i1, covered = header_windows(xs, edges, sigma)
    assert covered.all(), (name, covered)
    for j in range(PER_CLASS):
        w = oref.response(edges[j], edges[j + 1], xs[i0[j]:i1[j]], sigma[j]) * h[i0[j]:i1[j]]
        wg = w if g is None else w * g[i0[j]:i1[j]]
        assert i1[j] > i0[j] and abs(wg.sum()) >= 0.1 * np.abs(wg).sum() > 0, (name, j)
    for a in (lam, f, g, edges, sigma):
        if a is not None:
            a.setflags(write=False)
    return lam, f, g, edges, sigma, float(D)


@functools.lru_cache(maxsize=None)
def case_rows(base, seed=0):
    lam, _, _, edges, sigma, D = hostile(base, seed)
    return rows(lam, edges, sigma, D)


@functools.lru_cache(maxsize=None)
def case_truth(name, seed=0):
    """truth() of hostile(name, seed), once per process; the two variants of a case share their weights"""
    lam, f, g, edges, sigma, D = hostile(name, seed)
    return truth(lam, f, edges, sigma, D, reference=g, rows_=case_rows(name.partition("+")[0], seed))


C_KINDS = ("signed", "range", "far_tail")


def pixel_vector(name, kind, seed=0):
    """the adjoint's pixel vector c for the case: `signed` standard normal; `range` the same times 10^(-100 .. 100); `far_tail` nonzero
    on the detector's first and last pixel alone, so that the points in the middle of the detector and beyond its ends have terms
    only from pixels that see them in their far tail; `even` (on_edge's) zero on the odd pixels.  (range_up+ref: times 1e-160, and `range` is not for that case.)"""
    rng = np.random.default_rng([seed, zlib.crc32((name.partition("+")[0] + kind).encode())])
    c = rng.standard_normal(PER_CLASS)
    if kind == "range":
        c = c * 10.0 ** rng.uniform(-100.0, 100.0, PER_CLASS)
    elif kind == "far_tail":
        c[1:-1] = 0.0
    elif kind == "even":
        c[1::2] = 0.0
    if name == "range_up+ref":  # out is 1e300 there: w_reference = -out c / den w stays in range only for a small c
        c = c * 1e-160
    return c


def adjoint_kind(name):
    """the pixel vector a case's adjoint is judged with where one per case is run: the three kinds in turn over BASES"""
    if name.startswith("on_edge"):
        return "even"  # nonzero on the even pixels alone: the points on their windows' ends have that pixel's term and no other
    return "signed" if name.startswith("range_up") else C_KINDS[BASES.index(name.partition("+")[0]) % 3]


@functools.lru_cache(maxsize=None)
def case_adjoint_truth(name, kind="signed", with_nus=False, seed=0):
    lam, f, g, edges, sigma, D = hostile(name, seed)
    nus = nus_of(lam) if with_nus else None
    return adjoint_truth(lam, pixel_vector(name, kind, seed), edges, sigma, D, flux=f, reference=g, nus=nus, rows_=case_rows(name.partition("+")[0], seed))


def nus_of(lam):
    return 2.99792458e18 / np.asarray(lam, dtype=np.float64)


def restated_adjoint(name, kind="signed", with_nus=False, seed=0):
    """observe_adjoint_reference.adjoint on the case -> (w_flux, w_ref or None)"""
    lam, f, g, edges, sigma, D = hostile(name, seed)
    return aref.adjoint(lam, pixel_vector(name, kind, seed), edges, sigma, D, flux=f, reference=g, nus=nus_of(lam) if with_nus else None)[:2]
