"""The line opacity on hostile line lists, judged against an extended-precision evaluation of the reference's own sum.

truth() walks calc_alan_entries (opacities_solvers/base.py:487-592) term by term: the window of every (line, depth) from oracle.window
(the reference's rule in fp64, :556-575), x = delta_nu / doppler_width, y = gamma / (sqrt(pi) pi) / doppler_width and the Humlicek
region (voigt.py:31-44, :148) decided in fp64 exactly as the reference decides them, then the chosen region's rational (voigt.py:47-84)
and the sum in numpy longdouble.  hostile_lists() builds the lists: every item of a class sits ON a decision boundary of the line path
(class bounds 64 / 128 / 4096 / N_nu, the 10-point floor, a grid frequency, a grid end, a tile edge, a far-range bound, a 64- or
256-line stretch), with the window half-width dialled exactly by solving the fp64 rule for alpha.  A kernel is held to be no further
from the truth, point by point and relative to the truth, than bound(): four times the oracle's own distance plus the allowance the
suite already gives the hot Voigt routine.

Grids are exact: nus[i] = (K0 - i) 2^30 Hz (about 6.4e14 Hz, 1.07 GHz apart), so every grid frequency, every grid difference and
d_nu are exact in fp64 and a line can be placed on a grid frequency, or an ulp (0.125 Hz) beside it, on purpose.

Used by tests/test_line_opacity_truth_cpu.py (the reference alone meets the conditions the GPU tests rest on),
tests/test_gpu_line_opacity_truth.py (every route of the line path) and scripts/line_truth_table.py.
"""
import ctypes as C

import numpy as np

L = np.longdouble
CL = np.clongdouble
EXTENDED = bool(np.finfo(L).eps <= 1e-18)  # a host without an extended long double has no truth to offer: the GPU tests skip
SQRT_PI = 1.7724538509055159  # voigt.py:12
PI = 3.141592653589793

FACTOR = 4.0  # tests/formal_solution_truth.py FACTOR (scripts/fuzz_raytrace.py: the ratio kernel / oracle, largest value 3.2)
TERM = 2e-13  # tests/test_gpu_hot_faddeeva.py TOL: what the hot Voigt routine's region IV is held to, point by point
FAR_VS_DIRECT = 2e-13  # tests/test_gpu_far_field.py FAR_VS_DIRECT: the far role against the direct sum
NEAR = 1e-12  # a term this close (relative) to a Humlicek boundary may take the neighbouring rational (oracle.count_region_flips)
NEAR_BOUND = 1e-4  # ... a step of the approximation itself: tests/test_gpu_hot_faddeeva.py bounds such points at 1e-4
NEAR_SHARE = 1e-3  # at most this share of a class's terms may be excluded that way
VISIBLE = 1e-9  # every term of a probe line is at least this share of the truth at its grid point (or exactly zero)
MIXED_LINE, MIXED_FLUX = 5e-5, 1e-4  # tests/test_gpu_far_field.py: the mixed mode's stated bounds on the line plane and the flux

# the constants of the line path (stardis_amd/csrc/sdx_kernels.h), restated: the CPU test recomputes every class's decision from them
NARROW_HALF_WIDTH, NARROW_REACH, MEDIUM_HALF_WIDTH, TILE, FAR_UNIT_TILES = 64, 128, 4096, 256, 8
FAR_RATIO = 6.0  # sdx_far_field_rule: near_points = FAR_RATIO * TILE / 2 + TILE / 2

D = 2.0 ** 30  # grid spacing [Hz]
K0 = 600000  # nus[0] = K0 * D


# ---- the reference's formulas in extended precision -----------------------------------------------------------------------------
def regions(x, y):
    """voigt.py:31-44 in fp64 -> region number 1..4 per point"""
    ax = np.abs(x)
    s = ax + y
    r = np.full(x.shape, 4, dtype=np.int8)
    r[y >= 0.195 * ax - 0.176] = 3
    r[s > 5.5] = 2
    r[s > 15.0] = 1
    return r


def near_boundary(x, y, rel=NEAR):
    """oracle.count_region_flips' own predicate: within `rel` (relative) of s = 15, s = 5.5 or y = 0.195 |x| - 0.176"""
    ax = np.abs(x)
    s, edge = ax + y, 0.195 * ax - 0.176
    third = (s <= 5.5) & (np.abs(y - edge) <= rel * (np.abs(y) + np.abs(edge)))
    return (np.abs(s - 15.0) <= rel * 15.0) | (np.abs(s - 5.5) <= rel * 5.5) | third


def near_boundary_f32(x, y, margin=1e-4):
    """the same for the fp32 routine of the mixed mode, whose x and y carry fp32 roundings: the margin — absolute — that
    tests/test_gpu_hot_faddeeva.py keeps from the boundaries when it pins that routine (an fp32 ulp of |x| + y = 15 is 1e-6)"""
    ax = np.abs(x)
    s, edge = ax + y, 0.195 * ax - 0.176
    return (np.abs(s - 15.0) <= margin) | (np.abs(s - 5.5) <= margin) | ((s <= 5.5 + margin) & (np.abs(y - edge) <= margin))


def faddeeva_re(x, y):
    """Re w(x + i y): region from the fp64 x, y; the region's rational (voigt.py:47, :50-56, :59-67, :70-84) in longdouble"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    reg = regions(x, y)
    out = np.zeros(x.shape, dtype=L)
    with np.errstate(all="ignore"):
        for k in (1, 2, 3, 4):
            m = reg == k
            if not m.any():
                continue
            xl, yl = x[m].astype(L), y[m].astype(L)
            z = xl.astype(CL) + CL(1j) * yl
            if k == 1:
                w = CL(1j) / L(SQRT_PI) * z / (z * z - L(0.5))
            elif k == 2:
                z2 = z * z
                w = CL(1j) * (z * (z2 / L(SQRT_PI) - L(1.4104739589))) / (L(0.75) + z2 * (z2 - L(3.0)))
            else:
                t = yl.astype(CL) - CL(1j) * xl
                if k == 3:
                    p = L(16.4955) + t * (L(20.20933) + t * (L(11.96482) + t * (L(3.778987) + t * L(0.5642236))))
                    q = L(16.4955) + t * (L(38.82363) + t * (L(39.27121) + t * (L(21.69274) + t * (L(6.699398) + t))))
                    w = p / q
                else:
                    u = t * t
                    p = L(36183.31) - u * (L(3321.99) - u * (L(1540.787) - u * (L(219.031) - u * (L(35.7668) - u * (L(1.320522) - u * L(0.56419))))))
                    q = L(32066.6) - u * (L(24322.8) - u * (L(9022.23) - u * (L(2186.18) - u * (L(364.219) - u * (L(61.5704) - u * (L(1.84144) - u))))))
                    w = np.exp(u) - t * p / q
            out[m] = w.real
    return out


def windows(n_depth, nus, line_nus, dws, gammas, alphas):
    """oracle.window for every (line, depth) -> (lo, hi), int64 (N_l, N_d).  (The library's orc_window with d_nu formed once.)"""
    import oracle

    lib = oracle.lib()
    nus = np.ascontiguousarray(nus, dtype=np.float64)
    ln, dw, g, a = _tables(n_depth, line_nus, dws, gammas, alphas)
    pn = nus.ctypes.data_as(C.POINTER(C.c_double))
    d_nu = C.c_double(lib.orc_d_nu(C.c_int64(nus.size), pn))
    lo, hi = np.empty(dw.shape, dtype=np.int64), np.empty(dw.shape, dtype=np.int64)
    a_, b_ = C.c_int64(), C.c_int64()
    n = C.c_int64(nus.size)
    same = np.all(dw == dw[:, :1], axis=1) & np.all(g == g[:, :1], axis=1) & np.all(a == a[:, :1], axis=1)  # one call serves every depth
    for l in range(ln.size):
        for d in range(1 if same[l] else n_depth):
            lib.orc_window(n, pn, d_nu, C.c_double(ln[l]), C.c_double(g[l, d if g.shape[1] > 1 else 0]), C.c_double(dw[l, d]), C.c_double(a[l, d]),
                           C.byref(a_), C.byref(b_))
            lo[l, d], hi[l, d] = a_.value, b_.value
        if same[l]:
            lo[l, 1:], hi[l, 1:] = lo[l, 0], hi[l, 0]
    return lo, hi


def _tables(n_depth, line_nus, dws, gammas, alphas):
    ln = np.ascontiguousarray(line_nus, dtype=np.float64).reshape(-1)
    dw = np.ascontiguousarray(dws, dtype=np.float64).reshape(ln.size, n_depth)
    g = np.ascontiguousarray(gammas, dtype=np.float64).reshape(ln.size, -1)
    a = np.ascontiguousarray(alphas, dtype=np.float64).reshape(ln.size, n_depth)
    return ln, dw, g, a


class Truth:
    """plane (N_d, N_nu) longdouble; near (N_d, N_nu): a term within NEAR of a region boundary lands there (near32: within an fp32
    margin, near_boundary_f32); n_terms, n_near, n_near32;
    filler (N_d, N_nu): the sum without the probe lines' terms; lo, hi (N_l, N_d); probe_index (n_probe,), probe_terms
    (n_probe, N_d, N_nu) longdouble, zeros outside the windows"""


def _sum_terms(nus, ln, dw, g, a, lo, hi, plane, filler, near, near32, probe_terms, slot, chunk):
    """add the terms of every (line, depth) item of the tables (depth axis: dw.shape[1]) -> (terms, terms near a region boundary, the
    same at fp32 precision)"""
    n_nu, n_depth = nus.size, dw.shape[1]
    n_terms = n_near = n_near32 = 0
    size = np.maximum(hi - lo, 0).reshape(-1)  # item k = l * n_depth + d
    edges = np.searchsorted(np.cumsum(size), np.arange(chunk, int(size.sum()) + chunk, chunk), side="right")
    flat_plane, flat_near, flat_near32 = plane.reshape(-1), near.reshape(-1), near32.reshape(-1)
    flat_probe = probe_terms.reshape(-1) if probe_terms is not None else None
    flat_filler = filler.reshape(-1)
    start = 0
    for stop in edges:
        stop = max(int(stop), start + 1) if start < size.size else start
        stop = min(stop, size.size)
        items = np.arange(start, stop)
        cnt = size[start:stop]
        start = stop
        total = int(cnt.sum())
        if total == 0:
            continue
        item = np.repeat(items, cnt)
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        l, d = item // n_depth, item % n_depth
        i = lo.reshape(-1)[item] + (np.arange(total) - first)
        gd = g[l, d] if g.shape[1] > 1 else g[l, 0]
        dwd, ad = dw[l, d], a[l, d]
        with np.errstate(all="ignore"):
            x = (nus[i] - ln[l]) / dwd  # voigt.py:148: (delta_nu + 1j gamma') / doppler_width
            y = (gd / (SQRT_PI * PI)) / dwd
            term = faddeeva_re(x, y) / (L(SQRT_PI) * dwd.astype(L)) * ad.astype(L)  # voigt.py:150, base.py:627
        np.add.at(flat_plane, d * n_nu + i, term)
        nb = near_boundary(x, y)
        flat_near[(d * n_nu + i)[nb]] = True
        n_terms += total
        n_near += int(nb.sum())
        nb = near_boundary_f32(x, y)
        flat_near32[(d * n_nu + i)[nb]] = True
        n_near32 += int(nb.sum())
        if flat_probe is not None:
            p = slot[l] >= 0
            if p.any():
                np.add.at(flat_probe, (slot[l][p] * n_depth + d[p]) * n_nu + i[p], term[p])
            np.add.at(flat_filler, (d * n_nu + i)[~p], term[~p])
        else:
            np.add.at(flat_filler, d * n_nu + i, term)
    assert start == size.size
    return n_terms, n_near, n_near32


def truth(n_depth, nus, line_nus, dws, gammas, alphas, probes=None, chunk=1 << 20):
    """-> Truth.  Lines (other than probe lines) whose three values are the same bits at every depth are evaluated at one depth and
    added to all: the same terms, once."""
    nus = np.ascontiguousarray(nus, dtype=np.float64)
    ln, dw, g, a = _tables(n_depth, line_nus, dws, gammas, alphas)
    n_nu, n_lines = nus.size, ln.size
    lo, hi = windows(n_depth, nus, ln, dw, g, a)
    t = Truth()
    t.lo, t.hi = lo, hi
    t.plane = np.zeros((n_depth, n_nu), dtype=L)
    t.filler = np.zeros((n_depth, n_nu), dtype=L)  # the same sum without the probe lines
    t.near = np.zeros((n_depth, n_nu), dtype=bool)
    t.near32 = np.zeros((n_depth, n_nu), dtype=bool)
    t.probe_index = np.flatnonzero(probes) if probes is not None else np.zeros(0, dtype=np.int64)
    slot = np.full(n_lines, -1, dtype=np.int64)
    slot[t.probe_index] = np.arange(t.probe_index.size)
    t.probe_terms = np.zeros((t.probe_index.size, n_depth, n_nu), dtype=L)
    same = np.zeros(n_lines, dtype=bool)
    if n_depth > 8 and n_lines:
        same = np.all(dw == dw[:, :1], axis=1) & np.all(g == g[:, :1], axis=1) & np.all(a == a[:, :1], axis=1) & (slot < 0)
    k = ~same
    t.n_terms, t.n_near, t.n_near32 = _sum_terms(nus, ln[k], dw[k], g[k], a[k], lo[k], hi[k], t.plane, t.filler, t.near, t.near32, t.probe_terms,
                                                 slot[k], chunk)
    if same.any():
        k = same
        one, fill1 = np.zeros((1, n_nu), dtype=L), np.zeros((1, n_nu), dtype=L)
        near1, near2 = np.zeros((1, n_nu), dtype=bool), np.zeros((1, n_nu), dtype=bool)
        nt, nn, nn32 = _sum_terms(nus, ln[k], dw[k][:, :1], g[k][:, :1], a[k][:, :1], lo[k][:, :1], hi[k][:, :1], one, fill1, near1, near2, None, None,
                                  chunk)
        t.plane += one
        t.filler += fill1
        t.near |= near1
        t.near32 |= near2
        t.n_terms += nt * n_depth
        t.n_near += nn * n_depth
        t.n_near32 += nn32 * n_depth
    for arr in (t.plane, t.filler, t.near, t.near32, t.probe_terms, t.lo, t.hi):
        arr.setflags(write=False)
    return t


def distance(a, ref, where=None):
    """the largest pointwise |a - ref| / ref over the points where ref != 0 (and `where` holds); 0.0 when there is none"""
    a, ref = np.asarray(a).astype(L), np.asarray(ref).astype(L)
    m = ref != 0
    if where is not None:
        m = m & where
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        return float((np.abs(a[m] - ref[m]) / np.abs(ref[m])).max())


def bound(oracle_distance, far_field=False):
    """what a kernel's pointwise distance from the truth, relative to the truth, may be"""
    return FACTOR * float(oracle_distance) + TERM + (FAR_VS_DIRECT if far_field else 0.0)


def judge(c, got, far_field, label="", record=None):
    """the asserts of a fp64 line plane `got` of Case c against the truth -> (distance, allowed): the zero pattern; the pointwise distance
    within bound() outside the near-boundary points, within NEAR_BOUND on them; and what the probe lines add — the plane minus the
    filler's truth against their own terms, on the scale of the whole sum."""
    r = c.reference()
    t = r["t"]
    got = np.asarray(got)
    assert got.shape == t.plane.shape and np.all(np.isfinite(got)), label
    assert np.array_equal(got == 0, t.plane == 0), label
    allowed = bound(r["oracle_distance"], far_field=far_field)
    dist = distance(got, t.plane, r["tight"])
    loose = distance(got, t.plane, ~r["tight"])
    if record is not None:
        record.append(dict(route=label, case=c.name, n_depth=c.n_depth, n_nu=c.n_nu, n_lines=c.n_lines, kernel=dist,
                           oracle=r["oracle_distance"], excluded_share=t.n_near / max(t.n_terms, 1)))
    print(f"{c.name:24s} {label:34s} kernel {dist:.3e} oracle {r['oracle_distance']:.3e} bound {allowed:.3e} near-boundary {loose:.3e}")
    assert dist <= allowed, (label, dist, allowed)
    assert loose <= NEAR_BOUND, (label, loose)
    probe = t.probe_terms.sum(axis=0)
    with np.errstate(all="ignore"):
        rest = np.abs((got.astype(L) - r["filler"]) - probe)
    m = (t.plane != 0) & r["tight"]
    assert np.all(rest[m] <= allowed * t.plane[m]), label
    return dist, allowed


# ---- dialling a window ----------------------------------------------------------------------------------------------------------
def d_nu_of(nus):
    return float(-np.diff(np.asarray(nus, dtype=np.float64)).max())  # base.py:524-526


def pixels_of(gamma, dw, alpha, d_nu):
    return ((gamma + dw) * alpha) / d_nu * 20  # base.py:560-563, in this order


def half_width_of(gamma, dw, alpha, d_nu, n_nu):
    p = pixels_of(gamma, dw, alpha, d_nu)
    forced = p if p > 10 else 10.0
    return int(n_nu) if forced >= float(n_nu) else int(forced)


def solve_alpha(gamma, dw, d_nu, pixels, accept):
    """an alpha whose fp64 pixels_of satisfies accept(p): start from the real-number solution, walk by ulps"""
    a = pixels * d_nu / 20.0 / (gamma + dw)
    for _ in range(200):
        p = pixels_of(gamma, dw, a, d_nu)
        if accept(p):
            return float(a)
        a = np.nextafter(a, np.inf if p < pixels else 0.0)
    raise ValueError(f"no alpha gives {pixels} pixels with gamma {gamma}, doppler width {dw}")


def alpha_for_half_width(hw, gamma, dw, d_nu, n_nu):
    """alpha that makes the reference's half-width exactly hw (hw >= 11; hw == n_nu: saturated), the pixel count half way to hw + 1"""
    if hw >= n_nu:
        return solve_alpha(gamma, dw, d_nu, float(hw) + 0.5, lambda p: p >= float(n_nu))
    return solve_alpha(gamma, dw, d_nu, hw + 0.5, lambda p: hw < p < hw + 1)


# ---- the lists ------------------------------------------------------------------------------------------------------------------
def grid(n_nu, jump=None):
    """descending, exact: spacing D; jump = (index, factor): spacing factor * D in front of that index"""
    step = np.ones(n_nu - 1)
    if jump is not None:
        step[:jump[0]] = jump[1]
    return (K0 * float(jump[1] if jump else 1) - np.concatenate([[0.0], np.cumsum(step)])) * D


def centre_index(nus, line_nu):
    return nus.size - np.searchsorted(nus[::-1], line_nu, side="left")  # base.py:556-558


DEPTH_DW = (1.0, 1.3, 0.8)  # Doppler width per depth relative to the first


class Case:
    """one list of a class.  hw[l, d]: the half-width claimed for probe item (l, d), -1 where nothing is claimed; centre[l] likewise."""

    def __init__(self, cls, name, nus, n_depth, gamma_cols=None):
        self.cls, self.name, self.nus, self.n_depth = cls, name, nus, n_depth
        self.d_nu, self.n_nu = d_nu_of(nus), nus.size
        self.rows = []  # (line_nu, dw[n_depth], gamma[n_depth], alpha[n_depth], probe, hw[n_depth], centre)
        self.gamma_cols = gamma_cols
        self.notes = {}
        self._ref = None

    def dws(self, scale):
        f = np.array([DEPTH_DW[d % 3] * (1.0 + 0.01 * (d // 3)) for d in range(self.n_depth)])
        return scale * D * f

    def add(self, line_nu, hw, probe=True, dw=3.1, y=None, pixels=None, accept=None, centre=-1, alpha=None, gamma=None):
        """one line.  hw: int or per-depth sequence (10: the floor, with 5 pixels unless `pixels`/`accept` say otherwise).
        y: the Voigt parameter at the first depth (default: 1 for windows up to 30 points, hw / 30 beyond — a profile flat enough
        that the window's edge terms stay visible)."""
        nd = self.n_depth
        hws = np.full(nd, hw, dtype=np.int64) if np.isscalar(hw) else np.asarray(hw, dtype=np.int64)
        dwv = self.dws(dw) if np.isscalar(dw) else np.asarray(dw, dtype=np.float64)
        if gamma is None:
            yy = y if y is not None else max(1.0, min(int(hws.max()), self.n_nu) / 30.0)
            gv = np.full(nd, yy * dwv[0] * (SQRT_PI * PI))
        else:
            gv = np.full(nd, gamma, dtype=np.float64) if np.isscalar(gamma) else np.asarray(gamma, dtype=np.float64)
        av = np.empty(nd)
        for d in range(nd):
            if alpha is not None:
                av[d] = alpha if np.isscalar(alpha) else alpha[d]
            elif hws[d] == 10:
                px = 5.0 if pixels is None else pixels
                av[d] = solve_alpha(gv[d], dwv[d], self.d_nu, px, accept or (lambda p, px=px: abs(p - px) < 1e-6))
            else:
                av[d] = alpha_for_half_width(int(hws[d]), gv[d], dwv[d], self.d_nu, self.n_nu)
        self.rows.append((float(line_nu), dwv, gv, av, bool(probe), hws if probe else np.full(nd, -1), int(centre)))

    def filler(self, n, rng, lo=None, hi=None, strength=1.0):
        """n floor-window lines between grid points, y from 0.01 to 1, Doppler widths from half a point to three: every region"""
        lo = self.nus[-1] if lo is None else lo
        hi = self.nus[0] if hi is None else hi
        for nu in np.sort(rng.uniform(lo, hi, n)):
            dw = float(rng.uniform(0.5, 3.0))
            self.add(nu, 10, probe=False, dw=dw, y=float(10.0 ** rng.uniform(-2.0, 0.0)), pixels=5.0 * strength)

    def build(self):
        order = np.argsort([r[0] for r in self.rows], kind="stable")
        rows = [self.rows[k] for k in order]
        self.line_nus = np.array([r[0] for r in rows])
        self.dw = np.ascontiguousarray(np.stack([r[1] for r in rows]))
        g = np.stack([r[2] for r in rows])
        self.gammas = np.ascontiguousarray(g[:, :1] if self.gamma_cols == 1 else g)
        if self.gamma_cols == 1:
            assert np.all(g == g[:, :1])
        self.alphas = np.ascontiguousarray(np.stack([r[3] for r in rows]))
        self.probe = np.array([r[4] for r in rows])
        self.hw = np.stack([r[5] for r in rows])
        self.centre = np.array([r[6] for r in rows])
        self.n_lines = self.line_nus.size
        del self.rows
        return self

    # -- the inputs, whole or without the probe lines
    def args(self, keep=None):
        k = slice(None) if keep is None else keep
        return (self.n_depth, self.nus, self.line_nus[k], self.dw[k], self.gammas[k], self.alphas[k])

    def lines(self, keep=None):
        _, _, ln, dw, g, a = self.args(keep)
        return dict(line_nus=ln, doppler_widths=dw, gammas=g, alphas=a)

    def reference(self):
        """-> dict(t: Truth of the whole list, filler: the plane of the list without its probe lines, oracle, evals, oracle_distance,
        tight: the points held to bound()): computed once, left unchanged"""
        if self._ref is None:
            import oracle

            t = truth(*self.args(), probes=self.probe)
            with np.errstate(all="ignore"):
                o, evals = oracle.calc_alan_entries(*self.args(), return_evals=True)
            o.setflags(write=False)
            tight = ~t.near
            self._ref = dict(t=t, filler=t.filler, oracle=o, evals=int(evals), tight=tight, oracle_distance=distance(o, t.plane, tight))
        return self._ref


def _probe_windows(c, nu, tag_centre=-1, hws=(10, 300, 4500, None), **kw):
    for hw in hws:
        c.add(nu, c.n_nu if hw is None else hw, centre=tag_centre, **kw)


def _grid_ends(long=False):
    """long: the same on 16389 points (fewer positions) — above 16384 a frequency shard of an indexed list runs the culled pre-pass
    (classification, sel, xlist), and the list then holds lines of every class beyond either end, plus 4096 / 4097 in the middle"""
    c = Case("grid_ends", "grid_ends_long" if long else "grid_ends", grid(16389 if long else 8197), 3)
    rng = np.random.default_rng(11 + long)
    n, nus = c.n_nu, c.nus
    # (searchsorted-left on the ascending grid: a line ON grid frequency i has centre i + 1, like the line an ulp below it)
    on_ends = ((nus[0], 1), (np.nextafter(nus[0], np.inf), 0), (np.nextafter(nus[0], 0.0), 1),
               (nus[-1], n), (np.nextafter(nus[-1], np.inf), n - 1), (np.nextafter(nus[-1], 0.0), n))
    for nu, centre in (on_ends[::3] if long else on_ends):
        _probe_windows(c, nu, centre)
    for k in ((0.5, 10.5, 200.0, 5000.0) if long else (0.5, 9.5, 10.5, 63.0, 200.0, 5000.0)):
        _probe_windows(c, nus[0] + k * D, 0)
        _probe_windows(c, nus[-1] - k * D, n)
    if long:
        for hw in (MEDIUM_HALF_WIDTH, MEDIUM_HALF_WIDTH + 1):
            c.add(line_with_centre(nus, 8200), hw, centre=8200)
    c.filler(600, rng)
    return c.build()


def _on_points():
    c = Case("on_points", "on_points", grid(2051), 3)
    rng = np.random.default_rng(12)
    for i in (255, 256, 257, 2047, 2048, c.n_nu - 1):
        v = c.nus[i]
        for nu, centre in ((v, i + 1), (np.nextafter(v, np.inf), i), (np.nextafter(v, 0.0), i + 1)):
            _probe_windows(c, nu, centre, hws=(10, 300))
    c.filler(500, rng)
    return c.build()


def _class_edges():
    c = Case("class_edges", "class_edges", grid(8197), 3)
    rng = np.random.default_rng(13)
    n = c.n_nu
    mid = c.nus[4098] + 0.37 * D  # centre 4098: a half-width of 4097 stays inside the grid on both sides
    assert centre_index(c.nus, mid) == 4098
    c.add(c.nus[700] + 0.2 * D, 10, pixels=float(np.nextafter(10.0, 0.0)), accept=lambda p: 9.999999 < p < 10.0)
    # (g + dw) a power of two makes pixels exactly 10.0: the reference's max(10, pixels) keeps the 10 on the tie
    dw_exact = np.array([2.0, 4.0, 8.0]) * D
    c.add(c.nus[900] + 0.2 * D, 10, dw=dw_exact, gamma=dw_exact * 3.0, pixels=10.0, accept=lambda p: p == 10.0)
    c.add(c.nus[1100] + 0.2 * D, 10, pixels=float(np.nextafter(10.0, np.inf)), accept=lambda p: 10.0 < p < 10.000001)
    for k, hw in enumerate((11, 64, 65, 128, 129)):
        c.add(c.nus[1280 + 256 * k] + 0.4 * D, hw)  # centres on tile edges
        c.add(c.nus[5000 + 300 * k] - 0.4 * D, hw)
    for hw in (4096, 4097, n - 1, n):
        c.add(mid, hw)
    c.add(mid + 3 * D, n, y=n / 30.0, alpha=float(2.0 ** 31 * 1.5 * c.d_nu / 20.0 / (n / 30.0 * 3.1 * D * SQRT_PI * PI + 3.1 * D)))
    c.add(c.nus[3000] + 0.3 * D, 10, alpha=0.0)  # a floor window of exact zeros
    c.filler(800, rng)
    return c.build()


def _depth_varying(n_depth):
    c = Case("depth_varying", f"depth_varying_{n_depth}", grid(2051), n_depth, gamma_cols=1)
    rng = np.random.default_rng(14 + n_depth)
    d = np.arange(n_depth)
    chunks = d // 64
    up = np.choose(np.minimum(chunks, 2), [40, 300, c.n_nu])  # narrow, then medium, then the whole grid
    down = np.choose(np.minimum(chunks, 2), [c.n_nu, 300, 40])
    mixed = np.where(d % 3 == 0, 20, np.where(d % 3 == 1, 700, c.n_nu))
    once = np.where(d == min(70, n_depth - 2), 200, 10)  # wide at exactly one depth
    for k, hws in enumerate((up, down, mixed, once)):
        c.add(c.nus[300 + 400 * k] + 0.3 * D, hws, y=2.0)
    c.filler(300, rng)
    return c.build()


COINCIDENT_K = (2, 63, 64, 65, 255, 256, 257, 1025)
COINCIDENT_START = (256, 192, 37, 512, 320, 101, 768, 64)  # multiples of 256, of 64 only, of neither


def _coincident(K, start, wide):
    c = Case("coincident", f"coincident_{K}_{'wide' if wide else 'narrow'}", grid(2051), 3)
    rng = np.random.default_rng(15 + K + wide)
    nu = c.nus[1111] + 0.25 * D
    below = np.sort(rng.uniform(c.nus[-1], nu - 50 * D, start))
    for v in below:
        c.add(v, 10, probe=False, dw=float(rng.uniform(0.5, 3.0)), y=float(10.0 ** rng.uniform(-2.0, 0.0)))
    for _ in range(K):
        c.add(nu, 200 if wide else 10)
    c.filler(1400 - start, rng, lo=nu + 50 * D)
    c.notes["start"], c.notes["K"] = start, K
    return c.build()


def _pile_up(wide):
    c = Case("pile_up", "pile_up_wide" if wide else "pile_up_narrow", grid(2051), 3)
    rng = np.random.default_rng(16 + wide)
    for side in (0, 1):
        off = rng.uniform(0.1, 50.0, 3000)
        for k, o in enumerate(off):
            nu = c.nus[0] + o * D if side == 0 else c.nus[-1] - o * D
            hw = 10
            if wide and k % 500 == 7:
                hw = (300, c.n_nu, 65)[(k // 500) % 3]
            c.add(nu, hw, probe=(k % 100 == 7), dw=float(rng.uniform(1.0, 3.0)), centre=0 if side == 0 else c.n_nu)
    c.filler(50, rng)
    return c.build()


def _profiles():
    c = Case("profiles", "profiles", grid(2051), 3)
    slot = iter(range(40, 2000, 45))  # 45 points apart: floor windows never meet

    def at():
        return c.nus[next(slot)] + 0.3 * D

    big = SQRT_PI * PI
    c.add(at(), 10, gamma=0.0)
    c.add(at(), 10, gamma=1e-30 * 3.1 * D * big)  # y = 1e-30
    c.add(at(), 10, gamma=1e-310)  # a subnormal gamma
    c.add(at(), 10, y=15.0)
    c.add(at(), 10, y=1e6, alpha=1e-9)
    c.add(at(), 10, dw=1e-7, gamma=0.0, alpha=1.0)  # ten points reach |x| = 1e8
    c.add(at(), 10, dw=1e-7, y=1e3, alpha=1.0)
    c.add(at(), 10, dw=2e7, gamma=0.0, alpha=1e-12)  # |x| < 1e-6 over the whole window
    c.add(at(), 10, dw=2e7, y=1e-3, alpha=1e-12)
    c.add(at(), 10, alpha=1e-285)
    c.add(at(), 10, gamma=0.0, dw=1.0, alpha=1e-285)
    return c.build()


def _profiles_big():
    """the upper end of the range: a strength of 1e290 saturates the window rule — one line over the whole grid, terms up to 1e280"""
    c = Case("profiles", "profiles_big", grid(2051), 3)
    c.add(c.nus[1000] + 0.3 * D, c.n_nu, y=1.0, alpha=1e290)
    return c.build()


def far_ranges(nus):
    """far_range[2 T], [2 T + 1] per full tile T, as far_ranges_block (sdx_kernels.h) defines them: the number of grid frequencies
    >= c + 6 h and >= c - 6 h, c and h the centre and half-width of the tile from its end frequencies.  A line is far from tile T
    when its centre index is < the first or > the second."""
    out = []
    for T in range(nus.size // TILE):
        a, b = nus[T * TILE], nus[T * TILE + TILE - 1]
        cc, h = 0.5 * (a + b), 0.5 * (a - b)
        out.append((int(np.count_nonzero(nus >= cc + FAR_RATIO * h)), int(np.count_nonzero(nus >= cc - FAR_RATIO * h))))
    return np.array(out)


def line_with_centre(nus, idx, frac=0.3):
    """a frequency between grid points whose centre index (base.py:556-558) is idx (0 < idx < N_nu)"""
    nu = nus[idx] + frac * (nus[idx - 1] - nus[idx])
    assert centre_index(nus, nu) == idx
    return nu


def _far_edges(jump):
    nus = grid(2051, jump=(400, 10.0) if jump else None)
    c = Case("far_edges", "far_edges_jump" if jump else "far_edges", nus, 3)
    rng = np.random.default_rng(17 + jump)
    fr = far_ranges(nus)
    c.notes["far_ranges"] = fr
    seen = set()
    for T in ((3, 5) if not jump else (3, 4)):
        for r in fr[T]:
            for idx in (r - 1, r, r + 1):
                if 0 < idx < c.n_nu and idx not in seen:
                    seen.add(idx)
                    c.add(line_with_centre(nus, idx), 1500, centre=idx)
    c.notes["bound_centres"] = sorted(seen)
    # windows that end on a tile's first or last point, one beside it, and in the middle of a tile
    for k, (centre, hw) in enumerate(((1100, 1100 - 256), (1100, 1100 - 257), (1100, 1100 - 255), (1100, 1100 - 384),
                                      (900, 1792 - 900), (900, 1793 - 900), (900, 1791 - 900), (900, 1664 - 900))):
        c.add(line_with_centre(nus, centre, 0.2 + 0.05 * k), hw, centre=centre)
    # cores (the points within NARROW_REACH of the centre) that end on a tile boundary
    for centre in (1024 - NARROW_REACH, 1024 + NARROW_REACH, 1024, 1280 - NARROW_HALF_WIDTH):
        c.add(line_with_centre(nus, centre, 0.6), 1300, centre=centre)
    c.filler(400, rng)
    return c.build()


def _sparse(kind):
    c = Case("sparse", f"sparse_{kind}", grid(2051), 3)
    rng = np.random.default_rng(18)
    if isinstance(kind, int):
        pos = np.sort(rng.uniform(c.nus[-1], c.nus[0], kind))
        for k, nu in enumerate(pos):
            c.add(nu, 300 if k == kind // 2 else 10, dw=float(rng.uniform(1.0, 3.0)))
    elif kind == "one_tile":
        for k, nu in enumerate(np.sort(rng.uniform(c.nus[5 * TILE - 1], c.nus[4 * TILE], 200))):
            c.add(nu, 90 if k % 50 == 0 else 10, dw=float(rng.uniform(1.0, 3.0)))
    else:  # every second tile holds no line, and no window reaches into it from the floor lines
        for T in range(0, 8, 2):
            for nu in np.sort(rng.uniform(c.nus[T * TILE + TILE - 12], c.nus[T * TILE + 11], 60)):
                c.add(nu, 10, dw=float(rng.uniform(1.0, 3.0)))
    return c.build()


def _walk(kind):
    """the narrow walk's other forms at the smallest shapes the rule of line_partials (stardis_hip.hip) admits: F = 2 frequencies per
    wave from 16384 points with a line per two points, F = 4 from 32768, the subsets form from four lines per point on an indexed list"""
    n_nu, n_lines = dict(f2=(16384, 8192), f4=(32768, 16384), sub=(2048, 8192))[kind]
    # (the subsets form also wants four line subsets: choose_splits gives four from 640 (tile, depth) pairs on, 80 depths on 8 tiles —
    # with fewer it gives eight and the rule declines.  Its filler is the same at every depth, so that the truth stays cheap.)
    c = Case("walk", f"walk_{kind}", grid(n_nu), 80 if kind == "sub" else 3)
    rng = np.random.default_rng(19 + n_nu)
    # probes at line indices on and beside the 64- and 256-line stretches, each on a class bound; then K coincident lines
    where = [(255, 10), (256, 64), (257, 65), (1023, 128), (1024, 129), (4095, 11), (4096, 10), (4160, 64)]
    run_at, K = 6000, 70
    n_fill = n_lines - len(where) - K
    fill = np.sort(rng.uniform(c.nus[-1], c.nus[0], n_fill))
    taken = 0
    for j, hw in where:
        f = j - taken
        c.add(0.5 * (fill[f - 1] + fill[f]), hw)
        taken += 1
    f = run_at - taken
    for k in range(K):
        c.add(0.5 * (fill[f - 1] + fill[f]), 10, probe=(kind != "sub" or k % 10 == 0))
    for nu in fill:
        dw = float(rng.uniform(0.5, 3.0))
        c.add(nu, 10, probe=False, dw=dw if kind != "sub" else np.full(c.n_depth, dw * D), y=float(10.0 ** rng.uniform(-2.0, 0.0)))
    c.notes["where"], c.notes["run_at"], c.notes["K"] = where, run_at, K
    return c.build()


_BUILDERS = {}
for _n in ("grid_ends", "on_points", "class_edges", "profiles", "profiles_big"):
    _BUILDERS[_n] = globals()["_" + _n]
_BUILDERS["grid_ends_long"] = (lambda: _grid_ends(True))
for _nd in (65, 129):
    _BUILDERS[f"depth_varying_{_nd}"] = (lambda nd=_nd: _depth_varying(nd))
for _k, _s in zip(COINCIDENT_K, COINCIDENT_START):
    for _w in (0, 1):
        _BUILDERS[f"coincident_{_k}_{'wide' if _w else 'narrow'}"] = (lambda k=_k, s=_s, w=_w: _coincident(k, s, w))
for _w in (0, 1):
    _BUILDERS["pile_up_wide" if _w else "pile_up_narrow"] = (lambda w=_w: _pile_up(w))
for _j in (0, 1):
    _BUILDERS["far_edges_jump" if _j else "far_edges"] = (lambda j=_j: _far_edges(j))
for _kind in (1, 63, 64, 65, "one_tile", "alternate_tiles"):
    _BUILDERS[f"sparse_{_kind}"] = (lambda kind=_kind: _sparse(kind))
WALKS = ("walk_f2", "walk_f4", "walk_sub")
for _kind in ("f2", "f4", "sub"):
    _BUILDERS[f"walk_{_kind}"] = (lambda kind=_kind: _walk(kind))

NAMES = tuple(n for n in _BUILDERS if not n.startswith("walk_"))
CLASSES = ("grid_ends", "on_points", "class_edges", "depth_varying", "coincident", "pile_up", "profiles", "far_edges", "sparse")
# mixed_precision = 1: the header excludes what fp32 cannot hold — `profiles` (range ends, |x| = 1e8, subnormal gamma)
MIXED_NAMES = tuple(n for n in NAMES if not n.startswith("profiles"))

_cases = {}


def case(name):
    """the Case of a name, cached for the life of the process"""
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def hostile_lists(names=NAMES):
    for name in names:
        yield case(name)


# what the GPU tests measured in this process: dict(route, case, n_depth, n_nu, n_lines, kernel, oracle, excluded_share);
# scripts/line_truth_table.py runs the tests and writes these out
RECORD = []
