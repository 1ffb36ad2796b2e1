"""The formal solution on hostile columns, judged against an 80-bit evaluation of the reference's own formulas.

On rough columns the double-precision oracle is an inadequate judge of a kernel: for tau just above 5e-4 the reference forms
w1 = w0 - tau e^-tau and w2 = 2 w1 - tau^2 e^-tau (radiation_field_solvers/base.py:38-45), one ulp of exp amplified by 1 / tau^2 and
1 / tau^3, so ANY double-precision evaluation is ~1e-16 / tau^3 from an exact evaluation of the same formulas.  truth() is that
evaluation (numpy longdouble, 64-bit mantissa); a kernel is held to be no further from it than four times the oracle's own distance
(bound()).  hostile_columns() draws the columns: every regime of the weights, waves that sit in one regime or straddle a
threshold, transparent layers in every position, and optical depths at both ends of the double range, where the common denominator
t0 t1 (t0 + t1) of the kernels' step leaves the normal numbers.

Used by tests/test_formal_solution_truth_cpu.py (the reference alone meets the conditions the GPU tests rest on),
tests/test_gpu_formal_solution_truth.py (every kernel of the family), scripts/r4/rt_truth.py and scripts/fuzz_raytrace.py.
"""
import numpy as np

from stardis_amd import constants as K, synth

L = np.longdouble
EXTENDED = bool(np.finfo(L).eps <= 1e-18)  # a host without an extended long double has no truth to offer: the GPU tests skip
TAU_SMALL, TAU_BIG = 5e-4, 50.0  # the thresholds of the reference's two-regime weights (:22-45)
NEAR = 1e-9  # no tau of a hostile column lies this close (relative) to a threshold
FACTOR = 4.0  # scripts/fuzz_raytrace.py: over 200 seeds the ratio's median was 1.0, its largest value 3.2
PER_GAP = 4e-15  # sqrt(a) sqrt(a') against exp((log a + log a') / 2): ~|log alpha| ulp, once per gap (sdx_kernels.h)

CLASSES = ("thin", "straddle_small", "moderate", "straddle_50", "thick", "everything", "ramp", "leading_transparent",
           "interior_transparent", "surface_transparent", "transparent", "tiny", "underflow", "huge", "overflow", "spike")
# what the header documents for the fp32 formal solution (mixed_precision = 1): no NaN-producing geometry, no range ends
F32_CLASSES = ("thin", "straddle_small", "moderate", "straddle_50", "thick", "everything", "ramp", "leading_transparent", "transparent")


# ---- the reference's formulas in extended precision -----------------------------------------------------------------------------
def truth(nus, temps, dist, thetas, weights, alphas, ray_table=None, correction=None, source=None, contribution=False):
    """-> (F, I) in longdouble, with contribution=True (F, I, C).
    plane-parallel: dist; spherical: ray_table = calculate_spherical_ray(...) (inward sweep first, :141-198, gap 0 wrapping to the
    last gap / depth as the reference's negative index does) and the photospheric correction (:340-344).
    source: optional (N_d, N_nu) source-function plane (default: the Planck function, blackbody.py:31-35).
    C (plane-parallel only): the flux contribution function, C[0] = 0, C[k] = sum_theta w_theta T[k] e[k-1] from the step's affine
    map I[g+1] = c[g] I[g] + e[g], (c, e) = (1, 0) where t0 == 0, T[N_d-1] = 1, T[k] = T[k+1] c[k] (sdx_contribution_dev)."""
    nus, temps, alphas = np.asarray(nus).astype(L), np.asarray(temps).astype(L), np.asarray(alphas).astype(L)
    nd, nn, nt = temps.size, nus.size, np.asarray(thetas).size
    # the table is formed in double by the caller (:302-305 / :349-381)
    rd = (np.asarray(dist).reshape(-1, 1) / np.cos(thetas)).astype(L) if ray_table is None else np.asarray(ray_table, dtype=np.float64).astype(L)
    with np.errstate(all="ignore"):
        mean = np.exp((np.log(alphas[1:]) + np.log(alphas[:-1])) * L(0.5))  # (N_g, N_nu)
        tau = mean[:, :, None] * rd[:, None, :]  # (N_g, N_nu, N_theta)
        if source is None:
            pre = (2 * L(K.H_CGS) * nus ** 3) / (L(K.C_CGS) ** 2)
            S = pre[None, :] / (np.exp((L(K.H_CGS) * nus)[None, :] / (L(K.K_B_CGS) * temps[:, None])) - 1)
        else:
            S = np.asarray(source).astype(L).reshape(nd, nn)
        ex = np.exp(-tau)
        small, mid = tau < TAU_SMALL, tau < TAU_BIG
        w0 = np.where(small, tau * (1 - tau / 2), np.where(mid, 1 - ex, L(1)))
        w1 = np.where(small, tau ** 2 * (L(0.5) - tau / 3), np.where(mid, (1 - ex) - tau * ex, L(1)))
        w2 = np.where(small, tau ** 3 * (L(1) / 3 - tau / 4), np.where(mid, 2 * ((1 - ex) - tau * ex) - tau ** 2 * ex, L(2)))
        I = np.zeros((nd, nn, nt), dtype=L)
        if ray_table is not None:
            for g in range(nd - 2, -1, -1):
                gm, dm = (g - 1, g - 1) if g > 0 else (nd - 2, nd - 1)
                tg, tm = tau[g], tau[gm]
                sg, sm, sp = S[g][:, None], S[dm][:, None], S[g + 1][:, None]
                second = w1[g] * ((sg - sm) * (tg / tm) - (sg - sp) * (tm / tg)) / (tg + tm)
                third = w2[g] * (((sm - sg) / tm) + ((sp - sg) / tg)) / (tg + tm)
                new = (1 - w0[g]) * I[g + 1] + w0[g] * sg + second + third
                I[g] = np.where((tg == 0) | (tm == 0), I[g + 1], new)
            I[1:] = 0  # (only I[0] of the sweep survives: the outward pass overwrites the other rows)
        # the outward pass as the affine map I[g+1] = c[g] I[g] + e[g]
        c = np.where(tau == 0, L(1), 1 - w0)
        e = np.empty_like(tau)
        for g in range(nd - 2):
            t0, t1 = tau[g], tau[g + 1]
            s0, s1, s2 = S[g][:, None], S[g + 1][:, None], S[g + 2][:, None]
            second = w1[g] * ((s1 - s2) * (t0 / t1) - (s1 - s0) * (t1 / t0)) / (t0 + t1)
            third = w2[g] * (((s2 - s1) / t1) + ((s0 - s1) / t0)) / (t0 + t1)
            e[g] = w0[g] * s1 + second + third
        g = nd - 2
        e[g] = w0[g] * S[nd - 1][:, None] + w2[g] * (S[nd - 2][:, None] - S[nd - 1][:, None]) / tau[g] ** 2
        e = np.where(tau == 0, L(0), e)
        for g in range(nd - 1):
            I[g + 1] = np.where(tau[g] == 0, I[g], c[g] * I[g] + e[g])
        wts = np.asarray(weights).astype(L)
        F = (I * wts[None, None, :]).sum(axis=2)
        if correction is not None:
            F = F * L(correction)
        if not contribution:
            return F, I
        if ray_table is not None:
            raise ValueError("the contribution function is plane-parallel")
        T = np.ones((nd, nn, nt), dtype=L)
        for k in range(nd - 2, -1, -1):
            T[k] = T[k + 1] * c[k]
        C = np.zeros((nd, nn), dtype=L)
        C[1:] = ((T[1:] * e) * wts[None, None, :]).sum(axis=2)
    return F, I, C


def distance(a, ref, finite):
    """per column (every axis behind the first): max_d |a - ref| / max(max_d |ref|, 1e-300) over the positions where `finite` (where
    the oracle is finite) holds — the error against the scale of the ray / column, as scripts/fuzz_raytrace.py measures it."""
    a, ref = np.asarray(a).astype(L), np.asarray(ref).astype(L)
    with np.errstate(all="ignore"):
        diff = np.where(finite, np.abs(a - ref), L(0))
        scale = np.where(finite, np.abs(ref), L(0)).max(axis=0)
        return (diff.max(axis=0) / np.maximum(scale, L(1e-300))).astype(np.float64)


def bound(oracle_distance, n_depth):
    """what a kernel's distance from the truth may be, given the oracle's (the largest of a class)"""
    return FACTOR * float(oracle_distance) + PER_GAP * (n_depth - 1)


# ---- hostile columns ------------------------------------------------------------------------------------------------------------
def near_threshold(alphas, ray_table, rel=NEAR):
    """per column: does some gap's tau at some angle — the mean opacity formed as exp((log a + log a') / 2) as the reference and the
    oracle do, and as sqrt(a) sqrt(a') as the kernels do — lie within `rel` (relative) of 5e-4 or 50?  Across such a threshold the
    reference's own formulas jump; two evaluations on either side of it are not comparable."""
    a = np.asarray(alphas, dtype=np.float64)
    a = a.reshape(a.shape[0], -1)
    rd = np.asarray(ray_table, dtype=np.float64)
    bad = np.zeros(a.shape[1], dtype=bool)
    with np.errstate(all="ignore"):
        for mean in (np.exp((np.log(a[1:]) + np.log(a[:-1])) * 0.5), np.sqrt(a[1:]) * np.sqrt(a[:-1])):
            tau = mean[:, :, None] * rd[:, None, :]
            for thr in (TAU_SMALL, TAU_BIG):
                bad |= (np.abs(tau - thr) <= rel * thr).any(axis=(0, 2))
    return bad


def _draw(name, n_depth, rng):
    """t[d], the optical depth per point of one column of a class (alpha = t / 1e6, the gaps ~1e6 long)"""
    log_u = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, n_depth)  # noqa: E731
    if name == "thin":  # the series at every angle up to 20
        return log_u(-9.0, -3.9)
    if name == "straddle_small":
        return rng.uniform(2e-4, 1.2e-3, n_depth)
    if name == "moderate":
        return log_u(-3.0, 1.0)
    if name == "straddle_50":
        return rng.uniform(15.0, 80.0, n_depth)
    if name == "thick":
        return log_u(2.0, 6.0)
    if name == "everything":
        return log_u(-9.0, 6.0)
    if name == "ramp":
        return np.geomspace(1e3, 1e-7, n_depth) * rng.uniform(0.5, 2.0, n_depth)
    if name == "transparent":
        return np.zeros(n_depth)
    if name == "tiny":  # the denominator about 1e-290: still a normal number
        return log_u(-100.0, -90.0)
    if name == "underflow":  # the denominator and w2 subnormal or zero: the rare-lane path
        return log_u(-110.0, -104.0)
    if name == "huge":  # the denominator about 1e300: finite
        return log_u(95.0, 101.0)
    if name == "overflow":  # the denominator inf: the rare-lane path
        return log_u(104.0, 110.0)
    # spike: its ordinary points from the upper three decades of `moderate` — below tau ~ 1e-2 the oracle's own cancellation (4e-13 at
    # 55 depth points, one angle, with the full range) exceeds the 1e-13 the oracle is held to in this class
    t = log_u(-2.0 if name == "spike" else -3.0, 1.0)
    if name == "leading_transparent":  # rows 0 .. k
        t[:int(rng.integers(0, max(1, n_depth - 1))) + 1] = 0.0
    elif name == "interior_transparent":  # one interior row: the reference divides by zero two gaps before it (NaN from there on)
        t[int(rng.integers(1, n_depth - 1)) if n_depth > 2 else 0] = 0.0  # (two points have no interior: the first row)
    elif name == "surface_transparent":  # the last row: NaN from the last gap but one
        t[-1] = 0.0
    elif name == "spike":
        t[int(rng.integers(0, n_depth))] = 1e107
    else:
        raise ValueError(f"unknown class {name!r}")
    return t


def hostile_columns(n_depth, per_class, rng, order, ray_table, classes=CLASSES):
    """-> (alphas [n_depth, n_nu], class_of_column [n_nu]): per_class columns of every class, alpha = t / 1e6.
    order = "grouped": a class's columns next to each other (whole waves in one regime); "interleaved": the classes alternate.
    ray_table: the (n_depth-1, n_theta) table the columns will be traced on — a column with a tau within 1e-9 (relative) of a
    threshold of the weights is drawn again from the next values of the stream."""
    if order not in ("grouped", "interleaved"):
        raise ValueError(order)
    cols = {}
    for name in classes:
        drawn = []
        while len(drawn) < per_class:
            a = _draw(name, n_depth, rng) / 1e6
            if not near_threshold(a, ray_table)[0]:
                drawn.append(a)
        cols[name] = drawn
    if order == "grouped":
        seq = [(name, k) for name in classes for k in range(per_class)]
    else:
        seq = [(name, k) for k in range(per_class) for name in classes]
    alphas = np.ascontiguousarray(np.stack([cols[name][k] for name, k in seq], axis=1))
    cls = np.array([name for name, _ in seq])
    assert alphas.shape == (n_depth, per_class * len(classes)) and all(int((cls == name).sum()) == per_class for name in classes)
    assert not near_threshold(alphas, ray_table).any()
    return alphas, cls


class Case:
    """one shape's inputs, and (reference()) the truth and the oracle on them, computed once"""

    def __init__(self, n_depth, n_theta, per_class=16, order="grouped", classes=CLASSES, spherical=False, seed=None):
        self.n_depth, self.n_theta, self.order, self.classes, self.spherical = n_depth, n_theta, order, tuple(classes), spherical
        rng = np.random.default_rng(100 * n_depth + n_theta if seed is None else seed)
        self.temps = np.linspace(3900.0, 9500.0, n_depth)
        self.dist = rng.uniform(0.5e6, 2e6, n_depth - 1)
        self.thetas, self.weights = synth.thetas_and_weights(n_theta)
        self.r = self.reference_r = self.correction = None
        if spherical:
            import oracle

            self.r = 6e8 + np.concatenate([[0.0], np.cumsum(self.dist)])  # grazing rays miss the inner shells: zeros in the chord table
            self.reference_r = float(self.r[-3])
            self.ray = oracle.calculate_spherical_ray(self.thetas, self.r)
            self.correction = (self.r[-1] / self.reference_r) ** 2
        else:
            self.ray = self.dist.reshape(-1, 1) / np.cos(self.thetas)
        self.alphas, self.cls = hostile_columns(n_depth, per_class, rng, order, self.ray, classes)
        self.n_nu = self.alphas.shape[1]
        self.nus = np.linspace(7.5e14, 3.0e14, self.n_nu)  # strictly descending, as the fused step wants them
        self._ref = None

    def columns(self, name):
        return self.cls == name

    def truth(self, alphas=None, contribution=False):
        """the truth on these inputs, for the case's own columns or for another plane on the same grid"""
        return truth(self.nus, self.temps, self.dist, self.thetas, self.weights, self.alphas if alphas is None else alphas,
                     ray_table=self.ray if self.spherical else None, correction=self.correction, contribution=contribution)

    def oracle(self, alphas=None, F_nu=None):
        import oracle

        a = self.alphas if alphas is None else alphas
        with np.errstate(all="ignore"):
            if self.spherical:
                return oracle.raytrace(self.nus, self.temps, None, self.thetas, self.weights, a, track=True, spherical_r=self.r, reference_r=self.reference_r)
            return oracle.raytrace(self.nus, self.temps, self.dist, self.thetas, self.weights, a, F_nu=F_nu, track=True)

    def reference(self):
        """-> dict(Ft, It, Fo, Io): computed once, left unchanged"""
        if self._ref is None:
            Ft, It = self.truth()
            Fo, Io = self.oracle()
            for a in (Ft, It, Fo, Io):
                a.setflags(write=False)
            self._ref = dict(Ft=Ft, It=It, Fo=Fo, Io=Io)
        return self._ref


_cases = {}


def case(n_depth, n_theta, per_class=16, order="grouped", classes=CLASSES, spherical=False):
    """the Case of a shape, cached for the life of the process (seed 100 n_depth + n_theta)"""
    key = (n_depth, n_theta, per_class, order, tuple(classes), spherical)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def per_class(c, a, ref, oracle_values, reduce_angles=False, keep=None):
    """{class: (largest distance of `a` from `ref`, largest distance of the oracle from `ref`)} over the class's columns, both
    over the positions where the oracle is finite.  reduce_angles: intensities (N_d, N_nu, N_theta), the worst ray of a column.
    keep: optional mask of the columns that count (N_nu)."""
    finite = np.isfinite(oracle_values)
    if keep is not None:
        finite = finite & np.asarray(keep, dtype=bool).reshape((1, -1) + (1,) * (finite.ndim - 2))
    da, do = distance(a, ref, finite), distance(oracle_values, ref, finite)
    if reduce_angles:
        da, do = da.max(axis=-1), do.max(axis=-1)
    return {name: (float(da[c.columns(name)].max()), float(do[c.columns(name)].max())) for name in c.classes}


# what the GPU tests measured in this process: (kernel label, quantity, n_depth, n_theta, order, class, kernel's distance, oracle's
# distance); scripts/formal_truth_table.py runs the tests and writes these out
RECORD = []
