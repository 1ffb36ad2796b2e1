"""The continuum opacity on hostile plasmas, judged against an extended-precision evaluation of the reference's own formulas.

truth() walks the five sources of calc_alphas (opacities_solvers/base.py:655-700) and their sum: the tabulated cross-section
(calc_alpha_file, :40-70, np.interp on the table, util.py:99-103) times a density, bound-free (:178-271: calc_contribution_bf :266-271
per level, alpha_spec += alpha_level :233, alpha_bf += alpha_spec :235, alpha_bf *= nu ** -3 :201 :237), free-free (:274-317), Rayleigh
(:74-135, the clip at 2.3e15 Hz :98-99) and Thomson (:139-174).  Every DECISION is taken in fp64 exactly as the reference takes it —
nu >= cutoff_frequency, the interval np.interp picks and its two clamps, nu > 2.3e15, which species a level belongs to and in which order
the levels come, and whether an fp64 value has left the fp64 range (it is infinity from that step on) — and every ARITHMETIC step in numpy
longdouble in the reference's order.  The comparisons are exact in fp64: there is no ambiguity at a boundary and no point is excluded from
any comparison.

hostile_plasmas() builds the cases.  Grids are exact: nus[i] = (K0 - i) 2^38 Hz (0.27 THz apart, about 1.1e15 Hz at the red end), so a
bound-free edge can be placed ON a grid frequency, or an ulp beside it, on purpose; the wavelengths a table is searched at are an input
of their own (sdx_continuum.lambdas, tracing_lambdas at :62) and sit on nodes, on and beyond the table's ends and an ulp beside them.

A kernel is held to bound(): FACTOR times the fp64 oracle's own distance from the truth plus n_ops 2^-53, point by point and relative to
the truth.  Every term of the continuum is non-negative, so a value formed by rounded operations is within (the sum of the relative
roundings on its longest chain, each counted as often as a power repeats it) 2^-53 of the exact value: n_ops() counts them beside the
kernel lines they come from.  Where the truth is exactly zero, not-a-number or infinite, so is the kernel.

What a relative bound cannot hold in fp64, for the oracle either, stays out of the cases by construction and the CPU test checks that it
does: a product that underflows (a subnormal density stands beside normal ones in its sum), a table whose cross-section more than halves
from one node to the next (the interpolation would cancel), a value within a rounding of the end of the fp64 range.

Used by tests/test_continuum_truth_cpu.py (the oracle alone meets the criterion; every class holds what it claims; the routing rule),
tests/test_gpu_continuum_truth.py (every route of the continuum) and scripts/continuum_truth_table.py.
"""
import numpy as np

L = np.longdouble
EXTENDED = bool(np.finfo(L).eps <= 1e-18)  # a host without an extended long double has no truth to offer: the GPU tests skip

FACTOR = 4.0  # tests/formal_solution_truth.py FACTOR
U = 2.0 ** -53

# the reference's constants (stardis_amd/constants.py; opacities_solvers/base.py:21-34, astropy's c, Ryd and sigma_T in cgs)
C_CGS = 29979245800.0
RYD_CM = 109737.31568160003
SIGMA_T = 6.6524587321000005e-25
RYDBERG_FREQUENCY = 3289841960250881.0
BF_CONSTANT = 2.815403624709817e29
FF_CONSTANT = 369234910.67735106
RAYLEIGH_CUT = 2.3e15
RAYLEIGH = dict(n_h=(20.24, 239.2, 2256.0), n_he=(1.913, 4.52, 7.90), n_h2=(28.39, 215.0, 1303.0))  # :111-125

D = 2.0 ** 38  # grid spacing [Hz]
SOURCES = ("file", "bf", "ff", "rayleigh", "electron", "total")

# ---- the routing rule of the fused step, restated (plan_continuum and the planned launch in line_prepass, stardis_amd/csrc/
# stardis_hip.hip; kContDepths, kPreBlock, kBlock, kPreDepths in sdx_kernels.h).  tests/test_continuum_truth_cpu.py holds these lines to
# the source text, the GPU tests hold route_rule() to what sdx_continuum_route reports of the launch.
CONT_DEPTHS, PRE_BLOCK, BLOCK, PRE_DEPTHS = 8, 1024, 256, 64
STAGE_MAX_NODES = 1024  # a 1-D table of at most this many nodes is searched from LDS
TILE_LDS_GATE = 48 * 1024  # the per-depth factors of eight depths (and the staged table) fit this, or the continuum runs untiled
LDS_LIMIT = 64 * 1024  # what a launch may ask for as dynamic LDS


def _ceil(a, b):
    return -(-int(a) // int(b))


def tile_bytes(n_lev, n_table):
    """plan_continuum's tile_shmem: [8][n_lev] coefficients, [8][6] per-depth factors, the staged table"""
    staged = 0 < n_table <= STAGE_MAX_NODES
    return (CONT_DEPTHS * (n_lev + 6) + (2 * n_table if staged else 0)) * 8


def untiled_bytes(n_lev, n_table):
    staged = 0 < n_table <= STAGE_MAX_NODES
    return max(8, (n_lev + (2 * n_table if staged else 0)) * 8)


def planned_bytes(n_lev):
    """the planned launch stages no table and keeps the bound-free edges behind the factors"""
    return (CONT_DEPTHS * (n_lev + 6) + n_lev) * 8


def largest_tiled_level_count(n_table):
    """the largest n_lev the tiles take with this table: from the rule, not from a list"""
    staged = 0 < n_table <= STAGE_MAX_NODES
    return (TILE_LDS_GATE // 8 - (2 * n_table if staged else 0)) // CONT_DEPTHS - 6


def line_blocks(n_cu, n_depth, n_lines):
    """line_prepass: 16 lines per block while all such blocks are resident at once, else 32 (un-culled launches)"""
    pre_lines = 16 if _ceil(n_lines, 16) * _ceil(n_depth, PRE_DEPTHS) <= 2 * n_cu else 32
    return _ceil(n_lines, pre_lines)


def route_rule(n_cu, n_depth, nu_count, n_nu, n_lines, n_lev, n_table, kernel="k_prepass_continuum", plan=False):
    """what sdx_continuum_route must report for a launch (without "n_cu"): kernel = "k_classify_continuum" for the 256-thread tiles that
    ride the classification launch; plan: the step is given a grid plan (honoured only by the tiled pre-pass launch)"""
    threads = BLOCK if kernel == "k_classify_continuum" else PRE_BLOCK
    staged = 0 < n_table <= STAGE_MAX_NODES
    tiles = _ceil(nu_count, threads)
    tiled = tile_bytes(n_lev, n_table) <= TILE_LDS_GATE
    planned = bool(plan and tiled and threads == PRE_BLOCK)
    out = dict(kernel=kernel, tiled=int(tiled), depths_per_block=1, table_in_lds=int(staged and not planned), planned=int(planned), threads=threads,
               tiles=tiles, rows=n_depth, shmem=untiled_bytes(n_lev, n_table))
    if not tiled:
        return out
    dgs = max(1, min(CONT_DEPTHS, (tiles * threads // PRE_BLOCK * n_depth) // (2 * n_cu)))
    if threads == PRE_BLOCK:
        other = line_blocks(n_cu, n_depth, n_lines) + (0 if planned else _ceil(n_nu + 2, PRE_BLOCK))
        slots = max(1, 2 * n_cu - other * _ceil(n_depth, PRE_DEPTHS))
        dgs = max(dgs, min(CONT_DEPTHS, _ceil(tiles * n_depth, slots)))
    else:
        dgs = CONT_DEPTHS
    out.update(depths_per_block=dgs, rows=_ceil(n_depth, dgs), shmem=planned_bytes(n_lev) if planned else tile_bytes(n_lev, n_table))
    return out


def shape_for_depths_per_block(n_cu, n_depth, want, plan=False, n_lev=3, n_table=37):
    """the smallest (n_nu, n_lines) at which the pre-pass launch runs `want` depths per block: few frequency tiles, the launch's line
    blocks take the other block slots of the chip.  n_nu ends three points into its last tile (lanes that return behind the barrier)."""
    best = None
    for n_lines in (4,) + tuple(min(16 * (2 * n_cu - k), 8176) for k in (64, 32, 16, 8, 4)):  # (below indexed_min_lines = 8192)
        for tiles in range(1, 1025):
            n_nu = (tiles - 1) * PRE_BLOCK + 3 if tiles > 1 else 1023
            r = route_rule(n_cu, n_depth, n_nu, n_nu, n_lines, n_lev, n_table, plan=plan)
            if r["depths_per_block"] == want:
                if best is None or n_nu < best[0]:
                    best = (n_nu, n_lines)
                break
    if best is None:
        raise ValueError(f"no shape gives {want} depths per block with {n_cu} compute units and {n_depth} depths")
    return best


# ---- operation counts ------------------------------------------------------------------------------------------------------------
INTERP_OPS = 6  # interp1: two differences and a division (3), x - xp[lo] (1), the product (1) -> 5 on a term no larger than the result
#                 (ascending: fp[lo] >= 0; descending: the cross-section at most halves per node), the sum (1)
COEF_OPS = 20  # k_bf_coef / the LDS staging: Ryd / cutoff (1), sqrt (x 1/2, 1), zi * (1): r to 2.5; r2 = r r (6), r4 = r2 r2 (13),
#                n5 = r4 r (16.5); (BF zi^4) n (2); the division (1): 19.5
INV3_OPS = 3  # inv_nu3: nu nu, (nu nu) nu, 1 / that
RAYLEIGH_OPS = 30  # alpha_rayleigh_point: c Ryd (1), nu / (2 that) (1): r to 2; r2 (5), r4 (11), r6 = r4 r2 (17), r8 = r4 r4 (23); a
#                    coefficient 20.24 n + 1.913 n' + 28.39 n'' (3); c8 r8 (27), two sums (29), sigma_T (30)


def n_ops(c):
    """-> dict source -> the relative roundings on the longest chain of a value of case c (docstring), None where c has no such source"""
    out = dict.fromkeys(SOURCES)
    added = 0
    if c.xp is not None:
        out["file"] = INTERP_OPS + 1  # sigma n[d]
        added += 1
    added += len(c.planes)
    if c.n_species:
        out["bf"] = COEF_OPS + c.n_lev + c.n_species + INV3_OPS + 1  # spec += per level, bf += per species, bf inv3
    if c.ff_ions is not None and len(c.ff_ions):
        out["ff"] = 4 + len(c.ff_ions) + INV3_OPS + 1  # n / sqrt(T) (2), FF ion^2 (1), their product (1); the sum; ff inv3
    if c.rayleigh:
        out["rayleigh"] = RAYLEIGH_OPS
    if c.n_e is not None:
        out["electron"] = 1
    present = [v for k, v in out.items() if v is not None]
    added += sum(out[k] is not None for k in ("bf", "ff", "rayleigh", "electron"))
    out["total"] = (max(present) if present else 0) + added  # t = t + source, in calc_alphas' order
    return out


def bound(oracle_distance, ops):
    """what a kernel's pointwise distance from the truth, relative to the truth, may be"""
    return FACTOR * float(oracle_distance) + ops * U


# ---- the truth -------------------------------------------------------------------------------------------------------------------
_F64_END = L(2.0) ** 1024 * (L(1) - L(2.0) ** -54)  # from here on fp64 rounds to infinity


def _r(x):
    """an fp64 value that has left the fp64 range is infinity from that step on"""
    x = np.asarray(x, dtype=L)
    if np.any(np.abs(x) >= _F64_END):
        x = np.where(np.abs(x) >= _F64_END, np.copysign(L(np.inf), x), x)
    return x


def interp_truth(x, xp, fp):
    """np.interp: the clamps and the interval in fp64, slope (x - xp[j]) + fp[j] in longdouble -> (value, kind per point):
    kind 0 clamped below, 1 clamped above, 2 on a node, 3 inside an interval"""
    x, xp, fp = (np.asarray(a, dtype=np.float64) for a in (x, xp, fp))
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, xp.size - 2)  # the largest j with xp[j] <= x
    kind = np.full(x.shape, 3, dtype=np.int8)
    kind[xp[j] == x] = 2
    kind[x >= xp[-1]] = 1
    kind[x <= xp[0]] = 0
    xl, xpl, fpl = x.astype(L), xp.astype(L), fp.astype(L)
    slope = (fpl[j + 1] - fpl[j]) / (xpl[j + 1] - xpl[j])
    val = slope * (xl - xpl[j]) + fpl[j]
    val = np.where(kind == 2, fpl[j], val)
    val = np.where(kind == 1, fpl[-1], val)
    val = np.where(kind == 0, fpl[0], val)
    return val, kind


def inv_nu3(nus):
    nl = np.asarray(nus, dtype=np.float64).astype(L)
    with np.errstate(all="ignore"):
        return _r(L(1) / (nl * nl * nl))  # tracing_nus ** -3 (:201, :298)


def species_of_levels(offs):
    """level -> species, in plasma order (:216-221)"""
    offs = np.asarray(offs, dtype=np.int64)
    return np.repeat(np.arange(offs.size - 1), np.diff(offs))


def truth(c):
    """-> dict source -> (n_depth, n_nu) longdouble plane, None where case c has no such source; "total" always"""
    nd, nn = c.n_depth, c.n_nu
    nus = np.asarray(c.nus, dtype=np.float64)
    out = dict.fromkeys(SOURCES)
    total = np.zeros((nd, nn), dtype=L)
    with np.errstate(all="ignore"):
        if c.xp is not None:
            sig, _ = interp_truth(c.lambdas, c.xp, c.fp)
            out["file"] = _r(sig[None, :] * c.table_density.astype(L)[:, None])  # :70
            total = _r(total + out["file"])
        for p in c.planes:
            total = _r(total + np.asarray(p, dtype=np.float64).astype(L))
        inv3 = inv_nu3(nus) if (c.n_species or (c.ff_ions is not None and len(c.ff_ions))) else None
        if c.n_species:
            bf = np.zeros((nd, nn), dtype=L)
            sp_of = species_of_levels(c.offs)
            for s in range(c.n_species):
                spec = np.zeros((nd, nn), dtype=L)  # alpha_spec (:214)
                zi = int(c.bf_ions[s]) + 1
                for lev in np.flatnonzero(sp_of == s):
                    cut = L(c.cutoff[lev])
                    r = L(zi) * np.sqrt(L(RYDBERG_FREQUENCY) / cut)
                    n5 = r * r * r * r * r  # :267
                    coef = _r(_r(L(BF_CONSTANT) * L(zi ** 4) * c.level_density[lev].astype(L)) / n5)  # :268
                    on = nus >= c.cutoff[lev]  # :266, in fp64
                    spec = _r(spec + np.where(on[None, :], coef[:, None], L(0)))  # :233
                bf = _r(bf + spec)  # :235
            out["bf"] = _r(bf * inv3[None, :])  # :237
            total = _r(total + out["bf"])
        if c.ff_ions is not None and len(c.ff_ions):
            ff = np.zeros(nd, dtype=L)
            for s, ion in enumerate(c.ff_ions):
                v = _r(c.ff_density[s].astype(L) / np.sqrt(c.temps.astype(L)))  # :310
                v = _r(v * (L(FF_CONSTANT) * L(int(ion) ** 2)))  # :312
                ff = _r(ff + v)  # :313
            out["ff"] = _r(ff[:, None] * inv3[None, :])  # :315
            total = _r(total + out["ff"])
        if c.rayleigh:
            nuc = np.where(nus > RAYLEIGH_CUT, 0.0, nus).astype(L)  # :99, in fp64
            r = nuc / (L(2) * (L(C_CGS) * L(RYD_CM)))  # :97, :100
            r2 = r * r
            r4 = r2 * r2
            c4, c6, c8 = (np.zeros(nd, dtype=L) for _ in range(3))
            for key in ("n_h", "n_he", "n_h2"):  # :111-125
                dens = getattr(c, key)
                if dens is not None:
                    k4, k6, k8 = RAYLEIGH[key]
                    c4, c6, c8 = _r(c4 + L(k4) * dens.astype(L)), _r(c6 + L(k6) * dens.astype(L)), _r(c8 + L(k8) * dens.astype(L))
            a = c4[:, None] * r4[None, :] + c6[:, None] * (r4 * r2)[None, :] + c8[:, None] * (r4 * r4)[None, :]  # :127-131
            out["rayleigh"] = _r(_r(a) * L(SIGMA_T))  # :133
            total = _r(total + out["rayleigh"])
        if c.n_e is not None:
            out["electron"] = np.repeat(_r(L(SIGMA_T) * c.n_e.astype(L))[:, None], nn, axis=1)  # :166-172
            total = _r(total + out["electron"])
    out["total"] = total
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def oracle_planes(c):
    """the fp64 oracle's five planes and their sum in calc_alphas' order -> dict like truth()"""
    import oracle

    nd, nn = c.n_depth, c.n_nu
    out = dict.fromkeys(SOURCES)
    total = np.zeros((nd, nn))
    with np.errstate(all="ignore"):
        if c.xp is not None:
            out["file"] = oracle.alpha_file_1d(c.lambdas, c.xp, c.fp, c.table_density)
            total = total + out["file"]
        for p in c.planes:
            total = total + p
        if c.n_species:
            out["bf"] = oracle.alpha_bf(c.nus, c.offs, c.bf_ions, c.cutoff, c.level_density)
            total = total + out["bf"]
        if c.ff_ions is not None and len(c.ff_ions):
            out["ff"] = oracle.alpha_ff(c.nus, c.temps, c.ff_ions, c.ff_density)
            total = total + out["ff"]
        if c.rayleigh:
            if c.n_h is None and c.n_he is None and c.n_h2 is None:  # (no species: the coefficients of :107-109 stay zero)
                out["rayleigh"] = np.zeros((nd, nn))
            else:
                out["rayleigh"] = oracle.alpha_rayleigh(np.array(c.nus, dtype=np.float64), c.n_h, c.n_he, c.n_h2)
            total = total + out["rayleigh"]
        if c.n_e is not None:
            out["electron"] = oracle.alpha_electron(nn, c.n_e)
            total = total + out["electron"]
    out["total"] = total
    return out


def distance(a, ref, where=None):
    """the largest pointwise |a - ref| / ref over the points where ref is finite and not zero (and `where` holds); 0.0 when there is
    none"""
    a, ref = np.asarray(a).astype(L), np.asarray(ref).astype(L)
    m = np.isfinite(ref) & (ref != 0)
    if where is not None:
        m = m & where
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        return float((np.abs(a[m] - ref[m]) / np.abs(ref[m])).max())


def same_special_values(got, ref):
    """zeros, NaNs and infinities (with their sign) at the same points"""
    got, ref = np.asarray(got), np.asarray(ref)
    return (np.array_equal(got == 0, ref == 0) and np.array_equal(np.isnan(got), np.isnan(ref))
            and np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)))


RECORD = []  # what the GPU tests measured in this process: dicts, see judge(); scripts/continuum_truth_table.py writes them out


def judge(c, source, got, route="", label="", cols=None, record=RECORD, ran=None):
    """the asserts of a fp64 plane `got` of source `source` of case c against the truth: the zero / NaN / infinity pattern, and the
    pointwise distance within bound() on every other point -> (distance, allowed).  cols: the columns of the case `got` holds (a
    shard); ran: the route and depths per block the caller asserted, for the record.  One record per class of columns."""
    ref = c.reference()
    t = ref["truth"][source]
    assert t is not None, (c.name, source)
    cls = c.col_cls
    if cols is not None:
        t, cls = t[:, cols], cls[cols]
    got = np.asarray(got)
    assert got.shape == t.shape and got.dtype == np.float64, (c.name, route, source, got.shape, t.shape)
    assert same_special_values(got, t), (c.name, route, source, "zeros, NaNs or infinities differ from the truth")
    ops, o_dist = ref["n_ops"][source], ref["oracle_distance"][source]
    allowed = bound(o_dist, ops)
    worst = 0.0
    for k in np.unique(cls):
        m = np.broadcast_to((cls == k)[None, :], t.shape)
        o_ref = ref["oracle"][source] if cols is None else ref["oracle"][source][:, cols]
        dist, o_k = distance(got, t, m), distance(o_ref, t, m)
        worst = max(worst, dist)
        if record is not None:
            record.append(dict(route=route, label=label, source=source, case=c.name, cls=str(k), n_depth=c.n_depth, n_nu=int(t.shape[1]), kernel=dist,
                               oracle=o_k, n_ops=ops, bound=allowed, ran=ran))
    print(f"{c.name:28s} {route:2s} {label:30s} {source:9s} kernel {worst:.3e} oracle {o_dist:.3e} bound {allowed:.3e} ({ops} ops)")
    assert worst <= allowed, (c.name, route, label, source, worst, allowed)
    return worst, allowed


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def grid(n_nu, k0=None):
    """descending, exact: nus[i] = (k0 - i) D, k0 = 4096 + n_nu unless given (the red end at 4097 D = 1.126e15 Hz)"""
    k0 = 4096 + n_nu if k0 is None else k0
    assert k0 - n_nu >= 1 and k0 * D < 2.0 ** 53
    return (k0 - np.arange(n_nu, dtype=np.float64)) * D


def nu_to_angstrom(nus):
    from stardis_amd import constants as K

    return K.nu_to_angstrom(np.asarray(nus, dtype=np.float64))


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


class Case:
    """one plasma of a class: the inputs of the five sources in the layout sdx_continuum takes them, col_cls[i] the class of column i.
    A source that is absent is None (n_species = 0 for bound-free)."""

    def __init__(self, cls, name, nus, n_depth, seed):
        self.cls, self.name, self.n_depth = cls, name, int(n_depth)
        self.nus = np.ascontiguousarray(nus, dtype=np.float64)
        self.n_nu = self.nus.size
        self.rng = np.random.default_rng(seed)
        self.lambdas = nu_to_angstrom(self.nus)
        self.col_cls = np.full(self.n_nu, cls, dtype=object)
        self.xp = self.fp = self.table_density = None
        self.offs, self.bf_ions, self.cutoff, self.level_density = np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros((0, n_depth))
        self.ff_ions = self.ff_density = None
        self.temps = np.linspace(4000.0, 9000.0, n_depth) if n_depth > 1 else np.array([5777.0])
        self.n_h = self.n_he = self.n_h2 = None
        self.rayleigh = False
        self.n_e = None
        self.planes = []
        self.notes = {}
        self._ref = None

    # -- sizes
    @property
    def n_species(self):
        return int(np.asarray(self.bf_ions).size)

    @property
    def n_lev(self):
        return int(np.asarray(self.cutoff).size)

    @property
    def n_table(self):
        return 0 if self.xp is None else int(self.xp.size)

    # -- sources with benign values (a class overwrites what it is about)
    def density(self, lo=1e8, hi=1e14, shape=None):
        shape = (self.n_depth,) if shape is None else shape
        return np.ascontiguousarray(10.0 ** self.rng.uniform(np.log10(lo), np.log10(hi), shape))

    def table(self, xp, fp=None):
        self.xp = np.ascontiguousarray(xp, dtype=np.float64)
        assert np.all(np.diff(self.xp) > 0)
        if fp is None:  # up and down, never more than halving per node (INTERP_OPS)
            fp = 4e-17 * np.exp(np.cumsum(self.rng.uniform(-0.6, 0.6, self.xp.size)))
        self.fp = np.ascontiguousarray(fp, dtype=np.float64)
        self.table_density = self.density(1e4, 1e9)
        return self

    def bound_free(self, offs, ions, cutoff):
        self.offs, self.bf_ions = np.asarray(offs, dtype=np.int32), np.asarray(ions, dtype=np.int32)
        self.cutoff = np.ascontiguousarray(cutoff, dtype=np.float64)
        assert self.offs[0] == 0 and self.offs[-1] == self.cutoff.size and self.offs.size == self.bf_ions.size + 1
        self.level_density = self.density(1e2, 1e12, (self.cutoff.size, self.n_depth))
        return self

    def free_free(self, ions):
        self.ff_ions = np.asarray(ions, dtype=np.int32)
        self.ff_density = self.density(1e20, 1e28, (self.ff_ions.size, self.n_depth))  # n_e n_ion (util.py:160-164)
        return self

    def rayleigh_of(self, h=True, he=True, h2=True):
        self.rayleigh = True
        self.n_h = self.density(1e12, 1e17) if h else None
        self.n_he = self.density(1e11, 1e16) if he else None
        self.n_h2 = self.density(1e8, 1e13) if h2 else None
        return self

    def electrons(self):
        self.n_e = self.density(1e10, 1e15)
        return self

    def everything(self, n_table=37):
        """every source present, benign: a table over the grid's wavelengths, two species with edges inside the grid, one free-free
        species, Rayleigh on H and He, electrons"""
        lam = self.lambdas
        self.table(np.linspace(lam.min() * 1.01, lam.max() * 0.99, n_table) if lam.min() < lam.max() else lam[0] * np.linspace(0.9, 1.1, n_table))
        span = (self.nus[-1], self.nus[0]) if self.n_nu > 1 else (0.5 * self.nus[0], 2.0 * self.nus[0])
        self.bound_free([0, 2, 3], [0, 1], self.rng.uniform(*span, 3))
        return self.free_free([1]).rayleigh_of(True, True, False).electrons()

    def reference(self):
        """-> dict(truth, oracle: planes per source; n_ops, oracle_distance per source): computed once, left unchanged"""
        if self._ref is None:
            t, o = truth(self), oracle_planes(self)
            for v in o.values():
                if v is not None:
                    v.setflags(write=False)
            self._ref = dict(truth=t, oracle=o, n_ops=n_ops(self),
                             oracle_distance={k: (distance(o[k], t[k]) if t[k] is not None else None) for k in SOURCES})
        return self._ref

    def sources(self):
        return [k for k in SOURCES[:-1] if self.reference()["truth"][k] is not None]

    def take(self, cols, name):
        """the same plasma on the columns `cols` of the grid (an index array or a slice), in that order"""
        import copy

        o = copy.copy(self)
        o.name = name
        o.nus, o.lambdas, o.col_cls = np.ascontiguousarray(self.nus[cols]), np.ascontiguousarray(self.lambdas[cols]), self.col_cls[cols]
        o.n_nu = o.nus.size
        o.planes = [np.ascontiguousarray(p[:, cols]) for p in self.planes]
        o._ref = None
        return o


def _edge_on_grid():
    """levels of two species, interleaved, whose edges are a grid frequency, the next fp64 above and the next below, at the first, an
    interior and the last grid point; one level above the whole grid (its term is exactly 0) and one below"""
    c = Case("edge_on_grid", "edge_on_grid", grid(1025), 9, 21).everything()
    pts = (0, 513, c.n_nu - 1)
    cut = []
    for p in pts:
        cut += [c.nus[p], up(c.nus[p]), down(c.nus[p])]
    cut += [1.5 * c.nus[0], 0.5 * c.nus[-1]]
    order = np.array([0, 4, 8, 9, 1, 5, 2, 6, 10, 3, 7])
    c.bound_free([0, 4, 11], [0, 1], np.array(cut)[order])
    for p in pts:
        c.col_cls[p] = "edge_on_grid"
        for q in (p - 1, p + 1):
            if 0 <= q < c.n_nu:
                c.col_cls[q] = "edge_beside_grid_point"
    c.notes["points"] = pts
    return c


def _edge_outside(above):
    c = Case("edge_above_grid" if above else "edge_below_grid", "edge_above_grid" if above else "edge_below_grid", grid(257), 7, 22 + above)
    c.everything()
    f = (up(c.nus[0]), 1.2 * c.nus[0], 3.0 * c.nus[0]) if above else (down(c.nus[-1]), 0.8 * c.nus[-1], 0.1 * c.nus[-1])
    c.bound_free([0, 1, 3], [1, 0], f)
    return c


TABLE_NODES = (2, 37, 1024, 1025)


def _table_nodes(n_table):
    """wavelengths on nodes, on xp[0] and xp[-1], beyond both ends, an ulp inside each end and an ulp beside interior nodes"""
    n_nu, n_depth = {2: (255, 7), 37: (1023, 8), 1024: (1025, 9), 1025: (1024, 17)}[n_table]
    c = Case("table_nodes", f"table_nodes_{n_table}", grid(n_nu), n_depth, 30 + n_table).everything()
    rng = c.rng
    xp = np.cumsum(rng.uniform(0.5, 3.0, n_table)) + 1500.0
    c.table(xp)
    lam = rng.uniform(xp[0], xp[-1], n_nu)
    kinds = np.full(n_nu, "inside_interval", dtype=object)
    hostile = [(xp[0], "table_end"), (xp[-1], "table_end"), (down(xp[0]), "beyond_table"), (0.5 * xp[0], "beyond_table"), (up(xp[-1]), "beyond_table"),
               (2.0 * xp[-1], "beyond_table"), (up(xp[0]), "ulp_inside_end"), (down(xp[-1]), "ulp_inside_end")]
    inner = np.unique(np.concatenate([[0, n_table - 1, n_table // 2], rng.integers(0, n_table, 40)]))
    for j in inner:
        hostile.append((xp[j], "table_end" if j in (0, n_table - 1) else "on_node"))
        if 0 < j < n_table - 1:
            hostile += [(up(xp[j]), "ulp_beside_node"), (down(xp[j]), "ulp_beside_node")]
    at = rng.permutation(n_nu)[:len(hostile)]  # anywhere in the grid: first, last and ragged tiles alike
    assert len(hostile) <= n_nu
    for i, (v, k) in zip(at, hostile):
        lam[i], kinds[i] = v, k
    c.lambdas = np.ascontiguousarray(lam)
    c.col_cls = kinds
    return c


def rayleigh_grid(n_nu, n_above):
    """descending and exact, with 2.3e15 Hz (a multiple of 2^14) on it between its two fp64 neighbours"""
    above = RAYLEIGH_CUT + np.arange(n_above, 0, -1) * D
    below = RAYLEIGH_CUT - np.arange(1, n_nu - n_above - 2) * D
    return np.concatenate([above, [up(RAYLEIGH_CUT), RAYLEIGH_CUT, down(RAYLEIGH_CUT)], below])


def _rayleigh_cut(h, he, h2):
    name = "rayleigh_cut_" + ("".join(k for k, on in (("H", h), ("He", he), ("H2", h2)) if on) or "none")
    c = Case("rayleigh_cut", name, rayleigh_grid(255, 40), 7, 40 + 4 * h + 2 * he + h2).everything()
    c.rayleigh_of(h, he, h2)
    c.col_cls[:40] = "far_above_cut"
    c.col_cls[40], c.col_cls[41], c.col_cls[42] = "ulp_above_cut", "at_cut", "ulp_below_cut"
    c.col_cls[43:] = "below_cut"
    return c


def _species_shapes(kind):
    c = Case("species_shapes", f"species_{kind}", grid(256), 17, 50 + len(kind)).everything()
    edges = lambda n: c.rng.uniform(c.nus[-1], c.nus[0], n)  # noqa: E731
    if kind == "none":
        c.bound_free([0], [], np.zeros(0))
        c.ff_ions = c.ff_density = None
    elif kind == "one":
        c.bound_free([0, 5], [0], edges(5)).free_free([1])
    elif kind == "three_interleaved":  # the G14 shape: species A holds levels 0 3 6 9 of the plasma, B 1 4 7, C 2 5 8
        order = np.array([0, 3, 6, 9, 1, 4, 7, 2, 5, 8])
        c.bound_free([0, 4, 7, 10], [0, 0, 1], np.sort(edges(10))[order]).free_free([1, 1, 2])
    elif kind == "empty_species":  # offs[s] == offs[s + 1]: first, middle and last
        c.bound_free([0, 0, 3, 3, 6, 6], [0, 1, 0, 2, 1], edges(6)).free_free([1, 2])
    elif kind == "ions_0_1_2":
        c.bound_free([0, 2, 4, 6], [0, 1, 2], edges(6)).free_free([1, 2, 3])
    elif kind == "ff_ion_zero":  # ion_number = 0: a term that is exactly zero, alone and beside others
        c.bound_free([0, 2], [0], edges(2)).free_free([0, 1, 0])
    elif kind == "ff_only_ion_zero":
        c.bound_free([0, 2], [0], edges(2)).free_free([0])
    return c


def _level_counts(n_lev, n_table):
    """levels of three species; a twentieth of the edges on grid frequencies, the rest between them, some outside the grid"""
    c = Case("level_counts", f"levels_{n_lev}_table_{n_table}", grid(257), 9, 60 + n_lev + n_table).everything(n_table if n_table else 37)
    if not n_table:
        c.xp = c.fp = c.table_density = None
    rng = c.rng
    cut = rng.uniform(0.9 * c.nus[-1], 1.1 * c.nus[0], n_lev)
    on = rng.permutation(n_lev)[:max(1, n_lev // 20)]
    cut[on] = c.nus[rng.integers(0, c.n_nu, on.size)]
    a, b = n_lev // 3, n_lev // 3 + n_lev // 2
    c.bound_free([0, a, b, n_lev], [0, 1, 0], cut)
    c.level_density = c.density(1e2, 1e9, (n_lev, c.n_depth))
    return c


def level_count_cases():
    """on both sides of both thresholds, from the rule: with a staged table of 1024 nodes, and with none"""
    a, b = largest_tiled_level_count(STAGE_MAX_NODES), largest_tiled_level_count(0)
    return ((1, 1024), (10, 1024), (a, 1024), (a + 1, 1024), (b, 0), (b + 1, 0), (4096, 0))


def _densities(kind):
    c = Case("densities", f"densities_{kind}", grid(1024), 8, 70 + len(kind)).everything()
    c.rayleigh_of(True, True, True)
    c.free_free([1, 2])
    if kind == "zero_rows":  # whole depth rows of exact zeros, in every source -> rows of the total that are exactly zero
        for d in (0, 3, 7):
            for a in (c.table_density, c.n_h, c.n_he, c.n_h2, c.n_e):
                a[d] = 0.0
            c.level_density[:, d] = 0.0
            c.ff_density[:, d] = 0.0
        c.level_density[:, 5] = 0.0  # ... and in one source alone
        c.n_he[6] = 0.0
    elif kind == "zero_levels":
        c.level_density[1, :] = 0.0
        c.level_density[2, ::2] = 0.0
        c.ff_density[0, :] = 0.0
    elif kind == "subnormal":  # beside normal values in the same sum (docstring): the sum holds the bound, the tiny term vanishes in it
        c.cutoff[1] = 0.5 * c.nus[-1]  # the level that stays normal contributes at every frequency
        c.level_density[0, :] = 5e-324
        c.level_density[2, 1::2] = 1e-310
        c.ff_density[1, :] = 3e-312
        c.n_h2[:] = 1e-315
        c.n_he[::2] = 5e-324
    elif kind == "overflow":  # rows 1 and 2: a coefficient beyond the fp64 range; row 4: finite free-free terms whose sum is not
        c.level_density[0, 1] = 1e300
        c.level_density[:, 2] = 3e299
        c.temps = c.temps.copy()
        c.temps[4] = 1e4
        c.ff_ions = np.array([1, 1], dtype=np.int32)
        c.ff_density[:, 4] = 4e301
        c.n_e[5] = 1e300  # (finite: sigma_T n_e)
    return c


def _file_planes(n):
    c = Case("file_planes", f"file_planes_{n}", grid(1025), 7, 80 + n).everything()
    c.planes = [np.ascontiguousarray(c.density(1e-12, 1e-6, (c.n_depth, c.n_nu))) for _ in range(n)]
    if n:
        c.planes[0][2, :] = 0.0
        c.planes[-1][:, 5] = 0.0
    return c


def _shape(n_nu, n_depth):
    """every source, benign values, edges on three grid points: the shapes of the issue's list that no class above has"""
    c = Case("shapes", f"shape_{n_nu}x{n_depth}", grid(n_nu), n_depth, 90 + n_nu + n_depth).everything()
    if n_nu > 2:
        c.cutoff[:] = c.nus[[0, n_nu // 2, n_nu - 1]]
    else:
        c.cutoff[:] = [c.nus[0], up(c.nus[0]), down(c.nus[0])]
    return c


def _clipped_in_place():
    """route A only: the frequencies calc_alpha_rayleigh has zeroed in its caller's array (:99), handed on to bound-free and free-free:
    nu ** -3 is infinite there, a bound-free sum of zeros times it NaN"""
    c = Case("clipped_in_place", "clipped_in_place", rayleigh_grid(257, 60), 7, 99).everything()
    c.bound_free([0, 2, 3], [0, 1], [c.nus[100], 0.0, c.nus[200]])  # (a level with no edge at all: on at nu = 0 too)
    c.level_density[1, 3] = 0.0
    c.col_cls[:61] = "clipped"
    c.col_cls[61:] = "kept"
    return c


_BUILDERS = {"edge_on_grid": _edge_on_grid, "edge_above_grid": lambda: _edge_outside(True), "edge_below_grid": lambda: _edge_outside(False)}
for _n in TABLE_NODES:
    _BUILDERS[f"table_nodes_{_n}"] = (lambda n=_n: _table_nodes(n))
for _h in (0, 1):
    for _he in (0, 1):
        for _h2 in (0, 1):
            _BUILDERS["rayleigh_cut_" + ("".join(k for k, on in (("H", _h), ("He", _he), ("H2", _h2)) if on) or "none")] = (
                lambda h=_h, he=_he, h2=_h2: _rayleigh_cut(h, he, h2))
SPECIES_KINDS = ("none", "one", "three_interleaved", "empty_species", "ions_0_1_2", "ff_ion_zero", "ff_only_ion_zero")
for _k in SPECIES_KINDS:
    _BUILDERS[f"species_{_k}"] = (lambda k=_k: _species_shapes(k))
for _nl, _nt in level_count_cases():
    _BUILDERS[f"levels_{_nl}_table_{_nt}"] = (lambda nl=_nl, nt=_nt: _level_counts(nl, nt))
DENSITY_KINDS = ("zero_rows", "zero_levels", "subnormal", "overflow")
for _k in DENSITY_KINDS:
    _BUILDERS[f"densities_{_k}"] = (lambda k=_k: _densities(k))
for _n in (0, 4):
    _BUILDERS[f"file_planes_{_n}"] = (lambda n=_n: _file_planes(n))
SHAPES = ((1, 1), (1, 7), (255, 1), (256, 8), (257, 17), (1023, 9), (1024, 7))
for _nn, _nd in SHAPES:
    _BUILDERS[f"shape_{_nn}x{_nd}"] = (lambda nn=_nn, nd=_nd: _shape(nn, nd))

NAMES = tuple(_BUILDERS)  # every case of routes A and B
_BUILDERS["clipped_in_place"] = _clipped_in_place
CLASSES = ("edge_on_grid", "edge_above_grid", "edge_below_grid", "table_nodes", "rayleigh_cut", "species_shapes", "level_counts", "densities",
           "file_planes", "shapes", "clipped_in_place")
# the fused step takes at least two depths and a grid of more than one point
FUSED_NAMES = tuple(n for n in NAMES if not (n.startswith("shape_") and (n.startswith("shape_1x") or n.endswith("x1"))))

_cases = {}


def case(name):
    """the Case of a name, cached for the life of the process"""
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def hostile_plasmas(names=NAMES):
    for name in names:
        yield case(name)


def benign_for_depths_per_block(n_nu, n_depth, seed=7):
    """a plain plasma on a grid sized for a depths-per-block case: three levels, the 37-node table, edges on grid points of the first,
    an interior and the last (ragged) tile"""
    c = Case("depths_per_block", f"dgs_{n_nu}x{n_depth}", grid(n_nu), n_depth, seed).everything()
    c.cutoff[:] = c.nus[[0, min(n_nu - 1, 1024), n_nu - 1]]
    return c
