"""Every route of the continuum opacity against the 80-bit truth on hostile plasmas (tests/continuum_truth.py).

A  the stand-alone sources (ops.alpha_file_1d / alpha_bf / alpha_ff / alpha_rayleigh / alpha_electron);
B  the stand-alone sum k_total_alphas (sdx_total_alphas_dev: the whole grid, a shard with an odd first column, one source at a time) and
   its host-buffer twin sdx_continuum_f64;
C  the fused step's untiled blocks, D its depth-group tiles, E the planned tiles, F the tiles that ride the classification launch of
   the two-collective mode — each from a fused step whose continuum description is the hostile plasma, with four lines of zero strength
   (their plane is +0.0 everywhere: total_alphas() is the continuum plane).

Each route is held to bound() point by point, with the zero / NaN / infinity pattern of the truth; all routes give the bits of route B;
and each fused test asserts, from the launch site's own report (sdx_continuum_route), the route and the depths per block it ran —
which is what the restated rule says (continuum_truth.route_rule, held to the source text by the CPU test)."""
import ctypes as C

import numpy as np
import pytest

import continuum_truth as T
from stardis_amd import _lib, ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not T.EXTENDED, reason="numpy.longdouble is not an extended type here")]

PREFIX = 16401  # columns in front of a case's grid in route F: a grid beyond the in-block spacing scan (16384), an odd first column


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def continuum_of(ctx, c, keep, only=None, prefix=0, temperature=None):
    """sdx_continuum of device pointers for case c (only: one source of it; prefix: that many columns of a longer grid in front)"""
    def up(a, dt=np.float64):
        keep.append(ctx.upload(np.ascontiguousarray(a, dtype=dt), dt))
        return keep[-1].ptr

    want = lambda k: only is None or only == k  # noqa: E731
    pad = lambda a: np.concatenate([np.full(prefix, a[0]), a]) if prefix else a  # noqa: E731
    s = _lib.Continuum()
    s.temperature = temperature if temperature is not None else up(c.temps)
    if c.xp is not None and want("file"):
        s.lambdas, s.n_table = up(pad(c.lambdas)), c.n_table
        s.table_wavelength, s.table_sigma, s.table_density = up(c.xp), up(c.fp), up(c.table_density)
    if only is None and c.planes:
        s.n_file_planes, s.file_plane_ld = len(c.planes), c.n_nu + prefix
        for k, p in enumerate(c.planes):
            s.file_plane[k] = up(np.concatenate([np.zeros((c.n_depth, prefix)), p], axis=1) if prefix else p)
    if c.n_species and want("bf"):
        s.bf_n_species, s.bf_n_levels = c.n_species, c.n_lev
        s.bf_species_offsets, s.bf_species_ion_number = up(c.offs, np.int32), up(c.bf_ions, np.int32)
        s.bf_cutoff, s.bf_level_density = up(c.cutoff), up(c.level_density)
    if c.ff_ions is not None and len(c.ff_ions) and want("ff"):
        s.ff_n_species, s.ff_species_ion_number, s.ff_number_density = len(c.ff_ions), up(c.ff_ions, np.int32), up(c.ff_density)
    if c.rayleigh and want("rayleigh"):
        s.rayleigh_enabled = 1
        s.ray_n_h, s.ray_n_he, s.ray_n_h2 = (None if a is None else up(a) for a in (c.n_h, c.n_he, c.n_h2))
    if c.n_e is not None and want("electron"):
        s.electron_density = up(c.n_e)
    return s


def route_a(ctx, c):
    """the five stand-alone sources -> dict source -> plane"""
    out = {}
    if c.xp is not None:
        out["file"] = ops.alpha_file_1d(c.lambdas, c.xp, c.fp, c.table_density, ctx=ctx).numpy()
    if c.n_species:
        out["bf"] = ops.alpha_bf(c.nus, c.offs, c.bf_ions, c.cutoff, c.level_density, c.n_depth, ctx=ctx).numpy()
    if c.ff_ions is not None and len(c.ff_ions):
        out["ff"] = ops.alpha_ff(c.nus, c.temps, c.ff_ions, c.ff_density, ctx=ctx).numpy()
    if c.rayleigh:
        plane, clipped = ops.alpha_rayleigh(c.nus, c.n_depth, c.n_h, c.n_he, c.n_h2, ctx=ctx)
        out["rayleigh"] = plane.numpy()
        assert np.array_equal(clipped, np.where(c.nus > T.RAYLEIGH_CUT, 0.0, c.nus))
    if c.n_e is not None:
        out["electron"] = ops.alpha_electron(c.n_nu, c.n_e, ctx=ctx).numpy()
    return out


def route_b(ctx, c, only=None, begin=0, count=None):
    """sdx_total_alphas_dev on columns [begin, begin + count) -> plane"""
    keep = []
    count = c.n_nu - begin if count is None else count
    s = continuum_of(ctx, c, keep, only=only)
    d_nus = ctx.upload(c.nus)
    out = ctx.empty((c.n_depth, count))
    ctx.call("sdx_total_alphas_dev", c.n_depth, c.n_nu, d_nus.ptr, begin, count, C.byref(s), None, 0, out.ptr, count)
    return out.numpy()


_b_total = {}


def b_total(ctx, c):
    """route B's total of a case: computed once, shared by the tests that compare with it"""
    if c.name not in _b_total:
        _b_total[c.name] = route_b(ctx, c)
        _b_total[c.name].setflags(write=False)
    return _b_total[c.name]


@pytest.mark.parametrize("name", T.NAMES)
def test_routes_a_and_b(ctx, name):
    c = T.case(name)
    a = route_a(ctx, c)
    assert sorted(a) == sorted(c.sources())
    for src, plane in a.items():
        T.judge(c, src, plane, "A", "ops.alpha_" + src)
        assert bits(route_b(ctx, c, only=src), plane), (name, src)  # each plane of B is A's
    total = b_total(ctx, c)
    T.judge(c, "total", total, "B", "sdx_total_alphas_dev")
    if c.n_nu >= 4:
        begin = min(37, c.n_nu // 2) | 1
        count = c.n_nu - begin - 1
        shard = route_b(ctx, c, begin=begin, count=count)
        assert bits(shard, total[:, begin:begin + count]), name
        T.judge(c, "total", shard, "B", f"shard from column {begin}", cols=slice(begin, begin + count))


@pytest.mark.parametrize("name", [n for n in T.NAMES if n != "file_planes_4"])
def test_host_buffer_twin_equals_route_b(ctx, name):
    """sdx_continuum_f64 takes no device planes (file planes are refused there): every other case"""
    c = T.case(name)
    keep = []

    def ptr(a, dt=np.float64):
        keep.append(np.ascontiguousarray(a, dtype=dt))
        return keep[-1].ctypes.data

    s = _lib.Continuum()
    s.temperature = ptr(c.temps)
    if c.xp is not None:
        s.lambdas, s.n_table, s.table_wavelength, s.table_sigma, s.table_density = ptr(c.lambdas), c.n_table, ptr(c.xp), ptr(c.fp), ptr(c.table_density)
    if c.n_species:
        s.bf_n_species, s.bf_n_levels, s.bf_species_offsets, s.bf_species_ion_number = c.n_species, c.n_lev, ptr(c.offs, np.int32), ptr(c.bf_ions, np.int32)
        s.bf_cutoff, s.bf_level_density = ptr(c.cutoff), ptr(c.level_density)
    if c.ff_ions is not None and len(c.ff_ions):
        s.ff_n_species, s.ff_species_ion_number, s.ff_number_density = len(c.ff_ions), ptr(c.ff_ions, np.int32), ptr(c.ff_density)
    if c.rayleigh:
        s.rayleigh_enabled = 1
        s.ray_n_h, s.ray_n_he, s.ray_n_h2 = (None if a is None else ptr(a) for a in (c.n_h, c.n_he, c.n_h2))
    if c.n_e is not None:
        s.electron_density = ptr(c.n_e)
    present = c.sources()
    out = {k: np.full((c.n_depth, c.n_nu), np.nan) for k in present + ["total"]}
    nus = c.nus.copy()
    ctx.call("sdx_continuum_f64", c.n_depth, c.n_nu, nus.ctypes.data, C.byref(s),
             *(out[k].ctypes.data if k in out else None for k in ("file", "bf", "ff", "rayleigh", "electron", "total")))
    assert np.array_equal(nus, np.where(c.nus > T.RAYLEIGH_CUT, 0.0, c.nus) if c.rayleigh else c.nus)  # (:99)
    assert bits(out["total"], b_total(ctx, c)), name
    a = route_a(ctx, c)
    for src in present:
        assert bits(out[src], a[src]), (name, src)
    T.judge(c, "total", out["total"], "B", "sdx_continuum_f64")


def test_clipped_in_place(ctx):
    """route A: bound-free and free-free on the array ops.alpha_rayleigh has clipped — infinite or NaN exactly where the oracle is"""
    import oracle

    c = T.case("clipped_in_place")
    _, clipped = ops.alpha_rayleigh(c.nus, c.n_depth, c.n_h, c.n_he, c.n_h2, ctx=ctx)
    want = np.array(c.nus)
    oracle.alpha_rayleigh(want, c.n_h, c.n_he, c.n_h2)
    assert np.array_equal(clipped, want) and np.count_nonzero(clipped == 0) == 61
    bf = ops.alpha_bf(clipped, c.offs, c.bf_ions, c.cutoff, c.level_density, c.n_depth, ctx=ctx).numpy()
    ff = ops.alpha_ff(clipped, c.temps, c.ff_ions, c.ff_density, ctx=ctx).numpy()
    with np.errstate(all="ignore"):
        o_bf = oracle.alpha_bf(clipped, c.offs, c.bf_ions, c.cutoff, c.level_density)
        o_ff = oracle.alpha_ff(clipped, c.temps, c.ff_ions, c.ff_density)
    assert T.same_special_values(bf, o_bf) and T.same_special_values(ff, o_ff)
    assert np.isnan(bf).any() and np.isposinf(ff[:, :61]).all()


def test_columns_are_independent_in_the_stand_alone_sum(ctx):
    """permuting the frequency columns permutes the plane bit for bit (k_total_alphas takes the grid in any order)"""
    for name in ("edge_on_grid", "table_nodes_1024", "table_nodes_1025", "file_planes_4"):
        c = T.case(name)
        perm = np.random.default_rng(5).permutation(c.n_nu)
        assert bits(route_b(ctx, c.take(perm, name + "_permuted")), b_total(ctx, c)[:, perm]), name


# ---- the fused step ----------------------------------------------------------------------------------------------------------------
def zero_lines(c, n_lines):
    """lines of zero strength between the grid points: a floor window each, every term +0.0"""
    rng = np.random.default_rng(3)
    ln = np.sort(rng.uniform(c.nus[-1], c.nus[0], n_lines))
    full = np.full((n_lines, c.n_depth), T.D)
    return dict(line_nus=ln, doppler_widths=full, gammas=full.copy(), alphas=np.zeros((n_lines, c.n_depth)))


def fused(ctx, c, plan=False, classify=False, n_lines=4):
    """one eager fused step on case c -> (total_alphas of the case's columns, what sdx_continuum_route reports, what the rule says)"""
    prefix = PREFIX if classify else 0
    nus = np.concatenate([c.nus[0] + np.arange(prefix, 0, -1) * T.D, c.nus]) if prefix else c.nus
    th, w = synth.thetas_and_weights(2)
    kw = dict(ctx=ctx, grid_plan=False, track_evaluations=False)
    if classify:
        kw.update(shard=(prefix, c.n_nu), classify_share=(0, n_lines), m_max=ctx.zeros((n_lines,)))
        ctx.set_option("indexed_min_lines", 1)
    try:
        syn = SpectralSynthesizer(nus, c.temps, np.full(c.n_depth - 1, 1.0e7), th, w, zero_lines(c, n_lines), None, **kw)
        keep = []
        syn.cont = continuum_of(ctx, c, keep, prefix=prefix, temperature=syn.d_t.ptr)
        if plan:
            handle = C.c_void_p()
            ctx.call("sdx_grid_plan_create", syn.n_nu, syn.d_nus.ptr, syn.n_lines, syn.d_ln.ptr, C.byref(syn.cont), C.byref(handle))
            syn.plan = handle
        if classify:
            syn.enqueue_classify()
            syn.enqueue()
            ctx.synchronize()
        else:
            syn.step()
        total, line = syn.total_alphas(), syn.alpha_line()
        ran = ctx.continuum_route()
        syn.close()
    finally:
        if classify:
            ctx.set_option("indexed_min_lines", 8192)
    assert not line.any() and not np.signbit(line).any()
    n_cu = ran.pop("n_cu")
    rule = T.route_rule(n_cu, c.n_depth, c.n_nu, nus.size, n_lines, c.n_lev, c.n_table,
                        kernel="k_classify_continuum" if classify else "k_prepass_continuum", plan=plan)
    return total, ran, rule


def letter(r):
    return "F" if r["kernel"] == "k_classify_continuum" else ("E" if r["planned"] else ("D" if r["tiled"] else "C"))


def check_fused(ctx, c, plan, classify, n_lines=4):
    total, ran, rule = fused(ctx, c, plan=plan, classify=classify, n_lines=n_lines)
    assert ran == rule, (c.name, ran, rule)  # the launch site's decision is the restated rule's
    assert 8 <= ran["shmem"] <= T.LDS_LIMIT
    T.judge(c, "total", total, letter(ran), f"{ran['depths_per_block']} depths/block, table {'in LDS' if ran['table_in_lds'] else 'not in LDS'}", ran=ran)
    assert bits(total, b_total(ctx, c)), (c.name, ran)  # every route gives route B's bits
    return ran


def tiled_case(name):
    """by name (nothing is built while the tests are collected): only a `levels_<n_lev>_table_<n_table>` case may be untiled"""
    if not name.startswith("levels_"):
        return True
    _, n_lev, _, n_table = name.split("_")
    return T.tile_bytes(int(n_lev), int(n_table)) <= T.TILE_LDS_GATE


@pytest.mark.parametrize("name", T.FUSED_NAMES)
def test_fused_step_untiled_or_tiled(ctx, name):
    """routes C and D: which of them a case takes follows from its level count and its table"""
    c = T.case(name)
    assert tiled_case(name) == (T.tile_bytes(c.n_lev, c.n_table) <= T.TILE_LDS_GATE)
    ran = check_fused(ctx, c, plan=False, classify=False)
    assert letter(ran) == ("D" if tiled_case(name) else "C") and not ran["planned"]
    assert ran["table_in_lds"] == int(0 < c.n_table <= T.STAGE_MAX_NODES)


@pytest.mark.parametrize("name", [n for n in T.FUSED_NAMES if tiled_case(n)])
def test_fused_step_planned(ctx, name):
    """route E, up to the last level count the tiles take (the largest planned request of dynamic LDS)"""
    ran = check_fused(ctx, T.case(name), plan=True, classify=False)
    assert letter(ran) == "E" and ran["shmem"] == T.planned_bytes(T.case(name).n_lev) and not ran["table_in_lds"]


@pytest.mark.parametrize("name", [n for n in T.FUSED_NAMES if not tiled_case(n)])
def test_a_plan_is_declined_by_the_untiled_continuum(ctx, name):
    ran = check_fused(ctx, T.case(name), plan=True, classify=False)
    assert letter(ran) == "C"


@pytest.mark.parametrize("name", [n for n in T.FUSED_NAMES if tiled_case(n)])
def test_fused_step_riding_the_classification(ctx, name):
    """route F: 256-thread tiles, always eight depths per block whatever the depth count (7, 8, 9, 17 among the cases)"""
    c = T.case(name)
    ran = check_fused(ctx, c, plan=False, classify=True)
    assert letter(ran) == "F" and ran["depths_per_block"] == T.CONT_DEPTHS and ran["threads"] == T.BLOCK
    assert ran["rows"] == -(-c.n_depth // T.CONT_DEPTHS)


def test_the_cases_reach_every_route():
    """by the rule the fused tests hold the launches to: C with the table in LDS and without it, D likewise, E at the largest planned
    request, F with fewer than eight depths, a ragged last group and a ragged last tile; the level counts on both sides of both
    thresholds"""
    seen = set()
    for name in T.FUSED_NAMES:
        c = T.case(name)
        r = T.route_rule(256, c.n_depth, c.n_nu, c.n_nu, 4, c.n_lev, c.n_table)  # (none of what is collected here depends on the chip)
        seen.add((letter(r), r["table_in_lds"]))
        if r["tiled"]:
            seen.add(("E", 0))
            f = T.route_rule(256, c.n_depth, c.n_nu, c.n_nu + PREFIX, 4, c.n_lev, c.n_table, kernel="k_classify_continuum")
            seen.add(("F", c.n_depth % 8 != 0, c.n_depth < 8, c.n_nu % T.BLOCK != 0))
            assert f["depths_per_block"] == 8
    assert {("C", 0), ("C", 1), ("D", 0), ("D", 1), ("E", 0)} <= seen
    assert ("F", True, True, True) in seen and ("F", True, False, True) in seen and ("F", False, False, False) in seen
    a, b = T.largest_tiled_level_count(T.STAGE_MAX_NODES), T.largest_tiled_level_count(0)
    assert tiled_case(f"levels_{a}_table_1024") and not tiled_case(f"levels_{a + 1}_table_1024")
    assert tiled_case(f"levels_{b}_table_0") and not tiled_case(f"levels_{b + 1}_table_0") and not tiled_case("levels_4096_table_0")
    assert T.planned_bytes(b) == max(T.planned_bytes(T.case(n).n_lev) for n in T.FUSED_NAMES if tiled_case(n)) > T.TILE_LDS_GATE


@pytest.mark.parametrize("plan", [False, True], ids=["tiles", "planned"])
@pytest.mark.parametrize("n_depth,want", [(9, 1), (17, 3), (7, 8), (9, 8)])
def test_depths_per_block(ctx, n_depth, want, plan):
    """the pre-pass launch at one depth per block, at three with a ragged last group (17 = 5 x 3 + 2), and at eight with fewer than
    eight depths and with one more: grids sized from the rule at this device's compute-unit count, their last tile three points long"""
    n_cu = ctx.continuum_route()["n_cu"]
    n_nu, n_lines = T.shape_for_depths_per_block(n_cu, n_depth, want, plan=plan)
    c = T.benign_for_depths_per_block(n_nu, n_depth)
    ran = check_fused(ctx, c, plan=plan, classify=False, n_lines=n_lines)
    assert ran["depths_per_block"] == want and ran["rows"] == -(-n_depth // want) and ran["planned"] == int(plan)
    assert n_depth % want != 0 or want == 1
    assert ran["tiles"] * T.PRE_BLOCK > n_nu  # lanes of the last tile return behind the barrier


@pytest.mark.parametrize("plan,classify", [(False, False), (True, False), (False, True)], ids=["D", "E", "F"])
def test_columns_are_independent_in_the_fused_step(ctx, plan, classify):
    """the grid without its first 37 columns: every remaining column moves to another lane and another tile and keeps its bits — a lane
    that read a neighbour's table value, nu ** -3 or Rayleigh powers would not (the fused step wants a descending grid: a shift stands
    in for the permutation)"""
    for name in ("edge_on_grid", "table_nodes_1024", "table_nodes_1025", "file_planes_4"):
        c = T.case(name)
        part = c.take(slice(37, None), name + "_from_37")
        total, ran, rule = fused(ctx, part, plan=plan, classify=classify)
        assert ran == rule and letter(ran) == ("F" if classify else "E" if plan else "D")
        assert bits(total, b_total(ctx, c)[:, 37:]), (name, ran)
