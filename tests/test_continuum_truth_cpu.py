"""What tests/test_gpu_continuum_truth.py rests on, checked without a GPU: the fp64 oracle alone meets the criterion on every hostile
plasma (within n_ops 2^-53 of the 80-bit truth at every point, the same zeros, NaNs and infinities), every class holds what it
claims, and the routing rule restated in tests/continuum_truth.py is the one in the host code.

The planned launch at the last level count the tiles take (762 without a staged table) asks for (8 (762 + 6) + 762) 8 = 55 248 bytes of
dynamic LDS, more than the 48 KiB plan_continuum's gate compares the UNPLANNED tile with.  Settled by reading: it is sound.  The gate is
not the launch limit — a workgroup of this chip may take far more than 64 KiB — but what keeps two 1024-thread blocks on a compute
unit's 160 KiB (tests/test_kernel_resources_cpu.py::test_prepass_blocks_fit_two_per_cu: 80 KiB each, static and dynamic together).  The
unplanned worst case is 49 152 + 28 552 bytes of static LDS (k_prepass_continuum<true, 32>) = 77 704; the planned kernels hold 17 416
bytes of static LDS at most, so their worst case is 55 248 + 17 416 = 72 664: below 80 KiB as well, and the request itself below
64 KiB.  The gate stays as it is; test_planned_request_stays_sound holds the request, tests/test_grid_plan_resources_cpu.py adds the
compiler's static figure to it, and the GPU test runs the launch (levels_762_table_0, planned)."""
import os
import re

import numpy as np
import pytest

import continuum_truth as T
from conftest import ROOT

pytestmark = pytest.mark.skipif(not T.EXTENDED, reason="numpy.longdouble is not an extended type here")

ALL = T.NAMES + ("clipped_in_place",)


@pytest.mark.parametrize("name", T.NAMES)
def test_oracle_alone_meets_the_criterion(name):
    c = T.case(name)
    ref = c.reference()
    for src in T.SOURCES:
        t, o = ref["truth"][src], ref["oracle"][src]
        assert (t is None) == (o is None) == (ref["n_ops"][src] is None or src == "total" and t is None)
        if t is None:
            continue
        assert o.shape == (c.n_depth, c.n_nu) == t.shape
        assert T.same_special_values(o, t), (name, src)
        d = ref["oracle_distance"][src]
        print(f"{name:28s} {src:9s} oracle {d:.3e} of {ref['n_ops'][src]} x 2^-53 = {ref['n_ops'][src] * T.U:.3e}")
        assert d <= ref["n_ops"][src] * T.U, (name, src, d, ref["n_ops"][src])
    special = ~np.isfinite(ref["truth"]["total"])
    assert special.any() == (name == "densities_overflow"), name  # only that case leaves the fp64 range


def test_no_value_is_subnormal_or_near_the_end_of_the_range():
    """a relative bound holds neither for a subnormal result nor where the rounding decides between a finite value and infinity"""
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    for c in T.hostile_plasmas():
        for src, t in c.reference()["truth"].items():
            if t is None:
                continue
            v = np.abs(t[np.isfinite(t) & (t != 0)])
            assert v.size == 0 or (v.min() >= tiny and v.max() <= 0.5 * huge), (c.name, src)


def test_tables_never_more_than_halve():
    for c in T.hostile_plasmas():
        if c.xp is not None:
            assert np.all(c.fp > 0) and np.all(c.fp[1:] >= 0.5 * c.fp[:-1]), c.name


def test_grids_are_exact_and_descending():
    for c in T.hostile_plasmas(ALL):
        assert np.all(np.diff(c.nus) < 0) or c.n_nu == 1, c.name
        k = c.nus / 2.0 ** 14
        regular = k == np.round(k)
        assert np.count_nonzero(~regular) <= 2, c.name  # (the two fp64 neighbours of 2.3e15 Hz)


def test_edge_classes_hold_what_they_claim():
    c = T.case("edge_on_grid")
    pts = c.notes["points"]
    assert pts[0] == 0 and pts[-1] == c.n_nu - 1 and 0 < pts[1] < c.n_nu - 1
    for p in pts:
        v = c.nus[p]
        assert np.count_nonzero(c.cutoff == v) == 1 and np.count_nonzero(c.cutoff == np.nextafter(v, np.inf)) == 1
        assert np.count_nonzero(c.cutoff == np.nextafter(v, -np.inf)) == 1
        assert c.col_cls[p] == "edge_on_grid"
    on = c.nus[None, :] >= c.cutoff[:, None]
    # never on: far above the grid, and an ulp above its first point; always on: far below it, and an ulp below its last point
    assert np.count_nonzero(~on.any(axis=1)) == 2 and np.count_nonzero(on.all(axis=1)) == 3 and np.count_nonzero(c.cutoff == c.nus[-1]) == 1
    sp = T.species_of_levels(c.offs)
    assert sorted(set(sp[np.isin(c.cutoff, [c.nus[p] for p in pts])])) == [0, 1]  # the edges on grid points lie in both species
    a, b = T.case("edge_above_grid"), T.case("edge_below_grid")
    assert np.all(a.cutoff > a.nus[0]) and a.cutoff.min() == np.nextafter(a.nus[0], np.inf)
    assert np.all(a.reference()["truth"]["bf"] == 0)
    assert np.all(b.cutoff < b.nus[-1]) and b.cutoff.max() == np.nextafter(b.nus[-1], -np.inf)
    assert np.all(b.reference()["truth"]["bf"] > 0)


@pytest.mark.parametrize("n_table", T.TABLE_NODES)
def test_table_classes_hold_what_they_claim(n_table):
    c = T.case(f"table_nodes_{n_table}")
    assert c.xp.size == n_table and (n_table <= T.STAGE_MAX_NODES) == (n_table != 1025)
    _, kind = T.interp_truth(c.lambdas, c.xp, c.fp)
    lam, xp, cls = c.lambdas, c.xp, c.col_cls
    assert np.count_nonzero(lam == xp[0]) >= 1 and np.count_nonzero(lam == xp[-1]) >= 1
    assert np.count_nonzero(lam < xp[0]) >= 2 and np.count_nonzero(lam > xp[-1]) >= 2
    for v in (np.nextafter(xp[0], np.inf), np.nextafter(xp[-1], -np.inf), np.nextafter(xp[0], -np.inf), np.nextafter(xp[-1], np.inf)):
        assert np.count_nonzero(lam == v) == 1
    on_node = np.isin(lam, xp)
    assert np.array_equal(on_node, (cls == "on_node") | (cls == "table_end"))
    assert np.count_nonzero(cls == "on_node") >= (0 if n_table == 2 else 3)
    assert np.array_equal(kind == 2, (cls == "on_node"))  # np.interp's own "x == xp[j]" branch; the ends are the clamps
    assert np.array_equal((kind == 0) | (kind == 1), (cls == "table_end") | (cls == "beyond_table"))
    beside = np.isin(lam, np.nextafter(xp[1:-1], np.inf)) | np.isin(lam, np.nextafter(xp[1:-1], -np.inf))
    assert np.array_equal(beside & (cls != "ulp_inside_end"), cls == "ulp_beside_node")


def test_rayleigh_classes_hold_what_they_claim():
    seen = set()
    for c in T.hostile_plasmas([n for n in T.NAMES if n.startswith("rayleigh_cut_")]):
        seen.add((c.n_h is not None, c.n_he is not None, c.n_h2 is not None))
        i = int(np.flatnonzero(c.nus == T.RAYLEIGH_CUT)[0])
        assert c.col_cls[i] == "at_cut" and c.nus[i - 1] == np.nextafter(T.RAYLEIGH_CUT, np.inf) and c.nus[i + 1] == np.nextafter(T.RAYLEIGH_CUT, 0.0)
        assert c.col_cls[i - 1] == "ulp_above_cut" and np.all(c.col_cls[:i - 1] == "far_above_cut") and i - 1 >= 10
        ray = c.reference()["truth"]["rayleigh"]
        assert np.all(ray[:, :i] == 0)  # clipped: exactly zero
        assert np.all(ray[:, i:] > 0) == any(seen_k for seen_k in (c.n_h is not None, c.n_he is not None, c.n_h2 is not None))
    assert len(seen) == 8


def test_species_level_and_density_classes_hold_what_they_claim():
    c = T.case("species_three_interleaved")
    assert c.n_species == 3 and np.any(np.diff(c.cutoff) < 0)  # plasma order is not frequency order
    c = T.case("species_empty_species")
    assert list(np.flatnonzero(np.diff(c.offs) == 0)) == [0, 2, 4]
    assert sorted(set(T.case("species_ions_0_1_2").bf_ions)) == [0, 1, 2]
    c = T.case("species_ff_only_ion_zero")
    assert np.all(c.reference()["truth"]["ff"] == 0) and np.all(c.ff_density > 0)
    c = T.case("species_none")
    assert c.n_species == 0 and c.reference()["truth"]["bf"] is None and c.reference()["truth"]["ff"] is None
    a, b = T.largest_tiled_level_count(T.STAGE_MAX_NODES), T.largest_tiled_level_count(0)
    assert sorted((cc.n_lev, cc.n_table) for cc in T.hostile_plasmas([n for n in T.NAMES if n.startswith("levels_")])) == sorted(
        [(1, 1024), (10, 1024), (a, 1024), (a + 1, 1024), (b, 0), (b + 1, 0), (4096, 0)])
    for cc in T.hostile_plasmas([n for n in T.NAMES if n.startswith("levels_")]):
        assert np.count_nonzero(np.isin(cc.cutoff, cc.nus)) >= 1 and cc.n_species == 3 and cc.offs[-1] == cc.n_lev
    c = T.case("densities_zero_rows")
    tot = c.reference()["truth"]["total"]
    assert [d for d in range(c.n_depth) if np.all(tot[d] == 0)] == [0, 3, 7] and np.all(c.reference()["truth"]["bf"][5] == 0)
    c = T.case("densities_subnormal")
    tiny = np.finfo(np.float64).tiny
    for arr in (c.level_density, c.ff_density, c.n_h2, c.n_he):
        assert np.any((arr > 0) & (arr < tiny))
    c = T.case("densities_overflow")
    r = c.reference()
    assert np.all(np.isposinf(r["truth"]["ff"][4])) and np.all(np.isfinite(r["truth"]["ff"][[0, 1, 2, 3, 5, 6, 7]]))
    with np.errstate(all="ignore"):
        terms = c.ff_density[:, 4] / np.sqrt(c.temps[4]) * T.FF_CONSTANT
        assert np.all(np.isfinite(terms)) and np.isinf(terms.sum())  # finite terms, an infinite sum
    assert np.any(np.isposinf(r["truth"]["bf"][1])) and np.any(np.isfinite(r["truth"]["bf"][1])) and np.all(np.isposinf(r["truth"]["bf"][2]) | (r["truth"]["bf"][2] == 0))
    assert np.all(np.isfinite(r["truth"]["electron"]))
    assert len(T.case("file_planes_0").planes) == 0 and len(T.case("file_planes_4").planes) == 4
    assert sorted(set(T.CLASSES) - {"clipped_in_place"}) == sorted({cc.cls for cc in T.hostile_plasmas()})


def test_clipped_in_place_pattern_is_the_oracles():
    """bound-free and free-free on the array calc_alpha_rayleigh has clipped: infinite or NaN exactly where the oracle is"""
    import oracle

    c = T.case("clipped_in_place")
    clipped = np.array(c.nus)
    oracle.alpha_rayleigh(clipped, c.n_h, c.n_he, c.n_h2)
    assert np.count_nonzero(clipped == 0) == 61 and np.all(clipped[61:] == c.nus[61:])
    again = T.Case("clipped_in_place", "clipped", c.nus, c.n_depth, 0)
    for k in ("offs", "bf_ions", "cutoff", "level_density", "ff_ions", "ff_density", "temps"):
        setattr(again, k, getattr(c, k))
    again.nus = clipped
    t = T.truth(again)
    with np.errstate(all="ignore"):
        bf = oracle.alpha_bf(clipped, c.offs, c.bf_ions, c.cutoff, c.level_density)
        ff = oracle.alpha_ff(clipped, c.temps, c.ff_ions, c.ff_density)
    assert T.same_special_values(bf, t["bf"]) and T.same_special_values(ff, t["ff"])
    assert np.all(np.isposinf(ff[:, :61])) and np.all(np.isnan(bf[:, :61]) | np.isposinf(bf[:, :61])) and np.isnan(bf[:, :61]).any()


def source_text():
    with open(os.path.join(ROOT, "stardis_amd", "csrc", "stardis_hip.hip")) as f:
        host = f.read()
    with open(os.path.join(ROOT, "stardis_amd", "csrc", "sdx_kernels.h")) as f:
        return host, f.read()


def test_restated_rule_is_the_one_in_the_host_code():
    """the lines of plan_continuum and of the planned launch that tests/continuum_truth.py restates, held to the source text"""
    host, kernels = source_text()
    squeeze = lambda s: re.sub(r"\s+", " ", s)  # noqa: E731
    host = squeeze(host)
    for line in (
        "p->stage_table = ca.table_sigma && ca.n_table > 0 && ca.n_table <= 1024;",
        "p->shmem = std::max<size_t>(8, (n_lev + (p->stage_table ? 2 * (size_t)ca.n_table : 0)) * sizeof(double));",
        "p->cont_tiles = (int)((g.nu_count + (int64_t)threads * kContPoints - 1) / ((int64_t)threads * kContPoints));",
        "const size_t tile_shmem = ((size_t)kContDepths * (n_lev + 6) + (p->stage_table ? 2 * (size_t)ca.n_table : 0)) * sizeof(double);",
        "if (tile_shmem <= 48 * 1024) {",
        "int dgs = (int)std::max<int64_t>(1, std::min<int64_t>(kContDepths, ((int64_t)p->cont_tiles * threads / kPreBlock * n_depth) / (2 * (int64_t)ctx->n_cu)));",
        "const int64_t slots = std::max<int64_t>(1, 2 * (int64_t)ctx->n_cu - other_blocks * ((n_depth + kPreDepths - 1) / kPreDepths));",
        "const int64_t fit = ((int64_t)p->cont_tiles * n_depth + slots - 1) / slots;",
        "dgs = (int)std::max<int64_t>(dgs, std::min<int64_t>(kContDepths, fit));",
        "if (threads == kBlock) dgs = kContDepths;",
        "p->cont_rows = (unsigned)((n_depth + dgs - 1) / dgs);",
        "planned_cp.shmem = ((size_t)kContDepths * (n_lev + 6) + n_lev) * sizeof(double);",
        "s.pre_lines = ((n_lines + 15) / 16) * ((n_depth + kPreDepths - 1) / kPreDepths) <= 2 * (int64_t)ctx->n_cu ? 16 : 32;",
        "if ((rc = plan_continuum(ctx, req.cont, g, kPreBlock, s.n_line_blocks, &planned_cp))) return rc;",
        "else if (int rc = plan_continuum(ctx, cont, g, kPreBlock, (int64_t)n_line_blocks + s.n_pixel_blocks, &cp)) return rc;",
        "s.n_pixel_blocks = (int)((n_nu + 2 + kPreBlock - 1) / kPreBlock);",
        "if (int rc = plan_continuum(ctx, cont, g, kBlock, 0, &cp)) return rc;",
        "int64_t indexed_min_lines = 8192;",
    ):
        assert squeeze(line) in host, line
    for name, value in (("kContDepths", T.CONT_DEPTHS), ("kPreBlock", T.PRE_BLOCK), ("kBlock", T.BLOCK), ("kPreDepths", T.PRE_DEPTHS), ("kContPoints", 1)):
        assert re.search(rf"constexpr int {name} = {value};", kernels), name
    assert T.TILE_LDS_GATE == 48 * 1024 and T.STAGE_MAX_NODES == 1024


def test_thresholds_follow_from_the_rule():
    for n_table in (0, 37, 1024, 1025, 5000):
        n = T.largest_tiled_level_count(n_table)
        assert T.tile_bytes(n, n_table) <= T.TILE_LDS_GATE < T.tile_bytes(n + 1, n_table)
        assert T.route_rule(256, 9, 257, 257, 4, n, n_table)["tiled"] == 1 and T.route_rule(256, 9, 257, 257, 4, n + 1, n_table)["tiled"] == 0
    assert T.largest_tiled_level_count(1025) == T.largest_tiled_level_count(0) > T.largest_tiled_level_count(1024) > 0


def fused_launch_shapes():
    """(n_lev, n_table) of every case the GPU tests put through a fused step"""
    return sorted({(c.n_lev, c.n_table) for c in T.hostile_plasmas(T.FUSED_NAMES)} | {(3, 37)})


def test_every_request_of_the_gpu_tests_stays_within_the_launch_limit():
    shapes = fused_launch_shapes()
    assert len(shapes) >= 10
    for n_lev, n_table in shapes:
        for kernel in ("k_prepass_continuum", "k_classify_continuum"):
            for plan in (False, True):
                r = T.route_rule(256, 9, 1025, 1025, 4, n_lev, n_table, kernel=kernel, plan=plan)
                want = (T.planned_bytes(n_lev) if r["planned"] else T.tile_bytes(n_lev, n_table)) if r["tiled"] else T.untiled_bytes(n_lev, n_table)
                assert r["shmem"] == want and 8 <= r["shmem"] <= T.LDS_LIMIT, (n_lev, n_table, kernel, plan, r)
                assert r["planned"] == int(plan and r["tiled"] and kernel == "k_prepass_continuum")


def test_planned_request_stays_sound():
    """the largest planned request (the static LDS beside it is the compiler's figure: tests/test_grid_plan_resources_cpu.py::
    test_the_largest_planned_request_still_fits_two_blocks_per_cu adds the two and holds the sum to 80 KiB)"""
    n = T.largest_tiled_level_count(0)
    assert n == 762 and T.planned_bytes(n) == 55248 > T.TILE_LDS_GATE and T.planned_bytes(n) <= T.LDS_LIMIT
    assert T.planned_bytes(n + 1) > T.planned_bytes(n)  # (and n + 1 is never planned: untiled)
    assert T.route_rule(256, 9, 1025, 1025, 4, n + 1, 0, plan=True)["planned"] == 0
    assert T.planned_bytes(T.largest_tiled_level_count(T.STAGE_MAX_NODES)) < T.planned_bytes(n)  # a staged table only lowers the level count


def test_depths_per_block_shapes_exist_for_any_chip():
    for n_cu in (64, 104, 228, 256, 304):
        n_nu, n_lines = T.shape_for_depths_per_block(n_cu, 9, 1)
        assert T.route_rule(n_cu, 9, n_nu, n_nu, n_lines, 3, 37)["depths_per_block"] == 1
        for n_depth, want in ((17, 3), (17, 5), (7, 8), (9, 8)):
            for plan in (False, True):
                n_nu, n_lines = T.shape_for_depths_per_block(n_cu, n_depth, want, plan=plan)
                r = T.route_rule(n_cu, n_depth, n_nu, n_nu, n_lines, 3, 37, plan=plan)
                assert r["depths_per_block"] == want and r["tiles"] * n_depth <= 4000 and n_nu % T.PRE_BLOCK in (3, 1023), (n_cu, n_depth, want, r)
                assert r["rows"] == -(-n_depth // want)
