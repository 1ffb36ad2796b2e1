"""Short line lists (fewer than "indexed_min_lines" lines): the last line block of the pre-pass launch lists the lines that have a
wide window (half-width > 64 grid points) at any depth, one list per line subset of the wide role, and the wide role of the line
kernel walks that list instead of testing every line of the list against its tile (context option "wide_list").  The list holds
the lines a subset would have met as possible hits, in the order in which it would have met them: every output must be the same
BIT FOR BIT with the option on and off, in every mode of use.  The fp32-mixed mode keeps the full scan (its fp32 partial sums are
flushed at chunk boundaries, which a compacted list would move), so it is identical by construction; the case stays here to hold
that."""
import numpy as np
import pytest

from stardis_amd import _lib, linelist as LL, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

BUILT = "wide-line list"  # the variant the profile records of the pre-pass launch carry when the list is built


@pytest.fixture
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def wide_lines(nus, lines, ctx=None):
    """number of lines with a wide window (half-width > 64 points, not empty) at any depth: the window rule of parallel.window_work"""
    if isinstance(lines, LL.LineList):
        a, g, dw = LL.line_params(lines, ctx)
        ln = np.asarray(lines.nu, dtype=np.float64)
    else:
        a, g, dw, ln = lines["alphas"], lines["gammas"], lines["doppler_widths"], lines["line_nus"]
    nus = np.asarray(nus, dtype=np.float64)
    n = nus.size
    d_nu = -np.max(np.diff(nus))
    centre = n - np.searchsorted(nus[::-1], np.asarray(ln, dtype=np.float64))
    g = np.asarray(g, dtype=np.float64).reshape(centre.size, -1)
    pixels = (g + np.asarray(dw, dtype=np.float64)) * np.asarray(a, dtype=np.float64) / d_nu * 20.0
    hw = np.minimum(np.where(pixels > 10.0, pixels, 10.0), float(n)).astype(np.int64)
    lo = np.clip(centre[:, None] - hw, 0, n)
    hi = np.clip(centre[:, None] + hw, 0, n)
    return int(np.count_nonzero(np.any((hw > 64) & (hi > lo), axis=1)))


def outputs(syn):
    return syn.F_nu().copy(), syn.total_alphas().copy(), syn.alpha_line().copy(), int(syn.evaluations())


def run(ctx, wide_list, nus, atm, lines, cont, th, w, **kw):
    """one eager step -> (F_nu, total_alphas, alpha_line, evaluations), whether the pre-pass built the list, the launches per kernel"""
    ctx.set_option("wide_list", wide_list)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, **kw)
    syn.step()
    out = outputs(syn)
    built = BUILT in ctx.profile_variant("k_prepass_continuum")
    launches = {k: ctx.profile(k)[0] for k in ("k_prepass_continuum", "k_line_all", "k_hlist", "k_raytrace")}
    ctx.call("sdx_profile_enable", 0)
    ctx.call("sdx_profile_reset")
    syn.close()
    return out, built, launches


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def both_ways(ctx, nus, atm, lines, cont, th, w, expect_built=True, expect_auto=None, **kw):
    off, built0, _ = run(ctx, 0, nus, atm, lines, cont, th, w, **kw)
    on, built1, _ = run(ctx, 1, nus, atm, lines, cont, th, w, **kw)
    auto, built2, _ = run(ctx, -1, nus, atm, lines, cont, th, w, **kw)
    assert not built0 and built1 == expect_built
    assert expect_auto is None or built2 == expect_auto  # (-1: the library's own rule, from 16 chunks of 64 lines per subset on)
    assert off[3] > 0 and np.all(np.isfinite(off[0]))
    assert same(on, off) and same(auto, off)
    return off


def small(n_lines, seed, lam=(6540.0, 6580.0), R=3.0e5, mix=(0.90, 0.09, 0.01), n_theta=4):
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(lam[0], lam[1], R=R)
    lines = synth.synth_lines(nus, atm, n_lines, seed=seed, mix=mix)
    th, w = synth.thetas_and_weights(n_theta)
    return atm, nus, lines, synth.synth_continuum_state(atm), th, w


@pytest.mark.parametrize("tag,n_wide,auto", [("S-c2", 141, True), ("S-c1", 149, False)])
def test_benchmark_workloads(ctx, tag, n_wide, auto):
    wl = synth.make_workload(tag)  # (bench.py's build_workload: the same grid, list, seed and angles)
    assert wide_lines(wl["nus"], wl["lines"]) == n_wide and 0 < n_wide < wl["lines"]["line_nus"].size
    both_ways(ctx, wl["nus"], wl["atm"], wl["lines"], wl["cont"], wl["thetas"], wl["weights"], expect_auto=auto)


@pytest.mark.parametrize("n_lines", [63, 64, 65, 2000, 8191])
def test_random_short_lists(ctx, n_lines):
    atm, nus, lines, cont, th, w = small(n_lines, seed=100 + n_lines, mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < n_lines
    both_ways(ctx, nus, atm, lines, cont, th, w)


@pytest.mark.parametrize("n_lines", [65, 2000])
def test_line_list_inputs(ctx, n_lines):
    """per-line scalars: the generating pre-pass builds the list too"""
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(6540.0, 6580.0, R=3.0e5)
    ll = synth.synth_linelist(nus, atm, n_lines, seed=7 + n_lines, mix=(0.7, 0.2, 0.1))
    th, w = synth.thetas_and_weights(4)
    assert 0 < wide_lines(nus, ll, ctx) < n_lines
    both_ways(ctx, nus, atm, ll, synth.synth_continuum_state(atm), th, w)


def test_no_wide_line_and_every_line_wide(ctx):
    atm, nus, lines, cont, th, w = small(700, seed=21)
    d_nu = -np.max(np.diff(nus))
    pixels = ((lines["gammas"] + lines["doppler_widths"]) * lines["alphas"] / d_nu * 20.0).max(axis=1)
    none = dict(lines, alphas=lines["alphas"] * (32.0 / pixels.max()))
    assert wide_lines(nus, none) == 0
    both_ways(ctx, nus, atm, none, cont, th, w)
    every = dict(lines, alphas=lines["alphas"] * (200.0 / pixels.min()))
    assert wide_lines(nus, every) == 700
    both_ways(ctx, nus, atm, every, cont, th, w)


def test_a_deep_model_has_several_depth_blocks_per_line(ctx):
    from test_gpu_engine import deep_atmosphere

    atm = deep_atmosphere(150)
    nus = synth.tracing_grid(6540.0, 6580.0, R=3.0e5)
    lines = synth.synth_lines(nus, atm, 900, seed=33, mix=(0.7, 0.2, 0.1))
    th, w = synth.thetas_and_weights(4)
    assert 0 < wide_lines(nus, lines) < 900
    off = both_ways(ctx, nus, atm, lines, synth.synth_continuum_state(atm), th, w)
    assert off[2].shape[0] == 150


def test_mixed_precision(ctx):
    atm, nus, lines, cont, th, w = small(2000, seed=44, mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < 2000
    ctx.set_option("mixed_precision", 1)
    try:
        both_ways(ctx, nus, atm, lines, cont, th, w, expect_built=False)  # (the tolerance path keeps the full scan: module docstring)
    finally:
        ctx.set_option("mixed_precision", 0)


def test_unequal_frequency_shards_reproduce_the_whole_grid(ctx):
    atm, nus, lines, cont, th, w = small(2000, seed=55, mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < 2000
    whole = both_ways(ctx, nus, atm, lines, cont, th, w)
    cut = nus.size // 3 + 17  # (inside a tile)
    for b, c in ((0, cut), (cut, nus.size - cut)):
        part = both_ways(ctx, nus, atm, lines, cont, th, w, shard=(b, c))
        assert all(np.array_equal(p, f[:, b:b + c]) for p, f in zip(part[:3], whole[:3])), (b, c)


def test_the_far_field_kernels_walk_the_list_too(ctx):
    atm, nus, lines, cont, th, w = small(1500, seed=66, lam=(6400.0, 6700.0), mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < 1500
    ctx.set_option("far_field", 1)
    try:
        both_ways(ctx, nus, atm, lines, cont, th, w)
    finally:
        ctx.set_option("far_field", -1)


@pytest.mark.parametrize("batch", [1, 4])
def test_graph_replays_count_their_blocks_from_zero_every_step(ctx, batch):
    """the counter of finished line blocks is set back by the block that builds the list: 50+ consecutive replays (single steps, and
    graphs of four steps), the first and the last step equal to each other and to the eager step without the list"""
    atm, nus, lines, cont, th, w = small(2000, seed=77, mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < 2000
    off, _, _ = run(ctx, 0, nus, atm, lines, cont, th, w)
    ctx.set_option("wide_list", 1)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx)
    syn.capture(batch=batch)
    steps = 0
    syn.step_batch() if batch > 1 else syn.step()
    first = outputs(syn)
    while steps < 52:
        steps += syn.step_batch() if batch > 1 else (syn.step() or 1)
    last = outputs(syn)
    syn.close()
    assert same(first, off) and same(last, off)


def test_two_contexts_stepped_alternately():
    a, b = _lib.Context(0), _lib.Context(0)
    try:
        wa, wb = small(2000, seed=88, mix=(0.7, 0.2, 0.1)), small(1100, seed=89, lam=(6500.0, 6530.0), mix=(0.7, 0.2, 0.1))
        assert 0 < wide_lines(wa[1], wa[2]) < 2000 and 0 < wide_lines(wb[1], wb[2]) < 1100
        ref = []
        for c, (atm, nus, lines, cont, th, w) in ((a, wa), (b, wb)):
            ref.append(run(c, 0, nus, atm, lines, cont, th, w)[0])
            c.set_option("wide_list", 1)
        syns = [SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=c) for c, (atm, nus, lines, cont, th, w) in ((a, wa), (b, wb))]
        for _ in range(10):
            for s in syns:
                s.step()
        for s, r in zip(syns, ref):
            assert same(outputs(s), r)
            s.close()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n_lines", [8192, 20000])
def test_long_lists_are_not_touched(ctx, n_lines):
    """from "indexed_min_lines" lines on the list launches find the wide lines: the option changes neither the launches nor a bit"""
    atm, nus, lines, cont, th, w = small(n_lines, seed=99, lam=(6400.0, 6700.0))
    assert 0 < wide_lines(nus, lines) < n_lines
    off, built0, launches0 = run(ctx, 0, nus, atm, lines, cont, th, w)
    on, built1, launches1 = run(ctx, 1, nus, atm, lines, cont, th, w)
    assert not built0 and not built1
    assert launches0 == launches1 and launches0["k_hlist"] > 0
    assert same(on, off)


def test_the_line_opacity_entry_point_builds_the_list_too(ctx):
    """sdx_line_opacity_f64 runs the line pre-pass alone (k_line_prepass): the same list, the same bits, the same evaluation count"""
    from stardis_amd import ops

    atm, nus, lines, cont, th, w = small(1200, seed=111, mix=(0.7, 0.2, 0.1))
    assert 0 < wide_lines(nus, lines) < 1200
    args = (56, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])
    got = []
    for mode in (0, 1):
        ctx.set_option("wide_list", mode)
        ctx.call("sdx_profile_enable", 1)
        ctx.call("sdx_profile_reset")
        got.append(ops.calc_alan_entries(*args, return_evaluations=True, ctx=ctx))
        assert (BUILT in ctx.profile_variant("k_line_prepass")) == bool(mode)
        ctx.call("sdx_profile_enable", 0)
    assert got[0][1] == got[1][1] and np.array_equal(got[0][0], got[1][0])
