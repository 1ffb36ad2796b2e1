"""The far field of the line kernels (line_far_body, context option "far_field"): (line, depth, tile) triples whose 256-point tile lies
wholly inside the line's window, clear of its core and at least three tile widths from its centre are summed at the tile's 16
Chebyshev nodes and carried to the grid points by the degree-15 interpolant.  It must agree with the direct sum far inside the
opacity tolerance (1e-12), keep the zeros of the reference, stay bit-identical under frequency sharding and work on grids whose
spacing jumps, whose length is no multiple of a tile, and with every kind of line list."""
import numpy as np
import pytest

import oracle
from conftest import rel_err
from stardis_amd import _lib, synth
from stardis_amd.engine import SpectralSynthesizer, shard_bounds

pytestmark = pytest.mark.gpu

FAR_VS_DIRECT = 2e-13  # measured <= 7e-15 on the 1e6-line list; the interpolation bound is 6e-18 of an item, the rest is rounding


@pytest.fixture
def far_ctx():
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def run(ctx, far, nus, atm, lines, cont, th, w, **kw):
    ctx.set_option("far_field", far)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, track_evaluations=False, **kw)
    syn.step()
    out = syn.alpha_line().copy(), syn.total_alphas().copy(), syn.F_nu().copy()
    # (the far field is a role of the line kernel's launch)
    launched = "far" in ctx.profile_variant("k_line_all")
    ctx.call("sdx_profile_enable", 0)
    syn.close()
    return out, launched


def workload(lam0, lam1, R, n_lines, seed, mix=(0.5, 0.3, 0.2), n_theta=4):
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(lam0, lam1, R=R)
    lines = synth.synth_lines(nus, atm, n_lines, seed=seed, mix=mix)
    th, w = synth.thetas_and_weights(n_theta)
    return atm, nus, lines, synth.synth_continuum_state(atm), th, w


_SPLIT_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from stardis_amd import _lib, synth
from stardis_amd.engine import SpectralSynthesizer
atm = synth.solar_atmosphere()
nus = synth.tracing_grid(4000.0, 4170.0, R=1.0e5)
lines = synth.synth_lines(nus, atm, 400, seed=5, mix=(0.5, 0.3, 0.2))  # (workload() below, seed 5)
th, w = synth.thetas_and_weights(4)
cont = synth.synth_continuum_state(atm)
assert 2 * 2048 < nus.size < 2 * 2048 + 256 and atm["temperatures"].size == 56  # just over two far units of 2048 points
shard = (700, nus.size - 730)  # begins inside the first unit, ends inside the third
ctx = _lib.Context(0)
for min_lines in (8192, 100):  # a short list (every line scanned) and the same list as a long one (hlist / wlist)
    ctx.set_option("indexed_min_lines", min_lines)
    out = []
    for far in (0, 1):
        ctx.set_option("far_field", far)
        ctx.call("sdx_profile_enable", 1)
        ctx.call("sdx_profile_reset")
        syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, track_evaluations=False, shard=shard)
        syn.step()
        out.append((syn.alpha_line().copy(), syn.F_nu().copy()))
        launches = [ctx.profile(k)[0] for k in ("k_line_all", "k_line_wide", "k_line_narrow", "k_line_far")]
        far_role = "far" in ctx.profile_variant("k_line_wide" if launches[1] else "k_line_all")
        ctx.call("sdx_profile_enable", 0)
        syn.close()
    assert not np.array_equal(out[0][0], out[1][0])  # lines wide enough for the far role
    print("LAUNCHES", min_lines, *launches, int(far_role))
    print("RESULT", min_lines, *(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in out[1]))
ctx.close()
"""


def test_split_launches_write_the_planes_of_the_single_launch():
    """SDX_SPLIT_LAUNCHES (profiling: the line kernel as two launches) keeps the far role in front of the first launch, with the line
    kernel's own subsets: a profiled run sums in the order of the run it profiles.  alpha_line and F_nu of a shard that begins and ends
    inside a far unit, short list and long, byte for byte; each run in a process of its own (the knob is read once)."""
    import os
    import subprocess
    import sys

    from conftest import ROOT

    def child(extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SDX_")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return [[ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith(tag)] for tag in ("RESULT", "LAUNCHES")]

    plain, plain_launches = child({})
    split, split_launches = child(dict(SDX_EXPERIMENT="1", SDX_SPLIT_LAUNCHES="1"))
    # (k_line_all, k_line_wide, k_line_narrow, k_line_far launches of the step, and whether the first carried the far role)
    for row in plain_launches:
        n_all, n_wide, n_narrow, n_far, far_role = (int(v) for v in row[1:])
        assert n_all >= 1 and n_wide == n_narrow == n_far == 0 and far_role, row
    for row in split_launches:
        n_all, n_wide, n_narrow, n_far, far_role = (int(v) for v in row[1:])
        assert n_all == 0 and n_wide == n_narrow >= 1 and n_far == 0 and far_role, row
    assert len(plain_launches) == len(split_launches) == 2
    assert len(plain) == 2 and [p[0] for p in plain] == ["8192", "100"]
    assert split == plain


@pytest.mark.parametrize("n_lines", [700, 9000])  # short lists are scanned completely; long ones go through hlist / wlist
def test_far_field_agrees_with_the_direct_sum_and_the_oracle(far_ctx, n_lines):
    atm, nus, lines, cont, th, w = workload(4000.0, 4300.0, 1.0e5, n_lines, seed=5)
    assert 4096 < nus.size < 32768  # below the automatic threshold: the option decides
    (line0, total0, F0), ran0 = run(far_ctx, 0, nus, atm, lines, cont, th, w)
    (line1, total1, F1), ran1 = run(far_ctx, 1, nus, atm, lines, cont, th, w)
    assert not ran0 and ran1
    assert not np.array_equal(line0, line1)  # (it is a different sum)
    assert np.array_equal(line0 == 0, line1 == 0)
    assert rel_err(line1, line0) < FAR_VS_DIRECT and rel_err(total1, total0) < FAR_VS_DIRECT
    assert rel_err(F1[1:], F0[1:]) < 1e-11
    ref = oracle.calc_alan_entries(56, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])
    assert np.array_equal(line1 == 0, ref == 0)
    assert rel_err(line1, ref) < 1e-12


def test_automatic_choice_follows_the_global_grid(far_ctx):
    """-1 (the default): grids of >= 32768 frequencies — decided from the GLOBAL grid, so a narrow shard of a long grid still runs it"""
    atm, nus, lines, cont, th, w = workload(4000.0, 4300.0, 1.0e5, 700, seed=6)
    _, ran = run(far_ctx, -1, nus, atm, lines, cont, th, w)
    assert not ran
    atm, nus, lines, cont, th, w = workload(4000.0, 5800.0, 1.0e5, 700, seed=6)
    assert nus.size >= 32768
    _, ran = run(far_ctx, -1, nus, atm, lines, cont, th, w)
    assert ran
    _, ran = run(far_ctx, -1, nus, atm, lines, cont, th, w, shard=(1000, 700))
    assert ran


@pytest.mark.parametrize("n_lines,world", [(700, 3), (9000, 5)])
def test_shards_reproduce_the_unsharded_far_field_bit_for_bit(far_ctx, n_lines, world):
    atm, nus, lines, cont, th, w = workload(4000.0, 5000.0, 1.0e5, n_lines, seed=7)
    (line, total, F), ran = run(far_ctx, 1, nus, atm, lines, cont, th, w)
    assert ran
    for rank in range(world):
        b, c = shard_bounds(nus.size, world, rank)
        (l, t, f), ran = run(far_ctx, 1, nus, atm, lines, cont, th, w, shard=(b, c))
        assert ran
        assert np.array_equal(l, line[:, b:b + c]) and np.array_equal(t, total[:, b:b + c]) and np.array_equal(f, F[:, b:b + c]), rank
    # ... and shards that begin and end inside a tile, one of them narrower than a tile
    for b, c in ((100, 300), (255, 2), (256 * 7 + 13, 256 * 3 + 1), (nus.size - 77, 77)):
        (l, t, f), _ = run(far_ctx, 1, nus, atm, lines, cont, th, w, shard=(b, c))
        assert np.array_equal(l, line[:, b:b + c]) and np.array_equal(f, F[:, b:b + c]), (b, c)


def test_grids_with_jumps_in_their_spacing_and_ragged_ends(far_ctx):
    """The distance test is made in index space from the tile's own end frequencies: segments of very different resolving power in
    one grid (tiles ten times wider than their neighbours), a grid a few points longer than a whole number of tiles, one shorter
    than a single tile."""
    atm = synth.solar_atmosphere()
    cont = synth.synth_continuum_state(atm)
    th, w = synth.thetas_and_weights(4)
    seg = [synth.tracing_grid(4000.0, 4100.0, R=3.0e5), synth.tracing_grid(4100.0, 4400.0, R=3.0e4)[1:], synth.tracing_grid(4400.0, 4450.0, R=6.0e5)[1:]]
    nus = np.concatenate(seg[::-1]) if seg[0][0] < seg[-1][0] else np.concatenate(seg)
    nus = np.sort(nus)[::-1].copy()
    assert np.all(np.diff(nus) < 0)
    for n in (nus.size, (nus.size // 256) * 256 + 3, 200):
        g = nus[:n].copy()
        lines = synth.synth_lines(g, atm, 600, seed=8, mix=(0.4, 0.3, 0.3))
        (line0, _, F0), _ = run(far_ctx, 0, g, atm, lines, cont, th, w)
        (line1, _, F1), ran = run(far_ctx, 1, g, atm, lines, cont, th, w)
        assert ran
        assert np.array_equal(line0 == 0, line1 == 0)
        assert rel_err(line1, line0) < FAR_VS_DIRECT, n
        assert rel_err(F1[1:], F0[1:]) < 1e-11, n
        if n == 200: assert np.array_equal(line0, line1)  # no full tile: no far field, the third plane is zeros


def test_mixed_precision_keeps_its_tolerance_with_the_far_field(far_ctx):
    atm, nus, lines, cont, th, w = workload(4000.0, 4300.0, 1.0e5, 9000, seed=9)
    (line64, _, F64), _ = run(far_ctx, 0, nus, atm, lines, cont, th, w)
    far_ctx.set_option("mixed_precision", 1)
    try:
        (line0, _, F0), _ = run(far_ctx, 0, nus, atm, lines, cont, th, w)
        (line1, _, F1), ran = run(far_ctx, 1, nus, atm, lines, cont, th, w)
    finally:
        far_ctx.set_option("mixed_precision", 0)
    assert ran
    assert rel_err(F0[1:], F64[1:]) < 1e-4 and rel_err(F1[1:], F64[1:]) < 1e-4
    # (the far items are evaluated in fp64 at the nodes: the tolerance path gets no further from the fp64 sum)
    assert rel_err(line0, line64) < 5e-5 and rel_err(line1, line64) < 5e-5


def test_a_column_of_gammas_and_a_deep_model(far_ctx):
    """gamma as an (N_l, 1) column (the molecular lists), and a model with more depth points than a wave has lanes"""
    atm, nus, lines, cont, th, w = workload(5000.0, 5300.0, 1.0e5, 12000, seed=10)
    lines["gammas"] = np.ascontiguousarray(lines["gammas"][:, :1])
    (line0, _, F0), _ = run(far_ctx, 0, nus, atm, lines, cont, th, w)
    (line1, _, F1), ran = run(far_ctx, 1, nus, atm, lines, cont, th, w)
    assert ran and rel_err(line1, line0) < FAR_VS_DIRECT and rel_err(F1[1:], F0[1:]) < 1e-11
    from test_gpu_engine import deep_atmosphere

    atm = deep_atmosphere(150)
    lines = synth.synth_lines(nus, atm, 500, seed=11, mix=(0.5, 0.3, 0.2))
    cont = synth.synth_continuum_state(atm)
    (line0, _, F0), _ = run(far_ctx, 0, nus, atm, lines, cont, th, w)
    (line1, _, F1), ran = run(far_ctx, 1, nus, atm, lines, cont, th, w)
    assert ran and line1.shape[0] == 150 and rel_err(line1, line0) < FAR_VS_DIRECT and rel_err(F1[1:], F0[1:]) < 1e-11


def test_the_stand_alone_line_opacity_entry_point_takes_the_option_too(far_ctx):
    """sdx_line_opacity_f64 (host buffers; what the mirror's calc_alan_entries calls): three partial planes reduced instead of two,
    the evaluation count — the reference's window sizes, whoever evaluates them — unchanged"""
    from stardis_amd import ops

    atm, nus, lines, cont, th, w = workload(4200.0, 4500.0, 1.0e5, 900, seed=12)
    args = (56, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])
    far_ctx.set_option("far_field", 0)
    a0, n0 = ops.calc_alan_entries(*args, return_evaluations=True, ctx=far_ctx)
    far_ctx.set_option("far_field", 1)
    a1, n1 = ops.calc_alan_entries(*args, return_evaluations=True, ctx=far_ctx)
    assert n0 == n1 and not np.array_equal(a0, a1)
    assert np.array_equal(a0 == 0, a1 == 0) and rel_err(a1, a0) < FAR_VS_DIRECT
    ref, evals = oracle.calc_alan_entries(*args, return_evals=True)
    assert n1 == evals and rel_err(a1, ref) < 1e-12


def test_a_step_that_fails_after_asking_for_far_ranges_leaves_nothing_behind(far_ctx):
    """The far ranges a step wants travel with its pre-pass request, not in the context: a synthesis refused inside the pre-pass — behind
    the request, where the continuum tiles are sized: bound-free species with a level count outside 1..4096 — leaves the context as it
    found it.  A synthesis, a stand-alone line opacity and the line windows on that context equal a fresh context's, byte for byte.
    Eight depths, eight 256-point tiles, 300 lines, four angles: no launch of such a step has the grid spacing to compute (the pre-pass
    blocks scan it), so the ranges come from k_far_ranges — once per synthesis, once per stand-alone line opacity."""
    from stardis_amd import ops
    from test_gpu_engine import deep_atmosphere

    atm = deep_atmosphere(8)
    nus = synth.tracing_grid(4000.0, 4000.0 * np.exp(2048 / 1.0e5), n_override=2048)  # (the spacing of R = 1e5)
    lines = synth.synth_lines(nus, atm, 300, seed=13, mix=(0.5, 0.3, 0.2))
    cont = synth.synth_continuum_state(atm)
    th, w = synth.thetas_and_weights(4)
    args = (8, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])

    def everything(ctx):
        planes, ran = run(ctx, 1, nus, atm, lines, cont, th, w)
        assert ran and ctx.profile("k_far_ranges")[0] == 1
        ctx.call("sdx_profile_enable", 1)
        alan = ops.calc_alan_entries(*args, ctx=ctx)
        assert ctx.profile("k_far_ranges")[0] == 2
        ctx.call("sdx_profile_enable", 0)
        return (*planes, alan, *ops.line_windows(*args, ctx=ctx))

    fresh = _lib.Context(0)
    try:
        want = everything(fresh)
    finally:
        fresh.close()
    far_ctx.set_option("far_field", 1)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=far_ctx, track_evaluations=False)
    syn.cont.bf_n_levels = 5000
    try:
        with pytest.raises(ValueError, match=r"synthesize: bf_n_levels must be set \(1\.\.4096\)"):  # (the pre-pass's own refusal)
            syn.step()
    finally:
        syn.close()
    got = everything(far_ctx)
    assert len(got) == len(want) == 6
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
