"""The grid plan (sdx_grid_plan, include/stardis_hip.h): what the pre-pass launch forms from the frequency grid, the line frequencies
and the tabulated cross-section alone — grid spacing, line centres, lines per centre index, the per-frequency continuum values — is
formed once per synthesizer and read by planned kernels (k_prepass_continuum<false, LINES, true>) instead of being formed in every
step.  The plan holds the step's own values, so every output must be the same BIT FOR BIT with and without it, in every mode of
use; nothing that changes from step to step may have moved into it; and a plan that does not belong to the call is refused."""
import ctypes as C

import numpy as np
import pytest

from stardis_amd import _lib, constants as K, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

PLANNED = "planned"  # the variant the profile records of the pre-pass launch carry when the planned kernel ran
STAGE = "k_prepass_continuum"


@pytest.fixture
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def outputs(syn):
    return syn.F_nu().copy(), syn.total_alphas().copy(), syn.alpha_line().copy(), int(syn.evaluations())


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def run(ctx, plan, nus, atm, lines, cont, th, w, prepare=None, graph=False, **kw):
    """one step (eager and profiled, or two replays of a recorded graph) -> outputs, whether the planned kernel ran"""
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, grid_plan=plan, **kw)
    keep = prepare(syn) if prepare else None  # (device arrays the description points at)
    if graph:
        syn.capture()
        syn.step()
        syn.step()
        planned = syn.plan is not None
    else:
        ctx.call("sdx_profile_enable", 1)
        ctx.call("sdx_profile_reset")
        syn.step()
        planned = PLANNED in ctx.profile_variant(STAGE)
        ctx.call("sdx_profile_enable", 0)
        ctx.call("sdx_profile_reset")
    out = outputs(syn)
    syn.close()
    del keep
    return out, planned


def both_ways(ctx, nus, atm, lines, cont, th, w, expect_planned=True, **kw):
    off, p0 = run(ctx, False, nus, atm, lines, cont, th, w, **kw)
    on, p1 = run(ctx, True, nus, atm, lines, cont, th, w, **kw)
    assert not p0 and p1 == expect_planned
    assert np.all(np.isfinite(off[0]))
    assert same(on, off)
    return off


def problem(n_nu, n_lines, seed, lam=(6540.0, 6580.0), mix=(0.7, 0.2, 0.1), n_theta=4, atm=None):
    atm = atm or synth.solar_atmosphere()
    nus = synth.tracing_grid(lam[0], lam[1], R=1.0, n_override=n_nu)
    lines = synth.synth_lines(nus, atm, n_lines, seed=seed, mix=mix)
    th, w = synth.thetas_and_weights(n_theta)
    return nus, atm, lines, synth.synth_continuum_state(atm), th, w


@pytest.mark.parametrize("n_lines", [300, 2000])
def test_odd_grid_short_and_listed(ctx, n_lines):
    """2051 points (no multiple of a tile or a block); 2000 lines: the wide-line list and its ticket run in a planned block"""
    ctx.set_option("wide_list", 1)
    nus, atm, lines, cont, th, w = problem(2051, n_lines, seed=5 + n_lines)
    off = both_ways(ctx, nus, atm, lines, cont, th, w)
    assert off[3] > 0


def test_seven_points(ctx):
    both_ways(ctx, *problem(7, 20, seed=3))


@pytest.mark.parametrize("n_lines", [0, 1])
def test_empty_and_single_line(ctx, n_lines):
    both_ways(ctx, *problem(900, n_lines, seed=11), expect_planned=n_lines > 0)


def test_lines_beyond_both_ends_of_the_grid(ctx):
    nus, atm, lines, cont, th, w = problem(1500, 200, seed=17)
    ln = lines["line_nus"].copy()
    span = nus.max() - nus.min()
    ln[:5] = nus.min() - span * np.array([0.5, 0.1, 0.01, 1e-4, 1e-9])
    ln[-5:] = nus.max() + span * np.array([1e-9, 1e-4, 0.01, 0.1, 0.5])
    lines = dict(lines, line_nus=ln, alphas=lines["alphas"] * 50.0)  # (strong enough that windows from outside reach the grid)
    assert np.all(np.diff(ln) >= 0)
    both_ways(ctx, nus, atm, lines, cont, th, w)


@pytest.mark.parametrize("n_depth", [65, 129])
def test_two_and_three_depth_blocks(ctx, n_depth):
    """several depth blocks per line: the atomicMax path of nhw_max / whw_max"""
    from test_gpu_engine import deep_atmosphere

    both_ways(ctx, *problem(1300, 260, seed=n_depth, atm=deep_atmosphere(n_depth)))


@pytest.mark.parametrize("n_nu", [16384, 16385])
def test_the_switch_away_from_the_in_block_spacing_scan(ctx, n_nu):
    both_ways(ctx, *problem(n_nu, 300, seed=n_nu, lam=(6400.0, 6700.0)))


def test_far_field_grid(ctx):
    """32 768 points and a few strong lines: the far field is on, the grid-spacing launch stays for its tile ranges"""
    nus, atm, lines, cont, th, w = problem(32768, 120, seed=23, lam=(5000.0, 7000.0), mix=(0.5, 0.3, 0.2))
    assert ctx.lib.sdx_far_field_active(ctx.handle, nus.size) == 1
    both_ways(ctx, nus, atm, lines, cont, th, w)


def test_odd_offset_shard_against_the_whole_grid(ctx):
    nus, atm, lines, cont, th, w = problem(3001, 400, seed=29)
    whole, _ = run(ctx, False, nus, atm, lines, cont, th, w)
    begin, count = 777, 1001
    shard = both_ways(ctx, nus, atm, lines, cont, th, w, shard=(begin, count))
    for a, b in zip(shard[:3], whole[:3]):
        assert np.array_equal(a, b[:, begin:begin + count])
    assert shard[3] == whole[3]


def test_mixed_precision(ctx):
    ctx.set_option("mixed_precision", 1)
    both_ways(ctx, *problem(2051, 500, seed=31))


def test_rayleigh_and_three_species_in_interleaved_level_order(ctx):
    """the plan's Rayleigh powers, and bound-free edges read from LDS with levels of three species interleaved (the G14 shape)"""
    nus, atm, lines, cont, th, w = problem(1777, 300, seed=37, lam=(3400.0, 3800.0))  # (the Balmer edge lies on the grid)

    def prepare(syn):
        c, s = syn.ctx, syn.cont
        n_lev = cont["level_density"].shape[0]
        order = np.array([0, 3, 6, 9, 1, 4, 7, 2, 5, 8])[:n_lev]  # species A: levels 0 3 6 9, B: 1 4 7, C: 2 5 8
        cutoff = ((cont["ionization_energy"] - np.asarray(cont["level_excitation"])) / K.H_CGS)[order]
        keep = [c.upload(np.array([0, 4, 7, 10], dtype=np.int32), np.int32), c.upload(np.array([0, 0, 1], dtype=np.int32), np.int32),
                c.upload(cutoff), c.upload(np.ascontiguousarray(cont["level_density"][order])),
                c.upload(cont["n_h1"]), c.upload(cont["n_he1"])]
        s.bf_n_species, s.bf_n_levels = 3, n_lev
        s.bf_species_offsets, s.bf_species_ion_number, s.bf_cutoff, s.bf_level_density = (k.ptr for k in keep[:4])
        s.ray_n_h, s.ray_n_he, s.rayleigh_enabled = keep[4].ptr, keep[5].ptr, 1
        return keep

    both_ways(ctx, nus, atm, lines, cont, th, w, prepare=prepare)


def test_line_list_as_scalars_steps_without_a_plan(ctx):
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(6540.0, 6580.0, R=1.0, n_override=2051)
    ll = synth.synth_linelist(nus, atm, 300, seed=41, mix=(0.7, 0.2, 0.1))
    th, w = synth.thetas_and_weights(4)
    both_ways(ctx, nus, atm, ll, synth.synth_continuum_state(atm), th, w, expect_planned=False)


def test_captured_graph_against_eager_steps(ctx):
    nus, atm, lines, cont, th, w = problem(2051, 600, seed=43)
    eager, _ = run(ctx, False, nus, atm, lines, cont, th, w)
    replay, planned = run(ctx, True, nus, atm, lines, cont, th, w, graph=True)
    assert planned and same(replay, eager)


def test_nothing_that_changes_per_step_was_hoisted(ctx):
    """a live plan, every per-step input overwritten in place: the step equals a fresh plan-less synthesizer on the new inputs.  Then
    the grid and the line frequencies themselves are overwritten and the plan refreshed."""
    nus, atm, lines, cont, th, w = problem(2051, 500, seed=47)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx)
    assert syn.plan is not None
    syn.step()
    first = outputs(syn)

    def fresh(nus_, atm_, lines_, cont_):
        ref = SpectralSynthesizer(nus_, atm_["temperatures"], atm_["dist"], th, w, lines_, cont_, ctx=ctx, grid_plan=False)
        ref.step()
        out = outputs(ref)
        ref.close()
        return out

    def overwrite(atm_, lines_, cont_):
        syn.d_a.set(lines_["alphas"]), syn.d_dw.set(lines_["doppler_widths"]), syn.d_g.set(lines_["gammas"])
        syn.d_t.set(atm_["temperatures"])
        # (engine._build_continuum's uploads, in its order: 3 table density, 7 level densities, 9 free-free densities, 10 electrons)
        syn._keep[3].set(cont_["n_hminus"]), syn._keep[7].set(cont_["level_density"])
        syn._keep[9].set(np.asarray(cont_["n_e"]) * np.asarray(cont_["n_h2"])), syn._keep[10].set(cont_["n_e"])

    assert same(first, fresh(nus, atm, lines, cont))
    atm2 = dict(atm, temperatures=atm["temperatures"] * 1.07, n_e=atm["n_e"] * 1.9, n_h=atm["n_h"] * 0.8)
    cont2 = synth.synth_continuum_state(atm2)
    lines2 = dict(synth.synth_lines(nus, atm2, 500, seed=48, mix=(0.6, 0.3, 0.1)), line_nus=lines["line_nus"])
    overwrite(atm2, lines2, cont2)
    syn.step()
    second = outputs(syn)
    assert not same(second, first)
    assert same(second, fresh(nus, atm2, lines2, cont2))
    # another grid and other line frequencies of the same sizes, in place; the plan follows by refresh_grid_plan()
    nus3 = synth.tracing_grid(5100.0, 5190.0, R=1.0, n_override=nus.size)
    lines3 = synth.synth_lines(nus3, atm2, 500, seed=49, mix=(0.6, 0.3, 0.1))
    syn.d_nus.set(nus3), syn._keep[0].set(K.nu_to_angstrom(nus3)), syn.d_ln.set(lines3["line_nus"])
    overwrite(atm2, lines3, cont2)
    syn.refresh_grid_plan()
    syn.step()
    third = outputs(syn)
    assert not same(third, second)
    assert same(third, fresh(nus3, atm2, lines3, cont2))
    syn.close()


def test_a_plan_that_does_not_belong_to_the_call_is_refused(ctx):
    nus, atm, lines, cont, th, w = problem(900, 100, seed=53)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx)
    other_nus, other_ln, other_table = ctx.upload(nus), ctx.upload(lines["line_nus"]), ctx.upload(cont["hminus_bf_cross_section"])
    ctx.synchronize()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    opt = _lib.SynthesisOptions()
    opt.grid_plan = syn.plan

    def call(n_nu=None, d_nus=None, n_lines=None, d_ln=None, cont_=None):
        return ctx.lib.sdx_synthesize_opt_dev(
            ctx.handle, syn.n_depth, syn.n_nu if n_nu is None else n_nu, d_nus or syn.d_nus.ptr, 0, syn.count if n_nu is None else n_nu,
            syn.n_lines if n_lines is None else n_lines, d_ln or syn.d_ln.ptr, syn.d_dw.ptr, syn.d_g.ptr, syn.gamma_cols, syn.d_a.ptr,
            C.byref(cont_ or syn.cont), syn.n_theta, syn.d_t.ptr, syn.d_ray.ptr, syn.d_w.ptr, syn.d_line.ptr, syn.d_total.ptr, syn.flux_ptr,
            syn.count, C.byref(opt), None)

    moved_table = _lib.Continuum.from_buffer_copy(syn.cont)
    moved_table.table_sigma = other_table.ptr
    for kw in (dict(d_nus=other_nus.ptr), dict(n_nu=syn.n_nu - 1), dict(d_ln=other_ln.ptr), dict(n_lines=syn.n_lines - 1), dict(cont_=moved_table)):
        assert call(**kw) == -1, kw
        assert "grid plan" in ctx.lib.sdx_last_error_string().decode()
    ctx.synchronize()
    for stage in (STAGE, "k_line_all", "k_raytrace", "k_dnu_partial"):
        assert ctx.profile(stage)[0] == 0, stage  # nothing was launched
    assert call() == 0  # (the call it was built for)
    ctx.synchronize()
    assert ctx.profile(STAGE)[0] == 1 and PLANNED in ctx.profile_variant(STAGE)
    ctx.call("sdx_profile_enable", 0)
    ctx.call("sdx_profile_reset")
    syn.close()
