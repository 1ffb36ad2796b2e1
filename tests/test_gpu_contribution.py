"""Flux contribution function and formation mean on the device (sdx_contribution_dev, sdx_contribution_f64, sdx_formation_mean_dev,
SpectralSynthesizer(keep_contribution=True)).

Measured on MI355X (gfx950), maxima over the compared columns, in units of F_nu[-1] of the column:
  |C_gpu - C_g15| (g15: the reference's own traced intensities on the g7 inputs), N_theta 1 / 4 / 20     8.5e-13 / 8.3e-13 / 4.1e-13   (1e-10)
  |sum_k C - F_nu[-1]| on the device's own numbers, g7 size, N_theta 1 / 4 / 20                         1.2e-15 / 5.1e-16 / 3.7e-16   (1e-12)
  the same at full S-c2, F_nu from k_raytrace<1> / k_raytrace_seg<8,7>                                  5.0e-16 / 4.9e-16             (1e-12)
  full S-c2 against the numpy restatement fed the device's total_alphas                                 1.2e-12                       (1e-10)
  source plane from sdx_blackbody_dev against the in-kernel Planck function                             1.0e-15                       (1e-10)
  formation mean of log10(1 .. N_d) against g15, N_theta 1 / 4 / 20                                     3.7e-13 / 3.7e-13 / 2.1e-13   (9.8e-9)
  300 depths x 5 angles (3 of 12 frequencies per wave fit LDS): sum identity / against the restatement  1.5e-15 / 3.4e-13             (1e-12 / 1e-10)
Every test prints its figure before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import contribution_reference as cref
from conftest import load_golden
from stardis_amd import ops, synth
from stardis_amd.engine import SpectralSynthesizer, shard_bounds

pytestmark = pytest.mark.gpu

FLUX_TOL = 1e-10   # the project's flux tolerance: C is a decomposition of the flux
SUM_TOL = 1e-12    # the project's tolerance for reordered sums
STAGES = ("k_raytrace", "k_prepass_continuum", "k_line_prepass", "k_line_all", "k_reduce_partials", "k_total_alphas", "k_dnu_partial", "k_line_far", "k_classify", "k_hlist",
          "k_far_ranges", "k_scale", "k_accumulate")  # profile names of the step's launches


def g7_inputs(n_theta):
    g7 = load_golden("g7_raytrace")
    ray = np.ascontiguousarray(g7["dist"].reshape(-1, 1) / np.cos(g7[f"thetas_{n_theta}"]))
    return g7, ray, np.ascontiguousarray(g7[f"weights_{n_theta}"])


def against_g15(C_gpu, n_theta, label, columns=None):
    g7, g15 = load_golden("g7_raytrace"), load_golden("g15_contribution")
    F, C_ref = g7[f"F_nu_{n_theta}"][-1], g15[f"C_{n_theta}"]
    ok = np.isfinite(F)
    assert np.flatnonzero(~ok).tolist() == [11]  # column 11 (the reference's own flux is NaN) is the only one not compared
    if columns is not None:
        ok &= columns
    err = np.abs(C_gpu[:, ok] - C_ref[:, ok]) / np.where(F[ok] == 0, 1.0, F[ok])
    print(f"{label} N_theta={n_theta}: max |C_gpu - C_ref| / F_ref[-1] = {err.max():.3e}")
    assert np.all(np.abs(C_gpu[:, ok] - C_ref[:, ok]) <= FLUX_TOL * F[ok])
    return err.max()


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_contribution_dev_against_golden(ctx, n_theta):
    g7, ray, w = g7_inputs(n_theta)
    C_gpu = ops.contribution_arrays(g7["nus"], g7["temperatures"], ray, w, g7["total_alphas"], ctx=ctx)
    against_g15(C_gpu, n_theta, "sdx_contribution_dev")
    assert not C_gpu[:, 7].any()  # opacity 0 at every depth: exactly 0
    assert not C_gpu[0].any()     # nothing lies below row 0


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_contribution_f64_against_golden(ctx, n_theta):
    g7, ray, w = g7_inputs(n_theta)
    nus, t, total = (np.ascontiguousarray(g7[k], dtype=np.float64) for k in ("nus", "temperatures", "total_alphas"))
    out = np.full(total.shape, np.nan)
    p = lambda a: a.ctypes.data  # noqa: E731
    ctx.call("sdx_contribution_f64", t.size, nus.size, n_theta, p(nus), p(t), p(ray), p(w), p(total), None, p(out))
    against_g15(out, n_theta, "sdx_contribution_f64")
    assert not out[:, 7].any()
    assert np.array_equal(out, ops.contribution_arrays(nus, t, ray, w, total, ctx=ctx), equal_nan=True)  # the twin: same kernel, same bits


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_engine_against_golden(ctx, n_theta):
    """The engine forms its own total_alphas from the inputs g7 was made from (continuum state, 60 lines); columns 7 and 11 of g7 were
    overwritten by hand afterwards, which the engine cannot be given: it is compared on the other 198."""
    g7 = load_golden("g7_raytrace")
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(6560.0, 6570.0, step=0.05)
    assert np.array_equal(nus, g7["nus"])
    lines = synth.synth_lines(nus, atm, 60, seed=21, mix=(0.7, 0.2, 0.1))
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], g7[f"thetas_{n_theta}"], g7[f"weights_{n_theta}"], lines,
                              synth.synth_continuum_state(atm), ctx=ctx, keep_contribution=True)
    syn.step()
    ctx.synchronize()
    own = np.ones(nus.size, bool)
    own[[7, 11]] = False
    against_g15(syn.contribution.numpy(), n_theta, "engine", columns=own)
    syn.close()


def sum_identity(Cg, F_last, label):
    nan = ~np.isfinite(F_last)
    assert np.array_equal(np.isnan(Cg).any(axis=0), nan)  # a column is undefined in C exactly where the flux is
    ok = ~nan
    s = Cg[:, ok].sum(axis=0)
    zero = F_last[ok] == 0
    assert not s[zero].any()
    err = np.abs(s[~zero] - F_last[ok][~zero]) / F_last[ok][~zero]
    print(f"{label}: max |sum_k C - F_nu[-1]| / F_nu[-1] = {err.max():.3e} over {err.size} columns")
    assert err.max() <= SUM_TOL
    return err.max()


@pytest.mark.parametrize("seg", [0, 1], ids=["k_raytrace", "segmented"])
@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_sum_identity_g7_size(ctx, seg, n_theta):
    g7, ray, w = g7_inputs(n_theta)
    ctx.set_option("segmented_raytrace", seg)
    try:
        F, _ = ops.raytrace_arrays(g7["nus"], g7["temperatures"], ray, w, g7["total_alphas"], ctx=ctx)
    finally:
        ctx.set_option("segmented_raytrace", -1)
    Cg = ops.contribution_arrays(g7["nus"], g7["temperatures"], ray, w, g7["total_alphas"], ctx=ctx)
    sum_identity(Cg, F[-1], f"g7 size, N_theta={n_theta}, segmented_raytrace={seg}")


@pytest.fixture(scope="module")
def sc2():
    return synth.make_workload("S-c2")


def run(ctx, w, **kw):
    atm = w["atm"]
    syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx, **kw)
    syn.step()
    ctx.synchronize()
    return syn


@pytest.mark.parametrize("seg", [0, 1], ids=["k_raytrace", "segmented"])
def test_sum_identity_full_sc2(ctx, sc2, seg):
    assert sc2["nus"].size == 7634 and sc2["atm"]["temperatures"].size == 56 and sc2["thetas"].size == 20
    ctx.set_option("segmented_raytrace", seg)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        syn = run(ctx, sc2, keep_contribution=True)
        variant = ctx.profile_variant("k_raytrace")
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
    assert variant == ("k_raytrace_seg<8,7>" if seg else "k_raytrace<1>")
    sum_identity(syn.contribution.numpy(), syn.F_nu()[-1], f"S-c2, {variant}")
    syn.close()


def test_full_sc2_against_the_restatement(ctx, sc2):
    syn = run(ctx, sc2, keep_contribution=True)
    atm = sc2["atm"]
    ray = atm["dist"].reshape(-1, 1) / np.cos(sc2["thetas"])
    C_ref = cref.contribution_function(sc2["nus"], atm["temperatures"], ray, sc2["weights"], syn.total_alphas())
    F_ref = C_ref.sum(axis=0)
    Cg = syn.contribution.numpy()
    assert np.isfinite(F_ref).all() and (F_ref > 0).all()
    err = np.abs(Cg - C_ref) / F_ref
    print(f"S-c2 against the numpy restatement: max |C_gpu - C_ref| / F_ref[-1] = {err.max():.3e}")
    assert np.all(np.abs(Cg - C_ref) <= FLUX_TOL * F_ref)
    syn.close()


@pytest.mark.parametrize("world", [2, 8])
def test_shards_concatenate_bit_for_bit(ctx, sc2, world):
    whole = run(ctx, sc2, keep_contribution=True)
    Cw = whole.contribution.numpy()
    whole.close()
    parts = []
    for r in range(world):
        syn = run(ctx, sc2, shard=shard_bounds(sc2["nus"].size, world, r), keep_contribution=True)
        parts.append(np.array(syn.contribution.numpy()))
        syn.close()
    assert np.array_equal(np.concatenate(parts, axis=1), Cw)


def test_graph_replay_equals_eager(ctx, sc2):
    atm = sc2["atm"]
    syn = SpectralSynthesizer(sc2["nus"], atm["temperatures"], atm["dist"], sc2["thetas"], sc2["weights"], sc2["lines"], sc2["cont"], ctx=ctx,
                              keep_contribution=True, track_evaluations=False)
    syn.step()
    ctx.synchronize()
    eager, F = np.array(syn.contribution.numpy()), np.array(syn.F_nu())
    syn.contribution.zero()
    syn.capture(batch=2)
    syn.contribution.zero()
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.contribution.numpy(), eager) and np.array_equal(syn.F_nu(), F)
    syn.contribution.zero()
    assert syn.step_batch() == 2
    ctx.synchronize()
    assert np.array_equal(syn.contribution.numpy(), eager)
    syn.close()


def test_source_plane_from_blackbody(ctx):
    g7, ray, w = g7_inputs(4)
    nus, t = g7["nus"], g7["temperatures"]
    planck_run = ops.contribution_arrays(nus, t, ray, w, g7["total_alphas"], ctx=ctx)
    d_nus, d_t = ctx.upload(nus), ctx.upload(t)
    d_S = ctx.empty((t.size, nus.size))
    ctx.call("sdx_blackbody_dev", t.size, nus.size, d_nus.ptr, d_t.ptr, d_S.ptr, nus.size)
    with_plane = ops.contribution_arrays(nus, t, ray, w, g7["total_alphas"], ctx=ctx, source=d_S.numpy())
    F = g7["F_nu_4"][-1]
    ok = np.isfinite(F) & (F != 0)
    err = np.abs(with_plane[:, ok] - planck_run[:, ok]) / F[ok]
    print(f"source plane from sdx_blackbody_dev against the in-kernel Planck function: {err.max():.3e} of F_nu[-1]")
    assert err.max() <= FLUX_TOL
    assert not with_plane[:, 7].any()


@pytest.mark.parametrize("seg", [0, 1], ids=["k_raytrace", "segmented"])
def test_flag_leaves_the_step_alone(ctx, sc2, seg):
    """keep_contribution off and on: F_nu, total_alphas, alpha_line and the continuum flux bit-identical; off: no k_contribution launch."""
    ctx.set_option("segmented_raytrace", seg)
    ctx.call("sdx_profile_enable", 1)
    try:
        ctx.call("sdx_profile_reset")
        off = run(ctx, sc2, keep_continuum_flux=True)
        assert ctx.profile("k_contribution")[0] == 0
        launches_off = {k: ctx.profile(k)[0] for k in STAGES}
        ctx.call("sdx_profile_reset")
        on = run(ctx, sc2, keep_continuum_flux=True, keep_contribution=True)
        assert ctx.profile("k_contribution")[0] == 1
        assert {k: ctx.profile(k)[0] for k in launches_off} == launches_off
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
    assert np.array_equal(on.F_nu(), off.F_nu())
    assert np.array_equal(on.total_alphas(), off.total_alphas())
    assert np.array_equal(on.alpha_line(), off.alpha_line())
    assert np.array_equal(on.F_nu_continuum, off.F_nu_continuum)
    with pytest.raises(RuntimeError, match="keep_contribution"):
        off.contribution
    off.close(), on.close()


def test_formation_mean_bit_for_bit_and_against_golden(ctx):
    g15 = load_golden("g15_contribution")
    x_log, n_depth = g15["x_log10"], g15["x_log10"].size
    for n_theta in (1, 4, 20):
        g7, ray, w = g7_inputs(n_theta)
        d_C = ops.contribution_arrays(g7["nus"], g7["temperatures"], ray, w, g7["total_alphas"], ctx=ctx, device=True)
        Cg = d_C.numpy()
        for x in (x_log, g7["temperatures"]):
            got = ops.formation_mean(d_C, x, ctx=ctx)
            assert np.array_equal(got, cref.formation_mean(Cg, x), equal_nan=True)  # the numpy loop of the definition, bit for bit
        got, ref = ops.formation_mean(d_C, x_log, ctx=ctx), g15[f"mean_log10_{n_theta}"]
        assert np.isnan(got[7]) and np.isnan(ref[7])  # 0 / 0 on both sides
        ok = np.isfinite(g7[f"F_nu_{n_theta}"][-1])
        ok[7] = False
        assert ok.sum() == 198
        err = np.abs(got[ok] - ref[ok]).max()
        bound = n_depth * FLUX_TOL * (x_log.max() - x_log.min())
        print(f"formation mean of log10(1..N_d), N_theta={n_theta}: max |gpu - golden| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def test_engine_formation_mean(ctx, sc2):
    syn = run(ctx, sc2, keep_contribution=True)
    t = sc2["atm"]["temperatures"]
    host = syn.formation_mean(t).numpy()
    assert np.array_equal(host, cref.formation_mean(syn.contribution.numpy(), t), equal_nan=True)
    assert np.array_equal(syn.formation_mean(ctx.upload(t)).numpy(), host)
    assert (host >= t.min()).all() and (host <= t.max()).all()
    with pytest.raises(ValueError):
        syn.formation_mean(t[:-1])
    syn.close()


def refused(ctx, match, *args):
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        with pytest.raises(ValueError, match=match):
            ctx.call("sdx_contribution_dev", *args)
        assert ctx.lib.sdx_last_error_code() == -1  # SDX_ERR_ARG
        assert ctx.profile("k_contribution")[0] == 0  # nothing was launched
    finally:
        ctx.call("sdx_profile_enable", 0)


def test_refusals_before_any_launch(ctx, sc2):
    g7, ray, w = g7_inputs(4)
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (g7["nus"], g7["temperatures"], ray, w, g7["total_alphas"])]
    n_nu, n_depth = g7["nus"].size, g7["temperatures"].size
    d_C = ctx.empty((n_depth, n_nu))
    good = (n_depth, n_nu, 4, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, n_nu, None, 0, d_C.ptr, n_nu)
    ctx.call("sdx_contribution_dev", *good)
    ctx.synchronize()
    before = np.array(d_C.numpy())

    # more than 64 angles (the pointers are never read: the refusal comes first)
    refused(ctx, "64 angles", *((n_depth, n_nu, 65) + good[3:]))
    # a model too deep for 64 KB of LDS at one frequency per wave: 4 waves x (2 N_d + 4) doubles > 64 KB from N_d = 1023 on
    refused(ctx, "models this deep", *((1100, n_nu, 1) + good[3:]))
    # a mixed-precision context, through the C entry point and at the construction of an engine
    atm = sc2["atm"]
    ctx.set_option("mixed_precision", 1)
    try:
        refused(ctx, "mixed_precision", *good)
        with pytest.raises(ValueError, match="mixed_precision"):
            SpectralSynthesizer(sc2["nus"], atm["temperatures"], atm["dist"], sc2["thetas"], sc2["weights"], sc2["lines"], sc2["cont"], ctx=ctx,
                                keep_contribution=True)
    finally:
        ctx.set_option("mixed_precision", 0)
    th, wt = synth.thetas_and_weights(65)
    with pytest.raises(ValueError, match="64 angles"):
        SpectralSynthesizer(sc2["nus"], atm["temperatures"], atm["dist"], th, wt, sc2["lines"], sc2["cont"], ctx=ctx, keep_contribution=True)
    # bad leading dimension / null output
    refused(ctx, "leading dimension", *(good[:8] + (n_nu - 1,) + good[9:]))
    refused(ctx, "null pointer", *(good[:11] + (None, n_nu)))
    out = C.c_double()
    with pytest.raises(ValueError, match="formation_mean"):
        ctx.call("sdx_formation_mean_dev", n_depth, n_nu, None, n_nu, d[1].ptr, C.addressof(out))
    # the context is still usable, and computes what it computed before
    d_C.zero()
    ctx.call("sdx_contribution_dev", *good)
    ctx.synchronize()
    assert np.array_equal(d_C.numpy(), before, equal_nan=True)


def deep_model(ctx, n_depth, n_theta):
    """the g7 columns resampled to n_depth points: the sum identity against k_raytrace<1>'s flux, and the numpy restatement"""
    g7 = load_golden("g7_raytrace")
    pos = np.linspace(0.0, g7["temperatures"].size - 1.0, n_depth)
    rows = np.arange(g7["temperatures"].size, dtype=np.float64)
    cols = np.ones(g7["nus"].size, bool)
    cols[[7, 11]] = False  # (the two columns g7 zeroed by hand have no logarithm to interpolate)
    nus = np.ascontiguousarray(g7["nus"][cols])
    temps = np.interp(pos, rows, g7["temperatures"])
    total = np.ascontiguousarray(np.exp(np.stack([np.interp(pos, rows, np.log(col)) for col in g7["total_alphas"][:, cols].T], axis=1)))
    dist = np.interp(0.5 * (pos[1:] + pos[:-1]), rows[:-1] + 0.5, g7["dist"]) * (rows.size - 1.0) / (n_depth - 1.0)
    th, w = synth.thetas_and_weights(n_theta)
    ray = np.ascontiguousarray(dist.reshape(-1, 1) / np.cos(th))
    Cg = ops.contribution_arrays(nus, temps, ray, w, total, ctx=ctx)
    ctx.set_option("segmented_raytrace", 0)
    try:
        F, _ = ops.raytrace_arrays(nus, temps, ray, w, total, ctx=ctx)
    finally:
        ctx.set_option("segmented_raytrace", -1)
    sum_identity(Cg, F[-1], f"{n_depth} depths x {n_theta} angles")
    C_ref = cref.contribution_function(nus, temps, ray, w, total)
    F_ref = C_ref.sum(axis=0)
    err = np.abs(Cg - C_ref) / F_ref
    print(f"{n_depth} depths x {n_theta} angles against the numpy restatement: max |C_gpu - C_ref| / F_ref[-1] = {err.max():.3e}")
    assert np.all(np.abs(Cg - C_ref) <= FLUX_TOL * F_ref)


def test_deep_model_with_lowered_groups_per_wave(ctx):
    """300 depths x 5 angles: the staged columns of 12 frequencies per wave would not fit 64 KB of LDS, so the launch lowers the
    frequencies per wave to 3 (idle lanes), as k_raytrace<1> does: same sum identity, same agreement with the restatement."""
    deep_model(ctx, 300, 5)


@pytest.mark.parametrize("n_depth", [301, 302])
def test_deep_model_either_side_of_a_lowered_group(ctx, n_depth):
    """20 angles: the last depth at which 3 frequencies per wave fit LDS and the first at which the launch lowers them to 2 — where a
    launch sized by another layout than the kernel's first shows."""
    deep_model(ctx, n_depth, 20)
