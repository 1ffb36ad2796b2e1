"""k_raytrace_seg_step, the segmented formal solution in the shape the fused synthesis step launches (a fused total of 0, 2 or 3 line
planes, the Planck source, flux only; context option "segmented_raytrace" = 2, and the default wherever the segmented kernel is
chosen): the same bits as the general kernel k_raytrace_seg<8,7> ("segmented_raytrace" = 1) in F_nu, total_alphas and the continuum
flux, the launch label of each mode, and the general kernel for every shape outside the rule."""
import numpy as np
import pytest

from stardis_amd import _lib, synth
from stardis_amd.engine import SpectralSynthesizer, shard_bounds

pytestmark = pytest.mark.gpu

GENERAL, STEP = "k_raytrace_seg<8,7>", "k_raytrace_seg_step<8,7>"


def no_lines(n_depth):
    return dict(line_nus=np.zeros(0), doppler_widths=np.zeros((0, n_depth)), gammas=np.zeros((0, n_depth)), alphas=np.zeros((0, n_depth)))


def case(atm, nus, n_lines, n_theta=20, seed=3):
    nd = atm["temperatures"].size
    lines = synth.synth_lines(nus, atm, n_lines, seed=seed) if n_lines else no_lines(nd)
    th, w = synth.thetas_and_weights(n_theta)
    return nus, atm["temperatures"], atm["dist"], th, w, lines, synth.synth_continuum_state(atm)


def from_workload(w):
    return w["nus"], w["atm"]["temperatures"], w["atm"]["dist"], w["thetas"], w["weights"], w["lines"], w["cont"]


def shallow(atm, n):
    """the first n depth points of an atmosphere"""
    out = dict(atm)
    for k in ("temperatures", "r", "n_e", "n_h"):
        out[k] = np.ascontiguousarray(atm[k][:n])
    out["dist"] = np.ascontiguousarray(atm["dist"][:n - 1])
    return out


def run(ctx, mode, args, **kw):
    """one step under segmented_raytrace = mode -> (outputs, launch label)"""
    kw.setdefault("keep_line", False)
    kw.setdefault("track_evaluations", False)
    ctx.set_option("segmented_raytrace", mode)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        syn = SpectralSynthesizer(*args, ctx=ctx, **kw)
        syn.step()
        ctx.synchronize()
        label = ctx.profile_variant("k_raytrace")
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
    out = {"F": syn.F_nu().copy()}
    if syn.keep_total:
        out["total"] = syn.total_alphas().copy()
    if syn.keep_continuum_flux:
        out["Fc"] = syn.F_nu_continuum.copy()
    syn.close()
    return out, label


def same_bits(ctx, args, **kw):
    a, la = run(ctx, 1, args, **kw)
    b, lb = run(ctx, 2, args, **kw)
    assert la.startswith(GENERAL) and lb.startswith(STEP), (la, lb)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.isfinite(a[k][1:]).all(), k
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
    assert a["F"][-1].min() > 0.0
    return b


def test_full_s_c2(ctx):
    out = same_bits(ctx, from_workload(synth.make_workload("S-c2")), keep_continuum_flux=True)
    assert set(out) == {"F", "total", "Fc"} and not np.array_equal(out["F"], out["Fc"])


def test_s_c1_sized_grid(ctx):
    same_bits(ctx, from_workload(synth.make_workload("S-c1")), keep_continuum_flux=True)


def test_zero_line_run(ctx):
    atm = synth.solar_atmosphere()
    out = same_bits(ctx, case(atm, synth.tracing_grid(6500.0, 6600.0, None, None, n_override=5000), 0), keep_continuum_flux=True)
    assert np.array_equal(out["F"], out["Fc"])  # no lines: both launches trace the continuum plane


def test_far_field_three_planes(ctx):
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(4000.0, 4300.0, R=1.0e5)
    args = case(atm, nus, 700, n_theta=4, seed=5)
    ctx.set_option("far_field", 0)
    try:
        two = same_bits(ctx, args)
        ctx.set_option("far_field", 1)
        three = same_bits(ctx, args, keep_continuum_flux=True)
    finally:
        ctx.set_option("far_field", -1)
    assert not np.array_equal(two["total"], three["total"])  # (the far field is a different sum: it did run)


def test_keep_total_off(ctx):
    w = synth.make_workload("S-c2")
    kept = same_bits(ctx, from_workload(w))
    bare = same_bits(ctx, from_workload(w), keep_total=False, keep_continuum_flux=True)
    assert "total" not in bare and np.array_equal(bare["F"], kept["F"])


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_angles(ctx, n_theta):
    """one angle per lane puts 64 frequencies' columns into a workgroup's LDS: 55 depth points are the most that fit 64 KB (at 56 neither
    segmented kernel is chosen and both modes would run k_raytrace_cont)"""
    atm = synth.solar_atmosphere()
    if n_theta == 1:
        atm = shallow(atm, 55)
    same_bits(ctx, case(atm, synth.tracing_grid(6500.0, 6600.0, None, None, n_override=3001), 300, n_theta=n_theta), keep_continuum_flux=True)


@pytest.mark.parametrize("n_depth", [9, 50, 56])
def test_depths(ctx, n_depth):
    """8, 49 and 55 gaps over eight waves: segments of 1, 7 and 7 gaps, the first wave's of 1, 0 and 6"""
    atm = shallow(synth.solar_atmosphere(), n_depth)
    out = same_bits(ctx, case(atm, synth.tracing_grid(6500.0, 6600.0, None, None, n_override=2999), 300), keep_continuum_flux=True)
    assert out["F"].shape[0] == n_depth


def test_two_way_shard_against_the_whole_grid(ctx):
    w = synth.make_workload("S-c2")
    args = from_workload(w)
    whole, _ = run(ctx, 1, args, keep_continuum_flux=True)
    parts = []
    for rank in range(2):
        part, label = run(ctx, 2, args, keep_continuum_flux=True, shard=shard_bounds(w["nus"].size, 2, rank))
        assert label.startswith(STEP)
        parts.append(part)
    for k in whole:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), k


def test_labels(ctx):
    args = from_workload(synth.make_workload("S-c1"))
    assert run(ctx, -1, args)[1] == STEP
    assert run(ctx, 2, args)[1] == STEP
    assert run(ctx, 1, args)[1] == GENERAL
    assert run(ctx, 2, args, keep_continuum_flux=True)[1] == STEP + " (continuum)"
    assert run(ctx, 1, args, keep_continuum_flux=True)[1] == GENERAL + " (continuum)"
    assert run(ctx, 0, args)[1] == "k_raytrace<1>"


def test_shapes_outside_the_rule_run_the_general_kernel(ctx):
    import ctypes as C

    args = from_workload(synth.make_workload("S-c1"))
    ref, label = run(ctx, 2, args, keep_line=True)  # the summed line plane is an output the step kernel does not write
    assert label == GENERAL
    step, _ = run(ctx, 2, args)
    assert np.array_equal(ref["F"], step["F"]) and np.array_equal(ref["total"], step["total"])
    # a caller's source plane
    nus, temps = args[0], args[1]
    syn = SpectralSynthesizer(*args, ctx=ctx, keep_line=False, track_evaluations=False)
    source = ctx.upload(np.ascontiguousarray(1.0e-5 * (nus[None, :] / nus[0]) ** 3 * (temps[:, None] / temps[0])))
    F = ctx.empty((temps.size, nus.size))
    opt = _lib.SynthesisOptions()
    opt.source, opt.source_ld = source.ptr, nus.size
    ctx.set_option("segmented_raytrace", 2)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        ctx.call("sdx_synthesize_opt_dev", syn.n_depth, syn.n_nu, syn.d_nus.ptr, 0, syn.count, syn.n_lines, syn.d_ln.ptr, syn.d_dw.ptr,
                 syn.d_g.ptr, syn.gamma_cols, syn.d_a.ptr, C.byref(syn.cont), syn.n_theta, syn.d_t.ptr, syn.d_ray.ptr, syn.d_w.ptr, None, None,
                 F.ptr, syn.count, C.byref(opt), None)
        ctx.synchronize()
        assert ctx.profile_variant("k_raytrace") == GENERAL
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
    assert np.isfinite(F.numpy()).all()
    syn.close()
