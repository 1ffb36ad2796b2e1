"""The continuum flux traced beside the total one (SpectralSynthesizer(keep_continuum_flux=True), sdx_synthesis_options.
F_nu_continuum): F_nu of the same synthesis with no lines, bit for bit, on both formal-solution kernels; the step's own outputs
unchanged; the reference's raytrace of the continuum total; shards, graph replays and the normalised spectrum."""
import numpy as np
import pytest

import oracle
from conftest import rel_err
from stardis_amd import constants as K
from stardis_amd import synth
from stardis_amd.engine import SpectralSynthesizer, shard_bounds
from stardis_amd.postprocess import DeviceSpectrum
from test_gpu_engine import deep_atmosphere

pytestmark = pytest.mark.gpu


def no_lines(n_depth):
    return dict(line_nus=np.zeros(0), doppler_widths=np.zeros((0, n_depth)), gammas=np.zeros((0, n_depth)), alphas=np.zeros((0, n_depth)))


def run(ctx, w, lines, thetas=None, weights=None, **kw):
    atm = w["atm"]
    th = w["thetas"] if thetas is None else thetas
    wt = w["weights"] if weights is None else weights
    syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], th, wt, lines, w["cont"], ctx=ctx, **kw)
    syn.step()
    ctx.synchronize()
    return syn


@pytest.fixture(params=[-1, 0, 1], ids=["auto", "k_raytrace", "segmented"])
def seg_mode(request, ctx):
    ctx.set_option("segmented_raytrace", request.param)
    yield request.param
    ctx.set_option("segmented_raytrace", -1)


@pytest.mark.parametrize("tag,n_lines", [("S-c2", None), ("S-c3", 3000)], ids=["S-c2", "S-c3-3k"])
def test_continuum_flux_is_the_zero_line_flux(ctx, seg_mode, tag, n_lines):
    w = synth.make_workload(tag, n_lines=n_lines)
    plain = run(ctx, w, w["lines"])
    F, total, line = plain.F_nu(), plain.total_alphas(), plain.alpha_line()
    plain.close()
    both = run(ctx, w, w["lines"], keep_continuum_flux=True)
    assert np.array_equal(both.F_nu(), F)
    assert np.array_equal(both.total_alphas(), total)
    assert np.array_equal(both.alpha_line(), line)
    Fc = both.F_nu_continuum
    assert np.array_equal(both.emergent_continuum, Fc[-1])
    both.close()
    zero = run(ctx, w, no_lines(w["atm"]["temperatures"].size))
    assert np.array_equal(Fc, zero.F_nu())
    assert not np.array_equal(Fc, F)
    zero.close()


@pytest.mark.parametrize("n_theta,n_depth", [(1, 56), (4, 56), (20, 56), (20, 174), (20, 175)], ids=["1", "4", "20", "20-174deep", "20-175deep"])
def test_continuum_flux_against_oracle_raytrace(ctx, n_theta, n_depth):
    """The solar structure as it is (56 depths), and resampled to 174 and 175: at 20 angles k_raytrace_cont<1> stages 3 frequencies
    per wave up to 174 depths and 2 from 175 on (its third column and second batch of flux terms), where k_raytrace<1> still stages 3."""
    w = synth.make_workload("S-c1", n_lines=300)
    if n_depth != 56:
        w["atm"] = deep_atmosphere(n_depth)
        w["lines"] = synth.synth_lines(w["nus"], w["atm"], 300)
        w["cont"] = synth.synth_continuum_state(w["atm"])
    th, wt = synth.thetas_and_weights(n_theta)
    zero = run(ctx, w, no_lines(w["atm"]["temperatures"].size), thetas=th, weights=wt)
    cont_total = zero.total_alphas()
    zero.close()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        syn = run(ctx, w, w["lines"], thetas=th, weights=wt, keep_continuum_flux=True)
        variant = ctx.profile_variant("k_raytrace")
    finally:
        ctx.call("sdx_profile_enable", 0)
    if n_depth != 56:
        assert variant == "k_raytrace_cont<1>"
    atm = w["atm"]
    ref, _ = oracle.raytrace(w["nus"], atm["temperatures"], atm["dist"], th, wt, cont_total)
    assert rel_err(syn.F_nu_continuum, ref) <= 1e-10
    syn.close()


def test_shards_concatenate_to_the_whole_continuum(ctx):
    w = synth.make_workload("S-c2")
    whole = run(ctx, w, w["lines"], keep_continuum_flux=True)
    Fc = whole.F_nu_continuum
    whole.close()
    parts = []
    for r in range(2):
        syn = run(ctx, w, w["lines"], shard=shard_bounds(w["nus"].size, 2, r), keep_continuum_flux=True)
        parts.append(syn.F_nu_continuum)
        syn.close()
    assert np.array_equal(np.concatenate(parts, axis=1), Fc)


def test_graph_replay_equals_eager_step(ctx):
    w = synth.make_workload("S-c2")
    eager = run(ctx, w, w["lines"], keep_continuum_flux=True)
    F, Fc = eager.F_nu(), eager.F_nu_continuum
    eager.close()
    syn = SpectralSynthesizer(w["nus"], w["atm"]["temperatures"], w["atm"]["dist"], w["thetas"], w["weights"], w["lines"], w["cont"],
                              ctx=ctx, keep_continuum_flux=True, track_evaluations=False)
    syn.capture()
    syn.d_Fc.set(np.zeros_like(Fc))
    syn.step()
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.F_nu(), F)
    assert np.array_equal(syn.F_nu_continuum, Fc)
    syn.close()


def test_mixed_precision_refuses_the_continuum(ctx):
    w = synth.make_workload("S-c1", n_lines=100)
    ctx.set_option("mixed_precision", 1)
    try:
        with pytest.raises(ValueError, match="mixed_precision"):
            run(ctx, w, w["lines"], keep_continuum_flux=True)
    finally:
        ctx.set_option("mixed_precision", 0)


def test_continuum_is_required_for_the_properties(ctx):
    w = synth.make_workload("S-c1", n_lines=100)
    syn = run(ctx, w, w["lines"])
    with pytest.raises(RuntimeError):
        syn.F_nu_continuum
    with pytest.raises(RuntimeError):
        DeviceSpectrum(syn).normalized()
    syn.close()


def test_normalized_spectrum_against_host_filters(ctx):
    w = synth.make_workload("S-c2")
    syn = run(ctx, w, w["lines"], keep_continuum_flux=True)
    lam = K.nu_to_angstrom(w["nus"])
    f_lam = syn.F_nu()[-1] * w["nus"] / lam
    c_lam = syn.F_nu_continuum[-1] * w["nus"] / lam
    spec = DeviceSpectrum(syn)
    sigma, vpp, v_rot = 3.0, 0.6, 20.0
    got = spec.normalized(sigma_pix=sigma, velocity_per_pix=vpp, v_rot=v_rot).numpy()
    f = oracle.rotation_broadening(oracle.gaussian_filter1d(f_lam, sigma), vpp, v_rot)
    c = oracle.rotation_broadening(oracle.gaussian_filter1d(c_lam, sigma), vpp, v_rot)
    assert rel_err(got, f / c) <= 1e-12
    plain = spec.normalized().numpy()
    assert rel_err(plain, f_lam / c_lam) <= 1e-12
    assert plain.min() < 1.0 and plain.max() <= 1.0 + 1e-9  # absorption lines below the continuum
    syn.close()


def opt_step(ctx, syn, ray, opt, F, total=None):
    """One sdx_synthesize_opt_dev step on the synthesizer's resident inputs with a caller-chosen ray table and options."""
    import ctypes as C

    ctx.call("sdx_synthesize_opt_dev", syn.n_depth, syn.n_nu, syn.d_nus.ptr, 0, syn.count, syn.n_lines, syn.d_ln.ptr, syn.d_dw.ptr,
             syn.d_g.ptr, syn.gamma_cols, syn.d_a.ptr, C.byref(syn.cont), syn.n_theta, syn.d_t.ptr, ray.ptr, syn.d_w.ptr, None,
             total.ptr if total is not None else None, F.ptr, syn.count, C.byref(opt), None)
    ctx.synchronize()


def test_spherical_continuum_against_oracle(ctx):
    """inward sweep of both chains, the row-0 flux of the sweep and the photospheric correction of the continuum (k_raytrace_cont:
    the segmented kernel takes no inward rays)"""
    from stardis_amd import _lib

    w = synth.make_workload("S-c1", n_lines=300)
    atm, nus = w["atm"], w["nus"]
    th, wt = synth.thetas_and_weights(8)
    nd = atm["temperatures"].size
    r = 7.0e10 + np.concatenate([[0.0], np.cumsum(np.asarray(atm["dist"]))])
    ref_r = r[-12]
    ray = ctx.upload(np.ascontiguousarray(oracle.calculate_spherical_ray(th, r)))
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, wt, w["lines"], w["cont"], ctx=ctx)
    syn0 = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, wt, no_lines(nd), w["cont"], ctx=ctx)
    out = {k: ctx.empty((nd, nus.size)) for k in ("F", "F_on", "Fc", "F0", "total0")}
    opt = _lib.SynthesisOptions()
    opt.inward_rays, opt.photospheric_correction = 1, (r[-1] / ref_r) ** 2
    opt_step(ctx, syn, ray, opt, out["F"])
    opt_step(ctx, syn0, ray, opt, out["F0"], out["total0"])
    opt.F_nu_continuum, opt.continuum_ld = out["Fc"].ptr, nus.size
    opt_step(ctx, syn, ray, opt, out["F_on"])
    F, F_on, Fc, F0 = (out[k].numpy() for k in ("F", "F_on", "Fc", "F0"))
    assert np.array_equal(F_on, F)
    assert np.array_equal(Fc, F0)
    ref, _ = oracle.raytrace(nus, atm["temperatures"], None, th, wt, out["total0"].numpy(), spherical_r=r, reference_r=ref_r)
    assert rel_err(Fc, ref) <= 1e-10
    assert Fc[0].any()  # the inward sweep's flux at the innermost point
    syn.close(), syn0.close()


@pytest.mark.parametrize("seg", [-1, 0], ids=["segmented", "k_raytrace"])
def test_caller_source_plane(ctx, seg):
    from stardis_amd import _lib

    w = synth.make_workload("S-c1", n_lines=300)
    atm, nus = w["atm"], w["nus"]
    nd = atm["temperatures"].size
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx)
    syn0 = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], no_lines(nd), w["cont"], ctx=ctx)
    x = (K.H_CGS * nus[None, :]) / (K.K_B_CGS * atm["temperatures"][:, None])
    source = ctx.upload(np.ascontiguousarray(1.3e-5 * nus[None, :] ** 3 / np.expm1(x) * (1.0 + 0.1 * np.sin(np.arange(nd))[:, None])))
    out = {k: ctx.empty((nd, nus.size)) for k in ("F", "F_on", "Fc", "F0")}
    opt = _lib.SynthesisOptions()
    opt.source, opt.source_ld = source.ptr, nus.size
    ctx.set_option("segmented_raytrace", seg)
    try:
        opt_step(ctx, syn, syn.d_ray, opt, out["F"])
        opt_step(ctx, syn0, syn0.d_ray, opt, out["F0"])
        opt.F_nu_continuum, opt.continuum_ld = out["Fc"].ptr, nus.size
        opt_step(ctx, syn, syn.d_ray, opt, out["F_on"])
    finally:
        ctx.set_option("segmented_raytrace", -1)
    assert np.array_equal(out["F_on"].numpy(), out["F"].numpy())
    assert np.array_equal(out["Fc"].numpy(), out["F0"].numpy())
    syn.close(), syn0.close()


@pytest.mark.parametrize("seg", [-1, 0], ids=["segmented", "k_raytrace"])
def test_line_list_and_line_plane_are_excluded(ctx, seg):
    """f1 (per-line scalars, the engine's linelist branch) and an extra molecular-style line plane: neither reaches the continuum"""
    from stardis_amd import _lib

    w = synth.make_workload("S-c1", n_lines=300)
    atm, nus = w["atm"], w["nus"]
    nd = atm["temperatures"].size
    ctx.set_option("segmented_raytrace", seg)
    try:
        zero = run(ctx, w, no_lines(nd))
        F0 = zero.F_nu()
        ll = synth.synth_linelist(nus, atm, 300, synth.SEED)
        plain = run(ctx, w, ll)
        f1 = run(ctx, w, ll, keep_continuum_flux=True)
        assert np.array_equal(f1.F_nu(), plain.F_nu())
        assert np.array_equal(f1.F_nu_continuum, F0)
        # an extra line plane (include_molecules): the step's dense lines plus the plane; continuum = zero-line flux
        syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx)
        plane = ctx.upload(np.ascontiguousarray(0.5 * zero.total_alphas() * (1.0 + np.cos(np.arange(nus.size))[None, :] ** 2)))
        out = {k: ctx.empty((nd, nus.size)) for k in ("F", "F_on", "Fc")}
        opt = _lib.SynthesisOptions()
        opt.n_line_planes, opt.line_plane[0], opt.line_plane_ld = 1, plane.ptr, nus.size
        opt_step(ctx, syn, syn.d_ray, opt, out["F"])
        opt.F_nu_continuum, opt.continuum_ld = out["Fc"].ptr, nus.size
        opt_step(ctx, syn, syn.d_ray, opt, out["F_on"])
        assert np.array_equal(out["F_on"].numpy(), out["F"].numpy())
        assert np.array_equal(out["Fc"].numpy(), F0)
        for s in (zero, plain, f1, syn):
            s.close()
    finally:
        ctx.set_option("segmented_raytrace", -1)


def test_two_collective_phase_two(ctx):
    """the synthesis after the classification (line_m_max) on a culled long-list shard: the shard's continuum equals the unsharded one"""
    from test_gpu_round5 import long_list_case

    atm, nus, lines, cont, th, w = long_list_case(n_nu=20000, n_lines=9000)
    args = (nus, atm["temperatures"], atm["dist"], th, w, lines, cont)
    whole = SpectralSynthesizer(*args, ctx=ctx, track_evaluations=False, keep_continuum_flux=True)
    whole.step()
    F, Fc = whole.F_nu(), whole.F_nu_continuum
    whole.close()
    n_l = lines["line_nus"].size
    b, c = shard_bounds(nus.size, 4, 1)
    syn = SpectralSynthesizer(*args, ctx=ctx, shard=(b, c), track_evaluations=False, classify_share=(0, n_l), m_max=ctx.zeros((n_l,)),
                              keep_continuum_flux=True)
    syn.enqueue_classify()
    syn.enqueue()
    ctx.synchronize()
    assert np.array_equal(syn.F_nu(), F[:, b:b + c])
    assert np.array_equal(syn.F_nu_continuum, Fc[:, b:b + c])
    syn.close()
