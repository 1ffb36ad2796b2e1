"""k_raytrace_seg_step after the change of what a wave pays around its gaps — the flux sum of 20 angles as five 16-byte reads per half,
the pair's sums exchanged inside the quad, the fallback's rolled loop for every other angle count, F's row stride as 32 bits: F_nu,
total_alphas and the continuum flux numpy.array_equal between "segmented_raytrace" = 1 (k_raytrace_seg<8,7>, untouched) and 2 (the
step kernel), at the smallest shapes where each part can go wrong:
  angles   1 (64 columns per workgroup, no idle lane), 4 (16 columns, a half of two angles: aligned, but not the 128-bit form),
           19 and 21 (odd: halves of 10 + 9 and 11 + 10, runs that start at odd doubles), 20 (the 128-bit form)
  depths   9, 50 (a first wave without gaps), 55 and 56 (a first wave of 5 and 6 gaps: fewer items than the other waves'; 56 is the
           last depth the kernel is chosen at)
  columns  a count that is no multiple of the columns per workgroup (the last workgroup partly idle), and fewer than one workgroup's
  planes   0, 2 and 3 (the far field forced); total_alphas kept and not
  the ray table and the weights rewritten between two steps of one synthesizer: each step equals a fresh synthesizer's (nothing is
  cached from the rays today; the case is what a cached table would have to pass)."""
import numpy as np
import pytest

from stardis_amd import synth
from stardis_amd.engine import SpectralSynthesizer
from test_gpu_step_raytrace import GENERAL, STEP, case, run, same_bits, shallow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def atm():
    return synth.solar_atmosphere()


def grid(n):
    return synth.tracing_grid(6500.0, 6600.0, None, None, n_override=n)


@pytest.mark.parametrize("n_theta", [1, 4, 19, 20, 21])
def test_angles(ctx, atm, n_theta):
    """1001 columns: 15 workgroups of 64 + 41, 62 of 16 + 9, 333 of 3 + 2"""
    a = shallow(atm, 55) if n_theta == 1 else atm  # (one angle: 55 depths are the most whose 64 columns fit LDS)
    same_bits(ctx, case(a, grid(1001), 120, n_theta=n_theta), keep_continuum_flux=True)


@pytest.mark.parametrize("n_depth", [9, 50, 55, 56])
def test_depths(ctx, atm, n_depth):
    out = same_bits(ctx, case(shallow(atm, n_depth), grid(1000), 120), keep_continuum_flux=True)
    assert out["F"].shape == (n_depth, 1000)


@pytest.mark.parametrize("n_theta,n_nu", [(20, 2), (4, 9), (1, 40)])
def test_fewer_columns_than_a_workgroup_holds(ctx, atm, n_theta, n_nu):
    a = shallow(atm, 55) if n_theta == 1 else atm
    out = same_bits(ctx, case(a, grid(n_nu), 20, n_theta=n_theta), keep_continuum_flux=True)
    assert out["F"].shape[1] == n_nu


def test_zero_two_and_three_planes(ctx, atm):
    nus = synth.tracing_grid(4000.0, 4300.0, R=1.0e5)  # (7232 columns: the grid on which the forced far field is known to differ)
    zero = same_bits(ctx, case(atm, nus, 0), keep_continuum_flux=True)
    assert np.array_equal(zero["F"], zero["Fc"])
    args = case(atm, nus, 700, seed=5)
    ctx.set_option("far_field", 0)
    try:
        two = same_bits(ctx, args, keep_continuum_flux=True)
        ctx.set_option("far_field", 1)
        three = same_bits(ctx, args, keep_continuum_flux=True)
    finally:
        ctx.set_option("far_field", -1)
    assert not np.array_equal(two["total"], three["total"])  # (the far field is a different sum: it did run)
    assert np.array_equal(two["Fc"], zero["Fc"])


def test_keep_total_off(ctx, atm):
    args = case(atm, grid(1001), 120)
    kept = same_bits(ctx, args)
    bare = same_bits(ctx, args, keep_total=False, keep_continuum_flux=True)
    assert "total" not in bare and np.array_equal(bare["F"], kept["F"])


def test_rays_changed_between_two_steps(ctx, atm):
    """thetas (the ray table and the weights), then the depth grid's distances (the ray table alone), written into the buffers of one
    synthesizer between its steps: each step equals the step of a synthesizer made with those values — nothing a step derives from
    the rays outlives them"""
    nus = grid(1001)
    args = list(case(atm, nus, 120))
    th2, w2 = synth.thetas_and_weights(20)
    th2 = np.ascontiguousarray(th2[::-1] * 0.93)  # (other angles in another order; the weights follow them)
    w2 = np.ascontiguousarray(w2[::-1] * 1.07)
    dist3 = np.ascontiguousarray(atm["dist"] * np.linspace(0.8, 1.3, atm["dist"].size))
    ray = lambda dist, th: np.ascontiguousarray(np.asarray(dist, dtype=np.float64).reshape(-1, 1) / np.cos(th))  # noqa: E731
    ctx.set_option("segmented_raytrace", 2)
    ctx.call("sdx_profile_enable", 1)
    try:
        syn = SpectralSynthesizer(*args, ctx=ctx, keep_line=False, track_evaluations=False, keep_continuum_flux=True)
        syn.step()
        first = syn.F_nu().copy()
        assert ctx.profile_variant("k_raytrace").startswith(STEP)
        seen = []
        for dist, th, w in ((atm["dist"], th2, w2), (dist3, th2, w2)):
            syn.d_ray.set(ray(dist, th))
            syn.d_w.set(w)
            syn.step()
            seen.append((syn.F_nu().copy(), syn.F_nu_continuum.copy()))
        syn.close()
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
    assert not np.array_equal(seen[0][0], first) and not np.array_equal(seen[1][0], seen[0][0])
    for (F, Fc), dist in zip(seen, (atm["dist"], dist3)):
        fresh = list(args)
        fresh[2], fresh[3], fresh[4] = dist, th2, w2
        for mode, label in ((1, GENERAL), (2, STEP)):
            ref, got = run(ctx, mode, fresh, keep_continuum_flux=True)
            assert got.startswith(label)
            assert np.array_equal(ref["F"], F) and np.array_equal(ref["Fc"], Fc), mode
