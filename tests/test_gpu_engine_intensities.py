"""SpectralSynthesizer(keep_intensities=True): the emergent intensity of every ray behind every step, its disk integration with rigid
rotation, and that through the instrument — each held bit for bit against the array-level entry it is built from, on the small model
of tests/test_gpu_response.py (12 depth points, 300 frequencies, 40 lines, 8 angles).  Without the option a step launches what it
launched."""
import numpy as np
import pytest

from stardis_amd import constants as K
from stardis_amd import ops
from stardis_amd.engine import shard_bounds
from stardis_amd.instrument import Instrument
from test_gpu_response import profiled, small_model, synthesizer

pytestmark = pytest.mark.gpu

NEW_STAGES = ("k_emergent_intensity", "k_disk_integrate")


@pytest.fixture(scope="module")
def m():
    return small_model()


@pytest.fixture(scope="module")
def stepped(ctx, m):
    """one synthesizer with the option, stepped once: (syn, total_alphas, emergent intensities on the host)"""
    syn = synthesizer(ctx, m, keep_intensities=True)
    syn.step()
    ctx.synchronize()
    yield syn, np.array(syn.total_alphas()), np.array(syn.emergent_intensities.numpy())
    syn.close()


def ray_table(m):
    return np.asarray(m.atm["dist"], dtype=np.float64).reshape(-1, 1) / np.cos(m.thetas)


def test_emergent_intensities_are_the_array_entrys(ctx, m, stepped):
    syn, total, I = stepped
    assert syn.keep_total and I.shape == (8, 300)
    want = ops.emergent_intensity(m.nus, m.atm["temperatures"], ray_table(m), total, ctx=ctx)
    assert np.array_equal(I, want) and np.all(np.isfinite(I)) and np.all(I > 0)
    # the limb is darker than the centre, and the flux of the step is their weighted sum in the flux's order (V = 0)
    assert I[0].mean() > I[-1].mean()
    lam = K.nu_to_angstrom(m.nus)
    F_lambda = syn.F_nu()[-1] * m.nus / lam
    flat = np.array(syn.disk_integrated(0.0).numpy())
    assert np.max(np.abs(flat - F_lambda)) <= 5e-13 * np.max(F_lambda)  # (the step's flux comes from the segmented kernel: the project's flux parity)


def test_a_second_step_and_a_graph_replay_repeat_the_bits(ctx, m, stepped):
    syn, _, I = stepped
    syn.d_I.zero()
    syn.step()
    ctx.synchronize()
    assert np.array_equal(syn.emergent_intensities.numpy(), I)
    syn.capture()
    try:
        assert syn.graph is not None
        syn.d_I.zero()
        syn.step()  # (the replay of the recorded step: the launch is part of it)
        ctx.synchronize()
        assert np.array_equal(syn.emergent_intensities.numpy(), I)
    finally:
        syn._destroy_graphs()


@pytest.mark.parametrize("v_rot", [0.0, 7.5, 60.0])
def test_disk_integrated_is_the_array_entrys(ctx, m, stepped, v_rot):
    syn, _, I = stepped
    lam = K.nu_to_angstrom(m.nus)
    rings = I * m.nus / lam  # sdx_flux_nu_to_lambda_dev's operation, ring by ring
    want = ops.disk_integrate(lam, rings, np.sin(m.thetas), m.weights, v_rot, ctx=ctx)
    got = np.array(syn.disk_integrated(v_rot).numpy())
    assert got.shape == (300,) and np.array_equal(got, want)
    if v_rot:
        assert not np.array_equal(got, syn.disk_integrated(0.0).numpy())


@pytest.mark.parametrize("v_mac", [None, 3.2])
def test_observed_disk_integrated_is_the_instrument_applied_by_hand(ctx, m, v_mac):
    lam = K.nu_to_angstrom(m.nus)
    edges = np.linspace(lam[40], lam[-40], 61)
    inst = Instrument(edges, resolving_power=4.0e4, ctx=ctx, v_mac=v_mac)
    inst.set_radial_velocity(12.0)
    syn = synthesizer(ctx, m, keep_intensities=True, instrument=inst)
    try:
        syn.step()
        got = np.array(syn.observed_disk_integrated(25.0).numpy())
        flux = syn.disk_integrated(25.0)
        if v_mac is not None:
            flux = inst.macroturbulence(syn.d_lambdas, flux, 300, out=ctx.empty((300,)))
        by_hand = np.array(inst.observe(syn.d_lambdas, flux, 300, out=ctx.empty((inst.n_pix,)), broadened=True).numpy())
        assert got.shape == (60,) and np.array_equal(got, by_hand, equal_nan=True) and np.isfinite(got).sum() >= 50
        twin = ops.observe(lam, np.array(syn.disk_integrated(25.0).numpy()), edges, inst.sigma, v_rad=12.0, ctx=ctx, **({} if v_mac is None else {"v_mac": v_mac}))
        assert np.array_equal(got, twin, equal_nan=True)
        # the step's own observed spectrum is the unrotated one
        assert not np.array_equal(got, syn.d_observed.numpy(), equal_nan=True)
    finally:
        syn.close()


def test_without_the_option_nothing_is_launched_or_allocated(ctx, m):
    syn = synthesizer(ctx, m)
    try:
        with profiled(ctx):
            syn.step()
            ctx.synchronize()
            plain = {name: ctx.profile(name)[0] for name in NEW_STAGES + ("k_raytrace",)}
        assert plain == {"k_emergent_intensity": 0, "k_disk_integrate": 0, "k_raytrace": 1}
        assert syn.keep_intensities is False and syn.d_I is None and syn._disk is None
        with pytest.raises(RuntimeError, match="keep_intensities=True"):
            syn.emergent_intensities
        with pytest.raises(RuntimeError, match="keep_intensities=True"):
            syn.disk_integrated(10.0)
        F = np.array(syn.F_nu())
    finally:
        syn.close()
    with_it = synthesizer(ctx, m, keep_intensities=True, keep_total=False)
    try:
        assert with_it.keep_total  # (forced: the kernel reads the step's total_alphas)
        with profiled(ctx):
            with_it.step()
            ctx.synchronize()
            assert ctx.profile("k_emergent_intensity")[0] == 1 and ctx.profile("k_disk_integrate")[0] == 0
            with_it.disk_integrated(10.0)
            assert ctx.profile("k_disk_integrate")[0] == 1
        assert np.array_equal(with_it.F_nu(), F)  # the step's flux does not change
    finally:
        with_it.close()


def test_a_shard_and_a_rotating_instrument_raise(ctx, m):
    begin, count = shard_bounds(300, 2, 1)
    syn = synthesizer(ctx, m, keep_intensities=True, shard=(begin, count))
    try:
        syn.step()
        ctx.synchronize()
        whole = ops.emergent_intensity(m.nus[begin:begin + count], m.atm["temperatures"], ray_table(m), syn.total_alphas(), ctx=ctx)
        assert np.array_equal(syn.emergent_intensities.numpy(), whole)  # a shard keeps its own columns
        with pytest.raises(ValueError, match="whole spectrum"):
            syn.disk_integrated(10.0)
    finally:
        syn.close()
    lam = K.nu_to_angstrom(m.nus)
    inst = Instrument(np.linspace(lam[40], lam[-40], 31), resolving_power=4.0e4, ctx=ctx, v_rot=5.0)
    syn = synthesizer(ctx, m, keep_intensities=True, instrument=inst)
    try:
        syn.step()
        with pytest.raises(ValueError, match="rotation twice"):
            syn.observed_disk_integrated(10.0)
        assert np.isfinite(syn.disk_integrated(10.0).numpy()).all()  # (the flux on the grid is still offered)
    finally:
        syn.close()
    bare = synthesizer(ctx, m, keep_intensities=True)
    try:
        bare.step()
        with pytest.raises(RuntimeError, match="instrument"):
            bare.observed_disk_integrated(10.0)
    finally:
        bare.close()


@pytest.mark.parametrize("spherical", [False, True], ids=["plane-parallel", "spherical"])
def test_solver_level_functions_follow_raytrace(ctx, m, stepped, spherical):
    """radiation_field_solvers.emergent_intensities is the last row of the I_nus that raytrace() fills, bit for bit (plain kernel), and
    disk_integrated_flux at v_rot = 0 is the F_lambda of raytrace()'s F_nu[-1] to rounding (the rings are converted one by one, the
    spherical correction applied last: other roundings than the flux's, a few ulp over 8 angles)"""
    import types

    from stardis_amd.radiation_field.radiation_field_solvers import base as solvers

    _, total, _ = stepped
    NS = types.SimpleNamespace
    dist = np.asarray(m.atm["dist"], dtype=np.float64)
    r = 6.0e10 + np.concatenate([[0.0], np.cumsum(dist)])
    model = NS(spherical=spherical, temperatures=m.atm["temperatures"], geometry=NS(dist_to_next_depth_point=dist, r=r, reference_r=r[-2]))
    field = NS(thetas=m.thetas, I_nus_weights=m.weights, frequencies=m.nus, opacities=NS(total_alphas=total), source_function=None,
               track_individual_intensities=True, F_nu=np.zeros((12, 300)), I_nus=np.zeros((12, 300, 8)))
    ctx.set_option("segmented_raytrace", 0)
    try:
        F = np.array(solvers.raytrace(model, field))
    finally:
        ctx.set_option("segmented_raytrace", -1)
    I = solvers.emergent_intensities(model, field)
    assert I.shape == (8, 300) and np.array_equal(I, field.I_nus[-1].T)
    lam = K.nu_to_angstrom(m.nus)
    want = F[-1] * m.nus / lam
    flat = solvers.disk_integrated_flux(model, field, 0.0)
    assert flat.shape == (300,) and np.max(np.abs(flat - want) / want) <= 16 * np.finfo(float).eps
    broad = solvers.disk_integrated_flux(model, field, 40.0)
    assert np.all(np.isfinite(broad)) and np.all(broad > 0) and not np.array_equal(broad, flat)


def test_the_constructor_asks_the_librarys_refusals(ctx, m):
    ctx.set_option("mixed_precision", 1)
    try:
        with pytest.raises(ValueError, match="mixed_precision"):
            synthesizer(ctx, m, keep_intensities=True)
    finally:
        ctx.set_option("mixed_precision", 0)
