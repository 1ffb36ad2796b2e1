"""The flux contribution function through the drop-in: create_stellar_radiation_field(..., contribution=True) on the fused path and
on the general (source-by-source) path — the same bits on both —, the plain functions contribution_function / formation_mean,
run_stardis(..., contribution=True, continuum=True), and the refusal of spherical models before any device work."""
import types

import numpy as np
import pytest

import contribution_reference as cref
from stardis_amd import constants as K
from stardis_amd import synth
from test_gpu_continuum_dropin import case, field

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace


@pytest.mark.parametrize("variant,seg", [("plain", -1), ("plain", 0), ("molecules", -1), ("f1", -1)])
def test_contribution_field_fused_and_general(ctx, monkeypatch, variant, seg):
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    nus, plasma, model, config = case(variant)
    ctx.set_option("segmented_raytrace", seg)
    try:
        got = {}
        for fused in (True, False):
            plain = field(monkeypatch, fused, nus, model, plasma, config)
            assert not hasattr(plain, "contribution_function")
            both = field(monkeypatch, fused, nus, model, plasma, config, contribution=True, continuum=True)
            assert type(both.opacities).__name__ == ("FusedOpacities" if fused else "Opacities")
            assert np.array_equal(both.F_nu, plain.F_nu)
            Cf = both.contribution_function
            assert isinstance(Cf, np.ndarray) and Cf.shape == both.F_nu.shape and not Cf[0].any()
            F = both.F_nu[-1]
            err = np.max(np.abs(Cf.sum(axis=0) - F) / F)
            print(f"{variant} fused={fused}: max |sum_k C - F_nu[-1]| / F_nu[-1] = {err:.3e}")
            assert err <= 1e-12
            assert np.array_equal(rfs.contribution_function(model, both), Cf)  # the plain function, on the field's own opacities
            t = np.asarray(model.temperatures.value if hasattr(model.temperatures, "value") else model.temperatures, dtype=np.float64)
            assert np.array_equal(rfs.formation_mean(both, t), cref.formation_mean(Cf, t), equal_nan=True)
            got[fused] = np.array(Cf)
        assert np.array_equal(got[True], got[False])
    finally:
        ctx.set_option("segmented_raytrace", -1)


def test_spherical_model_is_refused_before_any_device_work(ctx, monkeypatch):
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    nus, plasma, model, config = case("spherical")
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        for fused in (True, False):
            with pytest.raises(NotImplementedError, match="plane-parallel"):
                field(monkeypatch, fused, nus, model, plasma, config, contribution=True)
        with pytest.raises(NotImplementedError, match="plane-parallel"):
            rfs.contribution_function(model, NS())
        launches = sum(ctx.profile(k)[0] for k in ("k_contribution", "k_raytrace", "k_prepass_continuum", "k_line_prepass", "k_total_alphas"))
    finally:
        ctx.call("sdx_profile_enable", 0)
    assert launches == 0


@pytest.mark.parametrize("continuum", [True, False])
def test_run_stardis_carries_the_contribution_function(ctx, monkeypatch, continuum):
    import stardis_amd.base as gpu_base
    from test_gpu_run_stardis import Quantity, install_stubs

    lambdas = np.arange(6555.0, 6575.0, 0.02)
    nus = K.C_CGS * 1.0e8 / lambdas
    plasma, model, config, _ = synth.fake_plasma(nus, synth.solar_atmosphere(), 300, seed=43)
    config.n_threads = 2
    config.result_options = NS(return_model=False, return_plasma=False, return_radiation_field=False)
    install_stubs(monkeypatch, plasma, model, config, [])
    sim = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"), contribution=True, continuum=continuum)
    Cf = sim.contribution_function
    assert Cf is sim.stellar_radiation_field.contribution_function and Cf.shape == (model.no_of_depth_points, nus.size)
    spectrum = np.asarray(getattr(sim.spectrum_nu, "value", sim.spectrum_nu), dtype=np.float64)
    assert np.max(np.abs(Cf.sum(axis=0) - spectrum) / spectrum) <= 1e-12
    assert hasattr(sim, "spectrum_normalized") == continuum and hasattr(sim, "spectrum_nu_continuum") == continuum
    plain = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"))
    assert np.array_equal(plain.spectrum_nu, sim.spectrum_nu) and not hasattr(plain, "contribution_function")
    model.spherical = True
    with pytest.raises(NotImplementedError, match="plane-parallel"):
        gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"), contribution=True)
