"""The continuum through the drop-in: create_stellar_radiation_field(..., continuum=True) on the fused path and on the general
(source-by-source) path, and run_stardis(..., continuum=True).  The continuum flux is F_nu of the same configuration with
opacity.line.disable = True and include_molecules = False, bit for bit, on both paths; F_nu is unchanged by the option."""
import copy
import types

import numpy as np
import pytest

from stardis_amd import constants as K
from stardis_amd import synth

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace


def case(variant):
    nus = synth.tracing_grid(6560.0, 6570.0, step=0.02)
    atm = synth.solar_atmosphere()
    plasma, model, config, _ = synth.fake_plasma(nus, atm, 300, seed=41, n_molecule_lines=200 if variant == "molecules" else 0)
    config.no_of_thetas = 8
    if variant == "molecules":
        config.opacity.line.include_molecules = True
    if variant == "f1":
        plasma.alpha_line_from_linelist = None  # per-line scalars: the pre-pass generates alpha, gamma, Doppler width
    if variant == "spherical":
        model.spherical = True
        r = 7.0e10 + np.concatenate([[0.0], np.cumsum(np.asarray(model.geometry.dist_to_next_depth_point))])
        model.geometry = NS(dist_to_next_depth_point=model.geometry.dist_to_next_depth_point, r=r, reference_r=r[-12])
        config.result_options = NS(return_radiation_field=True)  # tracked intensities next to the continuum
    return nus, plasma, model, config


def field(monkeypatch, fused, nus, model, plasma, config, **kw):
    import stardis_amd.radiation_field.base as rf

    monkeypatch.setattr(rf, "FUSED", fused)
    return rf.create_stellar_radiation_field(nus.copy(), model, plasma, config, **kw)


@pytest.mark.parametrize("variant,seg", [("plain", -1), ("plain", 0), ("molecules", -1), ("f1", -1), ("spherical", -1)])
def test_continuum_field_fused_and_general(ctx, monkeypatch, variant, seg):
    nus, plasma, model, config = case(variant)
    no_lines = copy.deepcopy(config)
    no_lines.opacity.line.disable = True
    no_lines.opacity.line.include_molecules = False
    ctx.set_option("segmented_raytrace", seg)
    try:
        got = {}
        for fused in (True, False):
            plain = field(monkeypatch, fused, nus, model, plasma, config)
            assert not hasattr(plain, "F_nu_continuum")
            both = field(monkeypatch, fused, nus, model, plasma, config, continuum=True)
            assert type(both.opacities).__name__ == ("FusedOpacities" if fused else "Opacities")
            assert np.array_equal(both.F_nu, plain.F_nu)
            if variant == "spherical":
                assert np.array_equal(both.I_nus, plain.I_nus, equal_nan=True)
            assert both.F_nu_continuum.shape == both.F_nu.shape
            zero = field(monkeypatch, fused, nus, model, plasma, no_lines)
            assert np.array_equal(both.F_nu_continuum, zero.F_nu)
            assert not np.array_equal(both.F_nu_continuum, both.F_nu)
            got[fused] = both.F_nu_continuum
        assert np.array_equal(got[True], got[False])
    finally:
        ctx.set_option("segmented_raytrace", -1)


@pytest.mark.parametrize("continuum", [True, False])
def test_run_stardis_continuum_attributes(ctx, monkeypatch, continuum):
    import stardis_amd.base as gpu_base
    from test_gpu_run_stardis import Quantity, install_stubs

    lambdas = np.arange(6555.0, 6575.0, 0.02)
    nus = K.C_CGS * 1.0e8 / lambdas
    plasma, model, config, _ = synth.fake_plasma(nus, synth.solar_atmosphere(), 300, seed=43)
    config.n_threads = 2
    config.result_options = NS(return_model=False, return_plasma=False, return_radiation_field=False)
    install_stubs(monkeypatch, plasma, model, config, [])
    kw = dict(continuum=True) if continuum else {}
    sim = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"), **kw)
    names = ("spectrum_nu_continuum", "spectrum_lambda_continuum", "spectrum_normalized")
    if not continuum:
        assert not any(hasattr(sim, n) for n in names)
        return
    field = sim.stellar_radiation_field
    Fc = field.F_nu_continuum
    assert np.array_equal(sim.spectrum_nu_continuum, Fc[-1])
    assert np.array_equal(sim.spectrum_lambda_continuum, (Fc * nus / lambdas)[-1])  # as spectrum_lambda (stardis/base.py:137-141)
    assert np.array_equal(sim.spectrum_normalized, sim.spectrum_nu / Fc[-1])
    assert sim.spectrum_normalized.min() < 1.0 and sim.spectrum_normalized.max() <= 1.0 + 1e-9
    plain = gpu_base.run_stardis("sun.yml", Quantity(lambdas, "AA"))
    assert np.array_equal(plain.spectrum_nu, sim.spectrum_nu)
