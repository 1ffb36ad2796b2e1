"""Drop-in driver: the reference's pipeline (stardis/base.py:13-45) with the radiation field on MI355X.

Config/model I/O and the TARDIS plasma stay the reference's (they are imported from an installed `stardis`); only
`create_stellar_radiation_field` — opacity assembly + formal solution — is replaced.  Needs `stardis`, `tardis` and
`astropy` installed, exactly like the reference; the hot path itself needs none of them.
"""
import logging

from stardis_amd.radiation_field.base import create_stellar_radiation_field

logger = logging.getLogger(__name__)


def run_stardis(config_fname, tracing_lambdas_or_nus, add_config_dict=None, *, continuum=False, contribution=False, instrument=None):
    """Same signature and return type as stardis.base.run_stardis.  continuum=True: the same single synthesis also traces the
    continuum, and the output gains spectrum_nu_continuum and spectrum_lambda_continuum (built as STARDISOutput builds
    spectrum_nu / spectrum_lambda, stardis/base.py:133-141) and spectrum_normalized = spectrum_nu / spectrum_nu_continuum —
    what a second run with opacity.line.disable (and no molecules) would give.
    contribution=True (plane-parallel models; combines with continuum): the output gains contribution_function (N_d, N_nu), what the
    layer below each depth point adds to the emergent flux — its sum over depth is spectrum_nu up to rounding
    (radiation_field_solvers.contribution_function, formation_mean).  A spherical model raises NotImplementedError.
    instrument (a stardis_amd.instrument.Instrument): the output gains spectrum_observed (n_pix,), spectrum_lambda through the instrument
    (radial velocity, line-spread function, pixels; Instrument.observe_host); with continuum=True also spectrum_observed_normalized, the
    same with spectrum_lambda_continuum as reference.  Works unchanged with a rotating instrument (Instrument(v_rot=...)): the star's
    rotation is applied in front of the pixels; Instrument(v_mac=...) adds the radial-tangential macroturbulence behind it."""
    try:
        from astropy import units as u
        from stardis.base import STARDISOutput, set_num_threads
        from stardis.io.base import parse_config_to_model
        from stardis.plasma import create_stellar_plasma
    except ImportError as exc:  # pragma: no cover - depends on the user's environment
        raise ImportError(
            "run_stardis needs the reference package for configuration, model I/O and the TARDIS plasma "
            "(pip install stardis); stardis_amd replaces only the radiation-field stage"
        ) from exc

    tracing_nus = tracing_lambdas_or_nus.to(u.Hz, u.spectral())  # wavelengths ascending -> frequencies descending
    config, adata, stellar_model = parse_config_to_model(config_fname, add_config_dict)
    set_num_threads(config.n_threads)  # still governs the plasma stage
    if contribution and bool(getattr(stellar_model, "spherical", False)):  # (before the plasma and any device work)
        from stardis_amd.radiation_field.radiation_field_solvers.base import SPHERICAL_CONTRIBUTION

        raise NotImplementedError(SPHERICAL_CONTRIBUTION)
    stellar_plasma = create_stellar_plasma(stellar_model, adata, config)
    if not continuum and not contribution:
        stellar_radiation_field = create_stellar_radiation_field(tracing_nus, stellar_model, stellar_plasma, config)
        sim = STARDISOutput(config.result_options, stellar_model, stellar_plasma, stellar_radiation_field)
        if instrument is not None:
            _add_observed_spectra(sim, instrument, False)
        return sim
    stellar_radiation_field = create_stellar_radiation_field(tracing_nus, stellar_model, stellar_plasma, config, continuum=continuum,
                                                             contribution=contribution)
    sim = STARDISOutput(config.result_options, stellar_model, stellar_plasma, stellar_radiation_field)
    if continuum:
        _add_continuum_spectra(sim, stellar_radiation_field.F_nu_continuum)
    if contribution:
        sim.contribution_function = stellar_radiation_field.contribution_function
    if instrument is not None:
        _add_observed_spectra(sim, instrument, continuum)
    return sim


def _add_observed_spectra(sim, instrument, continuum):
    """(plain arrays, the values in the unit of spectrum_lambda: the instrument's pixels are not the model's grid)"""
    sim.spectrum_observed = instrument.observe_host(sim.lambdas, sim.spectrum_lambda)
    if continuum:
        sim.spectrum_observed_normalized = instrument.observe_host(sim.lambdas, sim.spectrum_lambda, reference=sim.spectrum_lambda_continuum)


def _add_continuum_spectra(sim, F_nu_continuum):
    from astropy import units as u

    nus, lambdas = sim.nus, sim.lambdas
    try:
        flux_nu_unit, flux_lambda_unit = u.erg / u.s / u.cm**2 / u.Hz, u.erg / u.s / u.cm**2 / u.AA
    except AttributeError:  # (an astropy without the cgs units, as in the package's own tests: plain arrays, as spectrum_nu is there)
        F_nu = F_nu_continuum
        F_lambda = F_nu * getattr(nus, "value", nus) / getattr(lambdas, "value", lambdas)
    else:
        F_nu = F_nu_continuum * flux_nu_unit
        F_lambda = (F_nu * nus / lambdas).to(flux_lambda_unit)
    sim.spectrum_nu_continuum = F_nu[-1]
    sim.spectrum_lambda_continuum = F_lambda[-1]
    sim.spectrum_normalized = sim.spectrum_nu / sim.spectrum_nu_continuum


def patch_stardis():
    """Make an installed `stardis` use the GPU radiation field everywhere: stardis.base.run_stardis looks the function
    up in its own module namespace (stardis/base.py:5,39)."""
    import stardis.base as ref

    ref.create_stellar_radiation_field = create_stellar_radiation_field
    return ref
