"""The instrument model at build time and on the host: the entry points are declared, exported and mirrored; k_observe compiles for
gfx950 without spilled vector registers; the Instrument's validation raises before any device is asked for; and the properties of
the numpy restatement (tests/observe_reference.py) that pin the definition the device is held against."""
import ctypes
import os
import re

import numpy as np
import pytest

import observe_reference as oref
from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib

ENTRIES = {"sdx_observe_dev": 10, "sdx_observe_f64": 10}


def test_entry_points_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
    assert _lib.PROTOTYPES["sdx_observe_f64"][1][8] is ctypes.c_double  # the Doppler factor by value; the device entry reads a scalar
    assert _lib.PROTOTYPES["sdx_observe_dev"][1][8] is ctypes.c_void_p


def test_observe_kernel_does_not_spill(resources):  # noqa: F811
    found = [v for name, v in resources.items() if name.endswith("k_observe")]
    assert len(found) == 1, sorted(resources)
    print(found[0])
    assert found[0]["spill"] == 0, found[0]


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_observe_dev(None, 4, None, None, None, 1, None, None, None, None) == -1
    assert b"observe" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_observe_f64(None, 4, None, None, None, 1, None, None, 1.0, None) == -1


def test_instrument_validation_needs_no_device():
    from stardis_amd.instrument import Instrument, doppler_factor, pixel_sigma

    edges = np.linspace(6560.0, 6570.0, 11)
    bad = [
        dict(pixel_edges=edges),  # neither
        dict(pixel_edges=edges, resolving_power=5e4, sigma=0.1),  # both
        dict(pixel_edges=edges[::-1], resolving_power=5e4),
        dict(pixel_edges=np.r_[edges[:5], edges[4:]], resolving_power=5e4),  # a repeated edge
        dict(pixel_edges=np.r_[edges[:5], np.nan, edges[6:]], sigma=0.1),
        dict(pixel_edges=edges, sigma=0.0),
        dict(pixel_edges=edges, sigma=np.r_[np.full(9, 0.1), -1.0]),
        dict(pixel_edges=edges, sigma=np.full(9, 0.1)),  # one value too few
        dict(pixel_edges=edges, resolving_power=np.inf),
        dict(pixel_edges=edges.reshape(1, -1), sigma=0.1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            Instrument(**kw)
    e, s = pixel_sigma(edges, resolving_power=5e4)
    assert np.array_equal(s, (edges[:-1] + edges[1:]) / 2 / (5e4 * 2 * np.sqrt(2 * np.log(2)))) and np.array_equal(e, edges)
    assert np.array_equal(pixel_sigma(edges, sigma=0.07)[1], np.full(10, 0.07))
    assert doppler_factor(0.0) == 1.0 and doppler_factor(30.0) == oref.doppler_factor(30.0)
    with pytest.raises(ValueError):
        doppler_factor(3e5)
    if _lib.load().sdx_device_count() == 0:  # valid arguments: then, and only then, the device is asked for (no CPU fallback)
        with pytest.raises(RuntimeError):
            Instrument(edges, resolving_power=5e4)


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
LAM = np.arange(6560.0, 6570.0, 0.01)


def gaussian_line(lam, depth=0.6, centre=6565.0, width=0.05):
    return 1.0 - depth * np.exp(-0.5 * ((lam - centre) / width) ** 2)


def test_truncation_at_eight_sigma_is_below_rounding():
    rng = np.random.default_rng(11)
    flux = 1.0 + 0.1 * rng.standard_normal(LAM.size)
    edges = np.linspace(6562.0, 6568.0, 121)
    sigma = oref.sigma_of_R(edges, 5e4)
    a, b = oref.observe(LAM, flux, edges, sigma), oref.observe(LAM, flux, edges, sigma, truncated=False)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    err = np.max(np.abs(a - b) / np.abs(b))
    print(f"truncated against untruncated: {err:.2e}")
    assert err <= 1e-13


def test_equivalent_width_is_conserved():
    depth, width = 0.6, 0.05
    edges = np.linspace(6562.0, 6568.0, 151)  # 0.04 A pixels; the line and 8 sigma of the line-spread function lie far inside
    out = oref.observe(LAM, gaussian_line(LAM, depth, width=width), edges, oref.sigma_of_R(edges, 5e4))
    ew = np.sum((1.0 - out) * np.diff(edges))
    exact = depth * width * np.sqrt(2 * np.pi)
    print(f"equivalent width {ew:.12f} against {exact:.12f}: {abs(ew / exact - 1):.2e}")
    assert abs(ew / exact - 1) <= 1e-8


def test_shift_moves_the_line_to_the_pixel_of_its_shifted_centre():
    edges = np.linspace(6562.01, 6568.01, 151)  # (6565 is no pixel edge: the rest-frame minimum is no tie)
    sigma = oref.sigma_of_R(edges, 5e4)
    flux = gaussian_line(LAM)
    D = oref.doppler_factor(30.0)
    rest, moved = oref.observe(LAM, flux, edges, sigma), oref.observe(LAM, flux, edges, sigma, doppler=D)
    assert int(np.argmin(rest)) == int(np.searchsorted(edges, 6565.0, "right")) - 1
    assert int(np.argmin(moved)) == int(np.searchsorted(edges, 6565.0 * D, "right")) - 1 != int(np.argmin(rest))
    # only wavelengths move: the line is as deep as it was (to the pixel phase)
    assert abs(moved.min() - rest.min()) < 0.02


def test_reference_gives_the_normalised_spectrum():
    rng = np.random.default_rng(12)
    cont = 2.0 + 0.3 * np.sin(LAM)
    flux = cont * gaussian_line(LAM) * (1 + 0.01 * rng.standard_normal(LAM.size))
    edges = np.linspace(6562.0, 6568.0, 61)
    sigma = oref.sigma_of_R(edges, 3e4)
    both = oref.observe(LAM, flux, edges, sigma, reference=cont)
    ratio = oref.observe(LAM, flux, edges, sigma) / oref.observe(LAM, cont, edges, sigma)
    assert np.max(np.abs(both - ratio) / np.abs(ratio)) <= oref.SUM_TOL
    assert np.max(np.abs(oref.observe(LAM, flux, edges, sigma, reference=flux) - 1.0)) <= oref.SUM_TOL
