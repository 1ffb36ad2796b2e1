"""The per-line flux sensitivities without a GPU: the entry points are declared, exported and mirrored, a null context is refused with
a message, the kernels compile for gfx950 without spilled vector registers, the Python-side validation raises before any device is asked
for, and the CPU restatement the GPU tests judge by (tests/line_adjoint_truth.py) is what it claims to be."""
import ctypes
import os
import re

import numpy as np
import pytest

import line_adjoint_truth as A
import oracle
from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)
from test_response_cpu import NoDevice

from stardis_amd import _lib, ops

ENTRIES = {"sdx_line_adjoint_dev": 16, "sdx_line_adjoint_f64": 13, "sdx_response_weight_dev": 10}


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
        declared = [("int64_t" in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ctypes.c_int for a in m.group(1).split(",")]
        assert declared == list(args), name


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_line_adjoint_dev(None, 4, 1, None, 0, 1, 1, None, None, None, 4, None, None, 1, None, None) == -1
    assert b"line_adjoint" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_response_weight_dev(None, 4, 1, None, 1, None, 1, None, None, 1) == -1
    assert b"response_weight" in lib.sdx_last_error_string()
    assert lib.sdx_line_adjoint_f64(None, 4, 1, None, 1, None, None, None, 4, None, None, None, None) == -1
    assert b"line_adjoint" in lib.sdx_last_error_string()


def test_adjoint_kernels_do_not_spill(resources):  # noqa: F811
    adjoint = {name: v for name, v in resources.items() if name.startswith("k_line_adjoint")}
    print(sorted(adjoint))
    assert {"k_line_adjoint<4>", "k_line_adjoint<64>"} <= set(adjoint)  # four lanes per short item, a wave per long one
    assert {"k_line_adjoint_setup", "k_line_adjoint_plan", "k_line_adjoint_tiled", "k_line_adjoint_gather"} <= set(adjoint)
    assert "k_response_weight" in resources
    for name, v in list(adjoint.items()) + [("k_response_weight", resources["k_response_weight"])]:
        print(name, v)
        assert v["spill"] == 0, (name, v)
    # none of them is counted by the resource tests of the line kernels, the pre-pass or the formal solution
    for prefix in ("k_line_all<", "k_line_far<", "k_line_prepass", "k_prepass_continuum", "k_raytrace", "k_contribution"):
        assert not any(name.startswith(prefix) for name in list(adjoint) + ["k_response_weight"])


def test_validation_needs_no_device():
    from stardis_amd.engine import SpectralSynthesizer

    nus = np.linspace(7e14, 4e14, 5)
    ln, dw, g, al = np.array([5e14, 6e14]), np.ones((2, 4)), np.ones((2, 4)), np.ones((2, 4))
    good = dict(no_of_depth_points=4, tracing_nus_values=nus, line_nus=ln, doppler_widths=dw, gammas=g, alphas_array=al, weight=np.ones((4, 5)),
                ctx=NoDevice())
    for kw in (dict(weight=np.ones((4, 4))), dict(weight=np.ones((5, 4))), dict(weight=np.ones(20)), dict(gammas=np.ones((2, 3))),
               dict(shard=(2, 4)), dict(shard=(-1, 2)), dict(shard=(1, 2)), dict(doppler_widths=np.ones((2, 3)))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.line_adjoint(**args)
    with pytest.raises(AssertionError, match="the device was asked for"):  # (a valid call does reach the context)
        ops.line_adjoint(**good)

    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.keep_response, syn.n_depth, syn.count, syn.n_lines = NoDevice(), True, 4, 6, 2
    for bad in (np.zeros(5), np.zeros((4, 6)), np.zeros(7)):
        with pytest.raises(ValueError, match="weights"):
            syn.line_sensitivities(bad)
    syn.keep_response = False
    for ask in (lambda: syn.line_sensitivities(), lambda: syn.line_sensitivities(np.zeros(6), per_depth=True)):
        with pytest.raises(RuntimeError, match="keep_response=True"):
            ask()


@pytest.mark.parametrize("name", ["small", "ragged", "tiny", "odd", "long", "inner"])
def test_restatement(name):
    """The single-line planes add up to the full-list plane within 1e-15 of its maximum, every item has a positive scale, and (the two
    shapes with a mix of strengths) the list holds all three window regimes."""
    m = A.model(name)
    P = A.planes(name)
    full = oracle.calc_alan_entries(*A.line_args(m))
    worst = float(np.abs(P.sum(axis=0) - full).max() / full.max())
    r = A.restated(name)
    floor, middle, whole = A.regimes(name)
    print(f"{name}: planes against the full list {worst:.2e} of its maximum; floor-only / middle / whole-grid lines {floor.size} / {middle.size} / {whole.size}; "
          f"smallest scale {r.scale_ld.min():.3e}, longest window {int(r.terms_ld.max())}")
    assert worst <= 1e-15
    assert (r.scale_ld > 0).all() and (r.scale_l > 0).all() and (r.terms_ld > 0).all()
    lo, hi = A.windows(name)
    assert np.array_equal(P != 0, (np.arange(m.n_nu) >= lo[:, :, None]) & (np.arange(m.n_nu) < hi[:, :, None]))  # a plane is its window
    if name in ("small", "ragged"):
        assert floor.size and middle.size and whole.size
        assert (floor.size, middle.size, whole.size) == {"small": (21, 15, 12), "ragged": (22, 34, 25)}[name]
    if name == "tiny":
        assert (lo == 0).all() and (hi == m.n_nu).all()  # every window clipped at both ends
    if name == "long":
        assert whole.size and r.terms_ld.max() == m.n_nu >= 9000
    if name == "inner":  # windows of more than 4096 points (four tiles of the tiled role) that neither start nor end at an end of the grid
        inside = (hi - lo > 4096) & (lo > 0) & (hi < m.n_nu)
        assert inside.sum() >= 6 and ((lo[inside] % 1024) != 0).all() and (lo[inside] > 1024).all() and (hi - lo == 80).any()
        assert (hi < 6000).any() and (lo > 3000).any()  # some end inside, some start inside, the shard (3000, 6000) of the GPU tests
    # a shard's restatement is the sum over its columns, and an item whose window misses it has no term
    part = A.restated(name, shard=(m.n_nu // 3, m.n_nu // 3))
    assert (part.terms_ld <= r.terms_ld).all() and np.array_equal(part.terms_ld == 0, part.scale_ld == 0)
