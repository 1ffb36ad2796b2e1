"""The contribution-function entry points at build time: declared in the header, exported by the built library, mirrored in
_lib.PROTOTYPES with matching argument counts; k_contribution compiles for gfx950 without spilled vector registers at the figures
DESIGN.md section 4 records; the formal-solution kernels beside it keep theirs; without a device the Python entry points raise."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib

ENTRIES = {"sdx_contribution_dev": 14, "sdx_formation_mean_dev": 7, "sdx_contribution_f64": 11}


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
    # not new fields of the options struct: it still ends with the continuum pair
    assert [n for n, _ in _lib.SynthesisOptions._fields_][-2:] == ["F_nu_continuum", "continuum_ld"]


def test_contribution_kernel_resources(resources):  # noqa: F811
    k = resources["k_contribution"]
    assert k["spill"] == 0, k
    # what the compiler gives: 60 VGPRs, eight waves per SIMD; the LDS is dynamic (the launch sizes it:
    # k_raytrace's budget, 21 KB per block at 56 depths x 20 angles)
    assert (k["vgpr"], k["occ"], k["lds"]) == (60, 8, 0), k
    assert any(n.endswith("k_formation_mean") for n in resources)
    # one angle per lane and no other variant: more than 64 angles are refused
    assert not any(n.startswith("k_contribution") and n != "k_contribution" for n in resources)


def test_formal_solution_kernels_keep_their_figures(resources):  # noqa: F811
    assert {k: resources["k_raytrace"][k] for k in ("vgpr", "spill", "occ")} == {"vgpr": 71, "spill": 0, "occ": 7}
    # (77 since the flagged wave's replay keeps the fast pass's coefficients in the lanes that did not raise the flag; 79 before)
    assert {k: resources["k_raytrace_seg<8, 7>"][k] for k in ("vgpr", "spill", "occ")} == {"vgpr": 77, "spill": 0, "occ": 6}
    assert resources["k_raytrace_cont"]["spill"] == 0 and resources["k_raytrace_cont"]["occ"] == 5


def test_entry_points_fail_loudly():
    """Without a device the Python entry points raise (no CPU fallback, tests/test_abi_cpu.py's rule); the C entry points refuse a null
    context with SDX_ERR_ARG and a message, with or without one."""
    lib = _lib.load()
    assert lib.sdx_contribution_dev(None, 3, 0, 1, None, None, None, None, None, 0, None, 0, None, 0) == -1
    assert b"contribution" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_formation_mean_dev(None, 3, 0, None, 0, None, None) == -1
    assert lib.sdx_contribution_f64(None, 3, 0, 1, None, None, None, None, None, None, None) == -1
    if lib.sdx_device_count() > 0:
        return  # (a GPU is visible: what the entry points compute there is tests/test_gpu_contribution.py's business)
    from stardis_amd import ops
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    with pytest.raises(RuntimeError):
        ops.contribution_arrays(np.array([2.0, 1.0]), np.ones(3), np.ones((2, 1)), np.ones(1), np.ones((3, 2)))
    with pytest.raises(RuntimeError):
        ops.formation_mean(np.ones((3, 2)), np.ones(3))
    with pytest.raises(RuntimeError):
        rfs.formation_mean(type("F", (), {"contribution_function": np.ones((3, 2))})(), np.ones(3))
