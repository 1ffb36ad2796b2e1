"""The continuum-flux option at build time: the C struct and its ctypes mirror end with the two new fields, and the continuum
formal-solution kernel k_raytrace_cont compiles without spilled vector registers at the occupancy DESIGN.md gives for them, while the resource
figures of k_raytrace and k_raytrace_seg<8, 7> stay where they were."""
import os
import re

from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib


def test_options_struct_ends_with_the_continuum_fields():
    names = [n for n, _ in _lib.SynthesisOptions._fields_]
    assert names[-2:] == ["F_nu_continuum", "continuum_ld"]
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    body = re.search(r"typedef struct sdx_synthesis_options \{(.*?)\} sdx_synthesis_options;", text, re.S).group(1)
    fields = [re.sub(r"\[.*\]", "", line.split("/*")[0]).strip().rstrip(";").split()[-1].lstrip("*")
              for line in body.splitlines() if line.split("/*")[0].strip()]
    assert fields[-2:] == ["F_nu_continuum", "continuum_ld"]
    assert "sdx_divide_dev" in _lib.PROTOTYPES


def test_continuum_kernel_does_not_spill(resources):  # noqa: F811
    cont = resources["k_raytrace_cont"]
    assert cont["spill"] == 0, cont
    # five waves per SIMD: what its 31.5 KB of LDS per block at S-c3 allows too
    assert cont["occ"] == 5, cont
    # (the small grids trace the continuum with a second k_raytrace_seg launch: the fused segmented kernel measured slower)
    assert not any(k.startswith("k_raytrace_seg_cont") for k in resources)


def test_existing_raytrace_kernels_keep_their_figures(resources):  # noqa: F811
    assert {k: resources["k_raytrace"][k] for k in ("vgpr", "spill", "occ")} == {"vgpr": 71, "spill": 0, "occ": 7}
    # (77 since the flagged wave's replay keeps the fast pass's coefficients in the lanes that did not raise the flag; 79 before)
    assert {k: resources["k_raytrace_seg<8, 7>"][k] for k in ("vgpr", "spill", "occ")} == {"vgpr": 77, "spill": 0, "occ": 6}
