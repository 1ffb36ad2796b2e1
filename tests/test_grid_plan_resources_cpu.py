"""The planned pre-pass kernels (sdx_grid_plan: k_prepass_continuum<false, LINES, true>, 16 and 32 lines per block) by name, held to
the budget of every pre-pass kernel: two 1024-thread blocks per CU — 8 waves per SIMD, at most 64 VGPRs, none spilled, at most 80 KB
of LDS (tests/test_kernel_resources_cpu.py explains the figures and stays the authority for the kernels it finds by prefix).  The
launch that builds the plan runs once per synthesizer; it must not spill either."""
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one compiler run for this module)

PLANNED = ["k_prepass_continuum<false, 16, true>", "k_prepass_continuum<false, 32, true>"]


def test_planned_pre_pass_kernels_fit_two_blocks_per_cu(resources):  # noqa: F811
    for name in PLANNED:
        assert name in resources, sorted(resources)
        r = resources[name]
        assert r["spill"] == 0 and r["occ"] == 8 and r["vgpr"] <= 64 and r["lds"] <= 80 * 1024, (name, r)


def test_the_unplanned_twins_are_still_there(resources):  # noqa: F811
    for name in PLANNED:
        assert name.replace("true>", "false>") in resources, sorted(resources)


def test_the_build_launch_does_not_spill(resources):  # noqa: F811
    r = resources["k_grid_plan_build"]
    assert r["spill"] == 0 and r["occ"] == 8, r
