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


def test_the_largest_planned_request_still_fits_two_blocks_per_cu(resources):  # noqa: F811
    """static LDS (the compiler's figure) plus the largest dynamic request a planned launch can make — the last level count the tiles
    take, with the bound-free edges behind the factors: 55 248 bytes, above the 48 KiB the host's gate compares the unplanned tile with
    (tests/test_continuum_truth_cpu.py) — is within the 80 KiB of two blocks per CU; so is the unplanned worst case."""
    import continuum_truth as T

    n = T.largest_tiled_level_count(0)
    for name in PLANNED:
        assert resources[name]["lds"] + T.planned_bytes(n) <= 80 * 1024, (name, resources[name])
    for name in resources:
        if name.startswith("k_prepass_continuum<") and not name.endswith("true>"):
            assert resources[name]["lds"] + T.TILE_LDS_GATE <= 80 * 1024, (name, resources[name])


def test_the_unplanned_twins_are_still_there(resources):  # noqa: F811
    for name in PLANNED:
        assert name.replace("true>", "false>") in resources, sorted(resources)


def test_the_build_launch_does_not_spill(resources):  # noqa: F811
    r = resources["k_grid_plan_build"]
    assert r["spill"] == 0 and r["occ"] == 8, r
