"""What the compacted list of wide lines (context option "wide_list") relies on from `make -C stardis_amd/csrc resources`: the walk of
every line kernel — those that scan and the `k_line_listed` twins whose wide role walks the list — keeps its occupancy and spills no
vector register, and the pre-pass kernels, whose
last line block now builds the list, still fit two 1024-thread blocks per CU.  tests/test_kernel_resources_cpu.py stays the authority for
the kernels it names; this file adds the instantiations it does not."""
import pytest

from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: one compiler run for this module)

LINE_KERNELS = {
    # fp64: seven waves per SIMD without a far field, six with it (the queued walk)
    "k_line_all<4, false, false>": 7, "k_line_all<4, true, false>": 7, "k_line_all<4, false, true>": 6, "k_line_all<4, true, true>": 6,
    # the kernels whose wide role walks the list of wide lines: the same budgets
    "k_line_listed<4, false, false>": 7, "k_line_listed<4, true, false>": 7, "k_line_listed<4, false, true>": 6, "k_line_listed<4, true, true>": 6,
    # fp32-mixed, 256-point tiles
    "k_line_all_mixed<4, false, false>": 6, "k_line_all_mixed<4, true, false>": 6, "k_line_all_mixed<4, false, true>": 6,
    "k_line_all_mixed<4, true, true>": 6,
}


def test_every_line_kernel_keeps_its_occupancy_without_spills(resources):  # noqa: F811
    for name, waves in LINE_KERNELS.items():
        assert name in resources, sorted(resources)
        assert resources[name]["occ"] >= waves and resources[name]["spill"] == 0, (name, resources[name])
    # (and whatever other instantiation of these families the library ships: no spills either)
    for name in resources:
        if name.startswith(("k_line_all<", "k_line_all_mixed<", "k_line_listed<")):
            assert resources[name]["spill"] == 0, (name, resources[name])


def test_the_pre_pass_with_the_list_fits_two_blocks_per_cu(resources):  # noqa: F811
    """the kernels whose last line block builds the list (16 or 32 lines per block; the culled shapes do not contain it)"""
    pre = [k for k in resources if k.startswith(("k_line_prepass<", "k_prepass_continuum<"))]
    assert len(pre) >= 12, sorted(resources)
    for k in pre:
        r = resources[k]
        assert r["occ"] == 8 and r["vgpr"] <= 64 and r["lds"] <= 80 * 1024, (k, r)
        generating = k.startswith(("k_line_prepass<true", "k_prepass_continuum<true"))  # (their cold section parks registers: the existing test's bound)
        assert r["spill"] <= (24 if generating else 0), (k, r)
    # the counter-driven launch of culled shards is compiled without the list's tail
    for k in resources:
        if k.startswith("k_line_prepass_ticket<"):
            assert resources[k]["occ"] == 8 and resources[k]["vgpr"] <= 64, (k, resources[k])
