"""Compiler figures of the equivalent-width kernels (`make -C stardis_amd/csrc resources`; hipcc cross-compiles without a GPU): the four
k_ew_* kernels are there, none of them is counted by a pinned family of tests/test_kernel_resources_cpu.py, the walk spills no vector
register and uses no scratch, and its occupancy is the one DESIGN §4 states."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_kernel_resources_cpu import HIPCC

KERNELS = ("k_ew_plan", "k_ew_scan", "k_ew_walk", "k_ew_gather")
WALK_OCCUPANCY = 3  # waves per SIMD: 136 vector registers ("Isolated-line equivalent widths")


@pytest.fixture(scope="module")
def resources():
    """{kernel: dict(vgpr, spill, occ, lds, scratch)} of the k_ew_* kernels and the names of all kernels, from one resource build"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    proc = subprocess.run(["make", "-C", os.path.join(ROOT, "stardis_amd", "csrc"), "resources"], capture_output=True, text=True, timeout=900)
    text = proc.stdout + proc.stderr
    assert "Function Name" in text, text[-2000:]
    tags = (("VGPRs:", "vgpr"), ("VGPRs Spill:", "spill"), ("Occupancy [waves/SIMD]:", "occ"), ("LDS Size [bytes/block]:", "lds"), ("ScratchSize [bytes/lane]:", "scratch"))
    cur, table = None, {}
    for line in text.splitlines():
        if "Function Name:" in line:
            mangled = line.split("Function Name:")[1].split()[0]
            cur = next((k for k in KERNELS if f"{len(k)}{k}E" in mangled), mangled)  # (plain kernels of namespace sdx: the Itanium name holds <length><name>)
            table[cur] = {}
        for key, tag in tags:
            if cur and key in line:
                table[cur][tag] = int(line.split(key)[1].split()[0])
    return table


def test_the_kernels_are_there(resources):
    family = sorted(k for k in resources if "k_ew" in k)
    print({k: resources[k] for k in family})
    assert family == sorted(KERNELS)  # (no other kernel's name holds k_ew, and none of these a pinned family's prefix)
    for prefix in ("k_raytrace", "k_contribution", "k_line_all", "k_line_listed", "k_line_far", "k_line_prepass", "k_prepass_continuum"):
        assert not any(k.startswith(prefix) for k in family)


def test_no_spills_and_no_scratch(resources):
    for k in KERNELS:
        assert resources[k]["spill"] == 0 and resources[k]["scratch"] == 0, (k, resources[k])
    assert resources["k_ew_walk"]["lds"] == 0  # no static LDS: the launch's byte count (EwColumns::bytes()) is all there is


def test_walk_occupancy_is_the_documented_one(resources):
    print("k_ew_walk", resources["k_ew_walk"])
    assert resources["k_ew_walk"]["occ"] == WALK_OCCUPANCY and resources["k_ew_walk"]["vgpr"] <= 512 // WALK_OCCUPANCY
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Isolated-line equivalent widths" in text and f"{WALK_OCCUPANCY} waves per SIMD" in text


LAYOUT_PROBE = r"""
#include "sdx_rt_layout.h"
#include <cstdio>
int main()
{
    const int shapes[][2] = {{20, 56}, {1, 3}, {20, 167}, {20, 168}, {1, 403}, {1, 404}, {64, 2}, {7, 57}, {1, 9000}};
    for (auto& s : shapes) {
        const int gpw = rt_fit_gpw<EwColumns>(s[0], s[1]);
        std::printf("%d %d %d %zu\n", s[0], s[1], gpw, gpw ? EwColumns(s[0], s[1], gpw).bytes() : (size_t)0);
    }
    return 0;
}
"""


def test_lds_bytes_are_what_the_layout_says(tmp_path):
    """the host's launch shape from EwColumns, compiled for the host alone, against the layout written out here: seven per-depth constants
    and two slots per segment point for the block; pairs, the background's square roots and one set of flux terms per chain for a wave"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(LAYOUT_PROBE)
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "stardis_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True, timeout=600)
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {(G, nd): (gpw, nbytes) for G, nd, gpw, nbytes in rows}

    def expect(G, nd):
        for gpw in range(64 // G, 0, -1):
            shared = ((7 * nd + 1) & ~1) + 2 * 256
            wave = (3 * gpw * nd + 2 * gpw * G + 1) & ~1
            if 8 * (shared + 4 * wave) <= 64 * 1024:
                return gpw, 8 * (shared + 4 * wave)
        return 0, 0

    for key, value in got.items():
        assert value == expect(*key), (key, value, expect(*key))
    assert got[(20, 56)] == (3, 8 * (392 + 512 + 4 * 624)) and got[(20, 167)][0] == 3 and got[(20, 168)][0] == 2
    assert got[(1, 403)][0] == 1 and got[(1, 404)][0] == 0 and got[(1, 9000)][0] == 0
