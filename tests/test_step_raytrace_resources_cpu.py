"""k_raytrace_seg_step at build time, read off the gfx950 assembly and the compiler's resource remarks (hipcc cross-compiles without a
GPU): every instantiation free of spilled vector registers and of scratch at six waves per SIMD or more, no more spilled scalar
registers than k_raytrace_seg<8, 7> in the same build, and — the point of the kernel — fewer instructions than it.  The general
kernel keeps its figures: 77 VGPRs (79 until the replay of a flagged wave became per lane), no spill, six waves.

This tree: k_raytrace_seg<8, 7> 2204 instructions (1319 vector, 814 scalar), 19 spilled SGPRs behind 49 v_writelane / v_readlane;
k_raytrace_seg_step<8, 7, 2, true> 1830 (1175 / 596), none spilled, 76 VGPRs (profiles/EXPERIMENTS.md)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_rt_scalar_budget_cpu import CSRC, HIPCC, demangle, kernel_bodies, kernel_metadata, makefile_flags

GENERAL = "k_raytrace_seg<8, 7>"
STEP = [f"k_raytrace_seg_step<8, 7, {p}, {k}>" for p in (0, 2, 3) for k in ("false", "true")]


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "stardis_hip.s")
    proc = subprocess.run([HIPCC, "--offload-arch=gfx950", *makefile_flags(), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                           "-o", out, os.path.join(CSRC, "stardis_hip.hip")], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    occupancy, cur = {}, None
    for line in proc.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = demangle(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur:
            occupancy[cur] = int(m.group(1))
    text = open(out).read()
    return kernel_bodies(text), kernel_metadata(text), occupancy


def instructions(body):
    return [line.split()[0] for line in body.splitlines() if re.match(r"^\s+[a-z]\w*\s", line + " ") and not line.strip().startswith(";")]


def test_step_kernels_keep_their_registers(build):
    bodies, meta, occupancy = build
    for k in STEP:
        assert k in meta and k in occupancy, sorted(n for n in meta if "raytrace_seg" in n)
        print(k, {f: meta[k][f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}, "occupancy", occupancy[k])
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert occupancy[k] >= 6, (k, occupancy[k])
        assert meta[k]["sgpr_spill_count"] <= meta[GENERAL]["sgpr_spill_count"], (k, meta[k], meta[GENERAL])


def test_step_kernel_is_shorter_than_the_general_one(build):
    bodies, _, _ = build
    general, step = instructions(bodies[GENERAL]), instructions(bodies["k_raytrace_seg_step<8, 7, 2, true>"])
    for name, ins in ((GENERAL, general), ("k_raytrace_seg_step<8, 7, 2, true>", step)):
        print(name, len(ins), "instructions:", sum(i.startswith("v_") for i in ins), "vector,", sum(i.startswith("s_") for i in ins), "scalar,",
              sum(i.startswith(("v_writelane", "v_readlane")) for i in ins), "lane moves of spilled SGPRs")
    assert len(general) > 1000  # (the count is of instructions, not of an empty match)
    assert len(step) < len(general), (len(step), len(general))


def test_general_kernel_keeps_its_figures(build):
    _, meta, occupancy = build
    assert (meta[GENERAL]["vgpr_count"], meta[GENERAL]["vgpr_spill_count"], occupancy[GENERAL]) == (77, 0, 6), (meta[GENERAL], occupancy[GENERAL])
