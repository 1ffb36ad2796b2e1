"""k_raytrace_seg_step after the flux sum's 128-bit form, read off the gfx950 assembly and the compiler's resource remarks (hipcc
cross-compiles without a GPU).  Recorded (printed) for <8, 7, 2, true>: instructions, vector and scalar, VGPRs, spills, waves per SIMD,
against the parent commit's 1902 instructions (1222 vector, 620 scalar), 74 VGPRs, 0 / 0 spilled, 6 waves — counted on the parent
with this file's own count, label line to the end of the function: one branch lies behind the s_endpgm, up to which
test_step_raytrace_resources_cpu.py counts 1901 (the figures 1830, 1175 / 596 and 76 in that file's note are older than two changes
of the per-gap step).  Asserted: no scratch, no spilled vector or
scalar register in any instantiation, six waves per SIMD or more, and not more instructions than the parent.  A kernel with two flux
forms is LONGER in the file than its parent unless the rest pays for the second form; what a wave executes is the counters' business
(profiles/EXPERIMENTS.md)."""
import os
import re
import subprocess

import pytest

from test_rt_scalar_budget_cpu import CSRC, HIPCC, demangle, kernel_metadata, makefile_flags

STEP = [f"k_raytrace_seg_step<8, 7, {p}, {k}>" for p in (0, 2, 3) for k in ("false", "true")]
FLAGSHIP = "k_raytrace_seg_step<8, 7, 2, true>"
PARENT = dict(instructions=1902, vector=1222, scalar=620, vgpr_count=74, vgpr_spill_count=0, sgpr_spill_count=0, occupancy=6)


def function_bodies(text):
    """demangled kernel name -> its text from the label line to the end of the function (a kernel may end in the middle of its text:
    blocks laid out behind the s_endpgm are counted too)"""
    return {demangle(m.group(1)): m.group(2) for m in re.finditer(r"^(_ZN3sdx\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)}


def instructions(body):
    ins = [line.split()[0] for line in body.splitlines() if re.match(r"^\s+[a-z]\w*\s", line + " ") and not line.strip().startswith(";")]
    return [i for i in ins if i != "s_endpgm"]


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
    return function_bodies(text), kernel_metadata(text), occupancy


def test_every_instantiation_keeps_the_limits(build):
    _, meta, occupancy = build
    for k in STEP:
        assert k in meta and k in occupancy, sorted(n for n in meta if "raytrace_seg" in n)
        print(k, {f: meta[k][f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}, "occupancy", occupancy[k])
        assert meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
        assert occupancy[k] >= 6, (k, occupancy[k])


def test_flagship_instantiation_is_not_longer_than_the_parents(build):
    bodies, meta, occupancy = build
    ins = instructions(bodies[FLAGSHIP])
    now = dict(instructions=len(ins), vector=sum(i.startswith("v_") for i in ins), scalar=sum(i.startswith("s_") for i in ins),
               vgpr_count=meta[FLAGSHIP]["vgpr_count"], vgpr_spill_count=meta[FLAGSHIP]["vgpr_spill_count"],
               sgpr_spill_count=meta[FLAGSHIP]["sgpr_spill_count"], occupancy=occupancy[FLAGSHIP])
    print(FLAGSHIP, "parent", PARENT)
    print(FLAGSHIP, "now   ", now)
    assert len(ins) > 1000  # (the count is of instructions, not of an empty match)
    assert now["instructions"] <= PARENT["instructions"], (now, PARENT)
