"""The head of a line-kernel wave, read off the gfx950 assembly (hipcc cross-compiles without a GPU).

Before stardis_amd/csrc/sdx_line_geom.h a narrow wave (one frequency, lane <-> depth: 7634 of the ~11 000 waves of an S-c2 launch) ran four
emulated 64-bit divisions whose operands were all launch constants before its first load, a wide wave two emulated 32-bit ones and the
tile-prefix loop.  The host now forms the launch's geometry (LineGeom) and the kernels without a far field decode their block index with
it: no division emulation — its mark is the v_rcp_iflag_f32 that seeds every one, 64-bit or 32-bit — is left between a kernel's entry and
its first vector load (the narrow role's, which comes first in the text), and the multiply-high ladders are gone with it.

Whole kernel, parent -> this tree (instructions / scalar instructions / s_mul_hi_u32 / instructions before the first global_load):
    k_line_listed<4, false, false>   3369 -> 2487 / 2122 -> 1335 / 96 -> 18 / 969 -> 256
    k_line_all<4, false, false>      3267 -> 2386 / 2076 -> 1314 / 96 -> 18 / 946 -> 245
    k_line_all<4, true, false>       2392 -> 1711 / 1522 ->  923 / 73 -> 13 / 774 -> 235
    k_line_all_mixed<4, false, false> 4132 -> 3313 / 2360 -> 1626 / 89 -> 11 / 995 -> 275
Both fp64 kernels keep 71 - 72 VGPRs (7 waves per SIMD) with no spilled VGPR and no scratch (the parent's k_line_all<4, false, false> asked
for 32 bytes of it); what is left of s_mul_hi_u32 is the walks' own index arithmetic and the two line_div.  The kernels WITH a far field
keep the decode they had (LineWords, sdx_kernels.h, says why) and are not counted here.

Tried on top and removed by its number (profiles/EXPERIMENTS.md): k_line_listed<4, false, false> with the one-frequency narrow body alone —
1520 instructions, 820 scalar, 146 before the first load, 59 spilled SGPRs instead of 80 — ran as fast as with all three bodies (35.13
against 35.24 us, spreads 0.43 and 0.23).
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "stardis_amd", "csrc")
# the line kernels that take LineGeom: every instantiation without a far field
GEOM_KERNELS = ("k_line_all<4, false, false>", "k_line_all<4, true, false>", "k_line_listed<4, false, false>", "k_line_listed<4, true, false>",
                "k_line_all_mixed<4, false, false>", "k_line_all_mixed<4, true, false>")
# scalar instructions of the whole kernel: what this tree's build gives, and the parent's figure it must undercut by at least 600
SCALAR_PINNED = {"k_line_listed<4, false, false>": (1335, 2122), "k_line_all<4, false, false>": (1314, 2076)}
INSTRUCTION = re.compile(r"^\s+([a-z][a-z_0-9]+)(\s|$)")


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^FLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()


def demangle(name):
    filt = shutil.which("c++filt")
    text = subprocess.run([filt, name], capture_output=True, text=True).stdout if filt else name
    return text.split("(")[0].replace("void ", "").replace("sdx::", "").strip()


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "stardis_hip.s")
    proc = subprocess.run([HIPCC, "--offload-arch=gfx950", *makefile_flags(), "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "stardis_hip.hip")], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module")
def kernels(assembly):
    """demangled name -> (instructions of the whole function, instructions before its first vector load from memory)"""
    table = {}
    for m in re.finditer(r"^(_ZN3sdx\w+):[^\n]*\n(.*?)^\.Lfunc_end", assembly, re.S | re.M):
        name = demangle(m.group(1))
        if not name.startswith("k_line_"):
            continue
        ops = lambda text: [i.group(1) for i in (INSTRUCTION.match(line) for line in text.splitlines()) if i]  # noqa: E731
        table[name] = (ops(m.group(2)), ops(m.group(2).split("global_load")[0]))
    return table


@pytest.fixture(scope="module")
def metadata(assembly):
    table = {}
    for m in re.finditer(r"^\s+\.name:\s+(_ZN3sdx\w+)\n(.*?)^\s+\.wavefront_size:", assembly, re.S | re.M):
        table[demangle(m.group(1))] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", m.group(2), re.M)}
    return table


def test_no_division_emulation_before_the_first_load(kernels):
    for k in GEOM_KERNELS:
        assert k in kernels, sorted(kernels)
        whole, head = kernels[k]
        seeds = sum(op.startswith("v_rcp_iflag_f32") for op in head)
        ladders = sum(op.startswith("s_mul_hi") for op in head)
        print(f"{k}: {len(head)} instructions before the first global_load, {seeds} division seeds, {ladders} s_mul_hi; whole kernel "
              f"{sum(op.startswith('v_rcp_iflag_f32') for op in whole)} seeds")
        assert len(whole) > len(head) > 0
        assert seeds == 0 and ladders <= 2, (k, seeds, ladders)  # (at most a line_div and the 64-bit offset of the narrow plane, n_depth * pld)
        assert len(head) <= 330, (k, len(head))  # the parent: 774 - 1005


def test_scalar_instruction_counts(kernels):
    for k, (pinned, parent) in SCALAR_PINNED.items():
        scalar = sum(op.startswith("s_") for op in kernels[k][0])
        print(f"{k}: {len(kernels[k][0])} instructions, {scalar} scalar (parent {parent})")
        assert scalar <= parent - 600, (k, scalar)
        assert scalar == pinned, (k, scalar)


def test_registers_occupancy_and_spills(metadata):
    for k in GEOM_KERNELS:
        assert k in metadata, sorted(metadata)
        md = metadata[k]
        fields = {f: md[f] for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(k, fields)
        waves = 512 // ((md["vgpr_count"] + 7) // 8 * 8)
        if k.startswith(("k_line_all<", "k_line_listed<")):
            assert md["vgpr_count"] <= 72 and waves >= 7, (k, fields)
        elif k.startswith("k_line_all_mixed<4"):
            assert waves >= 6, (k, fields)
        assert md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (k, fields)
