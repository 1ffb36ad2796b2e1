"""Scalar-unit budget of the segmented formal solution, read off the gfx950 assembly (hipcc cross-compiles without a GPU).

A `v_fma_f64` may name one SGPR pair as an operand but no 64-bit literal, so every double constant of the per-gap step reaches the
vector unit through scalar registers.  Left as literals the compiler forms them again before every use (`s_mov_b32 sN, 0x...`, a
pair per constant): k_raytrace_seg<8,7> carried 294 such moves, 24 - 30 per gap next to ~58 vector instructions.  The kernel now
pins them once per wave (RtConst / rt_const_resident, sdx_math.h).

The cap of 175 is the count a build reached with the nine Horner coefficients of exp_neg alone pinned; it is a condition, not a
measurement of this tree.  With all fifteen constants pinned (log2 e, the two parts of ln 2, 5e-4, 64 and 1/3 as well) this tree
has 98: none in any per-gap block, the rest in Planck staging, the two reference (redo) forms and the pinning itself
(profiles/EXPERIMENTS.md).
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "stardis_amd", "csrc")
LITERAL_MOVE = re.compile(r"^\s*s_mov_b(?:32|64)\s+[^,]+,\s*0x[0-9a-fA-F]{5,}\b")
LITERAL_MOVE_CAP = 175


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^FLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "stardis_hip.s")
    proc = subprocess.run([HIPCC, "--offload-arch=gfx950", *makefile_flags(), "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "stardis_hip.hip")], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return open(out).read()


def demangle(name):
    filt = shutil.which("c++filt")
    text = subprocess.run([filt, name], capture_output=True, text=True).stdout if filt else name
    return text.split("(")[0].replace("void ", "").replace("sdx::", "").strip()


def kernel_bodies(text):
    """demangled kernel name -> its instructions (label line to s_endpgm)"""
    return {demangle(m.group(1)): m.group(2) for m in re.finditer(r"^(_ZN3sdx\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}


def kernel_metadata(text):
    """demangled kernel name -> {field: int} from the code object's metadata"""
    table = {}
    for m in re.finditer(r"^\s+\.name:\s+(_ZN3sdx\w+)\n(.*?)^\s+\.wavefront_size:", text, re.S | re.M):
        table[demangle(m.group(1))] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", m.group(2), re.M)}
    return table


def test_segmented_raytrace_literal_moves(assembly):
    bodies = kernel_bodies(assembly)
    assert "k_raytrace_seg<8, 7>" in bodies, sorted(bodies)
    moves = [line for line in bodies["k_raytrace_seg<8, 7>"].splitlines() if LITERAL_MOVE.match(line)]
    print("k_raytrace_seg<8, 7>: scalar moves of a literal:", len(moves))
    assert 0 < len(moves) <= LITERAL_MOVE_CAP, len(moves)


def test_formal_solution_kernels_keep_registers_out_of_scratch(assembly):
    meta = kernel_metadata(assembly)
    for k in ("k_raytrace_seg<8, 7>", "k_raytrace", "k_raytrace_cont"):
        assert k in meta, sorted(meta)
        print(k, {f: meta[k][f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0, (k, meta[k])
