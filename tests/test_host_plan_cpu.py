"""The transfer plan of the host-pointer (*_f64) entry points (stardis_amd/csrc/sdx_host_plan.h) on the host, no GPU: the row tables of all
nine entries — written out below from their shapes, as stardis_hip.hip declares them — go through a stand-alone program
(tests/host_plan_probe.cpp, built here with the host compiler, under AddressSanitizer and UBSan where that links) that lays each plan
out and binds it to an arena of exactly dev_need bytes.  What comes back is compared with a model of HostIo as it stood before the plan
existed (`Before`: the bump pointer of upload / alloc, plain integer arithmetic), fed the upload / alloc sequence each entry spelled by hand.

Shapes: n_depth in {2, 5, 56} x n_nu in {1, 31, 33, 400} x n_lines in {0, 1, 7} x gamma_cols in {1, n_depth} x n_theta in {1, 3, 20},
n_pix in {0, 1, 5}, every combination of the optional outputs and inputs, the shard (7, 19) of 33 for the 2-D rows, staged and not."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

N_DEPTH = (2, 5, 56)
N_NU = (1, 31, 33, 400)
N_LINES = (0, 1, 7)
N_THETA = (1, 3, 20)
N_PIX = (0, 1, 5)
STAGING_MAX = 512 << 20
F8, I4 = 8, 4


def pad(b):
    return (b + 255) & ~255


class Before:
    """HostIo's device side as it stood: alloc() bumps by pad(bytes or 8), upload() allocates whatever the size"""

    def __init__(self):
        self.dev = 0

    def alloc(self, nbytes):
        at = self.dev
        self.dev += pad(nbytes if nbytes else 8)
        return at

    upload = alloc


def bools(n):
    return itertools.product((False, True), repeat=n)


# ---- the nine entries: (rows for the probe, the device offset each row had before — None where the entry skipped it) ---------------
# a row is (kind, present, bytes) or ("O", present, pitch, row_bytes, n_rows) or ("b", present, bytes, back) or ("s", bytes)

def line_opacity(n_depth, n_nu, n_lines, gamma_cols, null_lines=False):
    ld, plane = n_lines * n_depth * F8, n_depth * n_nu * F8
    ins = [n_nu * F8, n_lines * F8, ld, n_lines * gamma_cols * F8, ld]
    io = Before()
    before = [io.upload(b) for b in ins] + [io.alloc(plane), io.alloc(8)]
    rows = [("i", True, ins[0])] + [("i", not null_lines, b) for b in ins[1:]] + [("o", True, plane), ("o", True, 8)]
    if null_lines:  # (n_lines = 0 with null line arrays: the rows are absent now; they were empty rows of 256 bytes)
        before = None
    return rows, before


def ray_inputs(n_depth, n_nu, n_theta):
    return [n_nu * F8, n_depth * F8, (n_depth - 1) * n_theta * F8, n_theta * F8, n_depth * n_nu * F8]


def raytrace(n_depth, n_nu, n_theta, i_nus):
    plane = n_depth * n_nu * F8
    ins = ray_inputs(n_depth, n_nu, n_theta)
    io = Before()
    before = [io.upload(b) for b in ins] + [io.upload(plane), io.alloc(plane * n_theta) if i_nus else None]
    return [("i", True, b) for b in ins] + [("b", True, plane, 1), ("o", i_nus, plane * n_theta)], before


def contribution(n_depth, n_nu, n_theta, source):
    plane = n_depth * n_nu * F8
    ins = ray_inputs(n_depth, n_nu, n_theta)
    io = Before()
    before = [io.upload(b) for b in ins] + [io.upload(plane) if source else None, io.alloc(plane)]
    return [("i", True, b) for b in ins] + [("i", source, plane), ("o", True, plane)], before


def response(n_depth, n_nu, n_theta, source, r_alpha, r_source):
    plane = n_depth * n_nu * F8
    ins = ray_inputs(n_depth, n_nu, n_theta)
    io = Before()
    before = [io.upload(b) for b in ins] + [io.upload(plane) if source else None, io.alloc(plane) if r_alpha else None, io.alloc(plane) if r_source else None]
    return [("i", True, b) for b in ins] + [("i", source, plane), ("o", r_alpha, plane), ("o", r_source, plane)], before


def line_adjoint(n_depth, n_nu, n_lines, gamma_cols, out_line, out_line_depth):
    items = n_lines * n_depth * F8
    ins = [n_nu * F8, n_lines * F8, items, n_lines * gamma_cols * F8, items, n_depth * n_nu * F8]
    io = Before()
    before = [io.upload(b) for b in ins] + [io.alloc(n_lines * F8) if out_line else None, io.alloc(items) if out_line_depth else None]
    return [("i", True, b) for b in ins] + [("o", out_line, n_lines * F8), ("o", out_line_depth, items)], before


def observe(n, n_pix, reference):
    grid = n * F8
    io = Before()
    before = [io.upload(grid), io.upload(grid), io.upload(grid) if reference else None, io.upload((n_pix + 1) * F8), io.upload(n_pix * F8), io.upload(F8),
              io.alloc(n_pix * F8)]
    rows = [("i", True, grid), ("i", True, grid), ("i", reference, grid), ("i", True, (n_pix + 1) * F8), ("i", True, n_pix * F8), ("i", True, F8),
            ("o", True, n_pix * F8)]
    return rows, before


def observe_adjoint(n, n_pix, reference, nus, w_reference):
    grid = n * F8
    ins = [grid, grid if reference else 0, grid if reference else 0, (n_pix + 1) * F8, n_pix * F8, F8, n_pix * F8, grid if nus else 0]
    io = Before()
    before = [io.upload(b) if b else None for b in ins] + [io.alloc(grid), io.alloc(grid) if w_reference else None]
    rows = [("i", True, grid), ("i", reference, grid), ("i", reference, grid), ("i", True, (n_pix + 1) * F8), ("i", n_pix > 0, n_pix * F8), ("i", True, F8),
            ("i", n_pix > 0, n_pix * F8), ("i", nus, grid), ("o", True, grid), ("o", w_reference, grid)]
    return rows, before


# the continuum's sources, each a group of host pointers that come and go together in practice; sizes (n_table, bf_n_species, bf_n_levels,
# ff_n_species) with and without empty rows
CONT_SIZES = ((40, 2, 5, 3), (1, 0, 0, 0))
CONT_GROUPS = ("table", "bf", "ff", "rayleigh", "electron")


def continuum_rows(n_depth, n_nu, sizes, have, n_levels):
    """continuum_uploads: (present, bytes) of its fourteen rows; `have` names the sources (or single pointers) whose host pointers are set"""
    n_table, bf_n_species, _, ff_n_species = sizes
    depth = n_depth * F8
    table = [("lambdas", "table", n_nu * F8), ("table_wavelength", "table", n_table * F8), ("table_sigma", "table", n_table * F8), ("table_density", "table", depth),
             ("bf_species_offsets", "bf", (bf_n_species + 1) * I4), ("bf_species_ion_number", "bf", bf_n_species * I4), ("bf_cutoff", "bf", n_levels * F8),
             ("bf_level_density", "bf", n_levels * depth), ("ff_species_ion_number", "ff", ff_n_species * I4), ("ff_number_density", "ff", ff_n_species * depth),
             ("ray_n_h", "rayleigh", depth), ("ray_n_he", "rayleigh", depth), ("ray_n_h2", "rayleigh", depth), ("electron_density", "electron", depth)]
    return [((group in have and ("-" + name) not in have), nbytes) for name, group, nbytes in table]


CONT_POINTERS = ("lambdas", "table_wavelength", "table_sigma", "table_density", "bf_species_offsets", "bf_species_ion_number", "bf_cutoff", "bf_level_density",
                 "ff_species_ion_number", "ff_number_density", "ray_n_h", "ray_n_he", "ray_n_h2", "electron_density")


def synthesize_shard(n_depth, n_nu, nu_begin, nu_count, n_lines, gamma_cols, n_theta, sizes, have, line, total, flux, evals, null_lines=False):
    ld, plane = n_lines * n_depth * F8, n_depth * nu_count * F8
    ins = [(True, n_nu * F8)] + [(not null_lines, b) for b in (n_lines * F8, ld, n_lines * gamma_cols * F8, ld)]
    ins += [(True, n_depth * F8), (True, (n_depth - 1) * n_theta * F8), (True, n_theta * F8)]
    ins += continuum_rows(n_depth, n_nu, sizes, have, sizes[2] if sizes[1] > 0 else 0)
    io = Before()
    before = [io.upload(b) if there else None for there, b in ins]
    before += [io.alloc(plane) if line else None, io.alloc(plane) if total else None, io.alloc(plane), io.alloc(8) if evals else None]
    rows = [("i", there, b) for there, b in ins]
    pitch, row = n_nu * F8, nu_count * F8
    rows += [("O", line, pitch, row, n_depth), ("O", total, pitch, row, n_depth), ("O", True, pitch, row, n_depth) if flux else ("s", plane), ("o", evals, 8)]
    return rows, before


def continuum(n_depth, n_nu, sizes, have, temperature, outs):
    """outs: (total, file, bf, ff, rayleigh, electron) requested"""
    plane = n_depth * n_nu * F8
    has_bf = "bf" in have and "-bf_cutoff" not in have and sizes[1] > 0
    ins = [(True, n_nu * F8)] + continuum_rows(n_depth, n_nu, sizes, have, sizes[2] if has_bf else 0) + [(temperature, n_depth * F8)]
    io = Before()
    before = [io.upload(b) if there else None for there, b in ins] + [io.alloc(plane) if o else None for o in outs]
    rows = [("b", True, n_nu * F8, int(outs[4]))] + [("i", there, b) for there, b in ins[1:]] + [("o", o, plane) for o in outs]
    return rows, before


def all_plans():
    """every (name, rows, offsets before) the test feeds the probe"""
    for n_depth, n_nu in itertools.product(N_DEPTH, N_NU):
        for n_lines in N_LINES:
            for gamma_cols in (1, n_depth):
                yield ("line_opacity", *line_opacity(n_depth, n_nu, n_lines, gamma_cols))
                if n_lines == 0:
                    yield ("line_opacity, null line arrays", *line_opacity(n_depth, n_nu, 0, gamma_cols, null_lines=True))
                else:
                    for out_line, out_line_depth in ((True, False), (False, True), (True, True)):
                        yield ("line_adjoint", *line_adjoint(n_depth, n_nu, n_lines, gamma_cols, out_line, out_line_depth))
                for n_theta in N_THETA:
                    for line, total, flux, evals in bools(4):
                        yield ("synthesize", *synthesize_shard(n_depth, n_nu, 0, n_nu, n_lines, gamma_cols, n_theta, CONT_SIZES[n_lines % 2], CONT_GROUPS, line, total,
                                                               flux, evals))
                        if n_nu == 33:
                            yield ("synthesize, shard", *synthesize_shard(n_depth, 33, 7, 19, n_lines, gamma_cols, n_theta, CONT_SIZES[1 - n_lines % 2], CONT_GROUPS,
                                                                          line, total, flux, evals, null_lines=n_lines == 0 and evals))
        for n_theta in N_THETA:
            for (flag,) in bools(1):
                yield ("raytrace", *raytrace(n_depth, n_nu, n_theta, flag))
                yield ("contribution", *contribution(n_depth, n_nu, n_theta, flag))
            for source, r_alpha, r_source in bools(3):
                if r_alpha or r_source:
                    yield ("response", *response(n_depth, n_nu, n_theta, source, r_alpha, r_source))
        for outs in bools(6):
            if any(outs):
                for sizes in CONT_SIZES:
                    yield ("continuum", *continuum(n_depth, n_nu, sizes, CONT_GROUPS, True, outs))
                yield ("continuum, no source", *continuum(n_depth, n_nu, CONT_SIZES[0], (), False, outs))
        for n_pix in N_PIX:  # (the instrument's grid is the synthesis's: n = n_nu, from 2 up)
            n = max(n_nu, 2)
            for reference, nus, w_reference in bools(3):
                if n_pix:
                    yield ("observe", *observe(n, n_pix, reference))
                if reference or not w_reference:
                    yield ("observe_adjoint", *observe_adjoint(n, n_pix, reference, nus, w_reference))
    # every combination of the continuum's sources, and every single pointer of them absent alone, at one shape
    for k in range(len(CONT_GROUPS) + 1):
        for have in itertools.combinations(CONT_GROUPS, k):
            for temperature in (False, True):
                for outs in bools(6):
                    if any(outs):
                        yield ("continuum, sources", *continuum(5, 33, CONT_SIZES[0], have, temperature, outs))
            for line, total, flux, evals in bools(4):
                yield ("synthesize, sources", *synthesize_shard(5, 33, 7, 19, 7, 5, 3, CONT_SIZES[0], have, line, total, flux, evals))
    for name in CONT_POINTERS:
        have = CONT_GROUPS + ("-" + name,)
        yield ("continuum, one pointer null", *continuum(5, 400, CONT_SIZES[0], have, True, (True,) * 6))
        yield ("synthesize, one pointer null", *synthesize_shard(5, 400, 0, 400, 7, 1, 3, CONT_SIZES[0], have, True, True, True, True))


def encode(rows, staging_max):
    def one(r):
        if r[0] == "s":
            return f"s {r[1]}"
        return " ".join([r[0], str(int(bool(r[1])))] + [str(int(v)) for v in r[2:]])
    return f"P {staging_max} {len(rows)}\n" + "\n".join(one(r) for r in rows) + "\n"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_plan") / "host_plan_probe")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "host_plan_probe.cpp")]
    proc = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True, timeout=300)
    sanitized = proc.returncode == 0
    if not sanitized:
        proc = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    print(f"host_plan_probe built with {cxx}, {'with' if sanitized else 'WITHOUT'} -fsanitize=address,undefined")

    def run(plans, staging_max):
        """[(dev_need, pin_need, staged, [row tuples])] of the plans' row tables"""
        text = "".join(encode(rows, staging_max) for rows in plans)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
        numbers = iter(out.stdout.split())
        got = []
        for rows in plans:
            head = [int(next(numbers)) for _ in range(3)]
            got.append((*head, [tuple(int(next(numbers)) for _ in range(9)) for _ in rows]))
        assert next(numbers, None) is None
        return got
    return run


def check(name, rows, before, got, staging):
    dev_need, pin_need, staged, out = got
    what = (name, rows, "staged" if staging else "not staged")
    assert staged == int(staging), what
    arena, ups, downs = [], [], []
    for k, (r, (present, dev_off, bound, width, up_off, down_off, n_rows, uploads, downloads)) in enumerate(zip(rows, out)):
        kind = r[0]
        there = True if kind == "s" else bool(r[1])
        nbytes = r[1] if kind == "s" else r[3] * r[4] if kind == "O" else r[2]
        assert present == int(there), what
        assert bound == dev_off, what  # the pointer the caller gets is the row's place in the arena
        if not there:  # absent: a null device pointer, no width, no copy
            assert (dev_off, width, up_off, down_off, uploads, downloads) == (-1, 0, -1, -1, 0, 0), what
            if before is not None:
                assert before[k] is None, what
            continue
        assert dev_off >= 0 and dev_off % 256 == 0 and width == pad(nbytes or 8) and width >= 256, what  # (an empty row: 256 bytes of its own)
        if before is not None:
            assert before[k] == dev_off, what
        arena.append((dev_off, dev_off + width))
        assert uploads == int(nbytes > 0 and (kind == "i" or kind == "b")), what
        assert downloads == int(nbytes > 0 and (kind in "oO" or (kind == "b" and r[3]))), what
        if kind == "O":
            pitch, row_bytes, count = r[2:]
            assert n_rows == (1 if pitch == row_bytes or count <= 1 else count), what
        else:
            assert n_rows == 1, what
        for off, copies, spans in ((up_off, uploads, ups), (down_off, downloads, downs)):
            if staging and copies:
                assert off >= 0 and off % 256 == 0, what
                spans.append((off, off + pad(nbytes)))
            else:
                assert off == -1, what
    for spans, need in ((arena, dev_need), (ups + downs, pin_need)):
        spans = sorted(spans)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), what  # pairwise disjoint
        assert need == (max(e for _, e in spans) if spans else 0), what   # the need is the end of the last row, and every row ends at or below it
    if not staging:
        assert pin_need == 0 and not ups and not downs, what
    assert not ups or not downs or max(e for _, e in ups) <= min(b for b, _ in downs), what  # uploads first, downloads behind them


PLANS = list(all_plans())


def test_the_shapes_cover_what_they_should():
    names = {p[0].split(",")[0] for p in PLANS}
    assert names == {"line_opacity", "raytrace", "contribution", "response", "line_adjoint", "observe", "observe_adjoint", "continuum", "synthesize"}
    sizes = {r[2] for _, rows, _ in PLANS for r in rows if r[0] in "io"}
    assert 0 in sizes and {248, 264} <= sizes and any(s > 256 and s % 256 == 0 for s in sizes)  # empty rows, both sides of 256, whole multiples


@pytest.mark.parametrize("staging", (True, False), ids=("staged", "not-staged"))
def test_every_entry_plan_against_the_bump_pointers_it_replaces(probe, staging):
    got = probe([rows for _, rows, _ in PLANS], STAGING_MAX if staging else 0)
    for (name, rows, before), g in zip(PLANS, got):
        check(name, rows, before, g, staging)


def test_a_call_too_large_to_stage_goes_unstaged_as_a_whole(probe):
    rows = [("i", True, 300), ("b", True, 1000, 1), ("O", True, 800, 152, 5), ("o", False, 64), ("s", 0)]
    fits, over = probe([rows, rows], pad(300) + 2 * pad(1000) + pad(760))[0], probe([rows], pad(300) + 2 * pad(1000) + pad(760) - 1)[0]
    check("at the limit", rows, None, fits, True)
    check("one byte over", rows, None, over, False)
    assert fits[1] == pad(300) + 2 * pad(1000) + pad(760) and fits[0] == over[0] == 256 * (2 + 4 + 3 + 0 + 1)
