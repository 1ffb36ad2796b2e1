"""The response functions without a GPU: the definitions (tests/response_truth.py) are the derivative they claim to be, the restatement
alone meets the conditions the GPU tests rest on, the entry points are declared, exported and mirrored, the kernels compile for gfx950
without spilled vector registers, and the Python-side validation raises before any device is asked for.

Source identity: I is linear in S, so sum_k R_source[k] S[k] = F exactly in theory.  In 80 bits the difference is held to
8 (N_d - 1) epsilons of the flux; in double precision to the same count of epsilons of sum_k |R_source[k] S[k]| — the magnitudes a
double-precision sum passes through (in `ramp` and `everything` the coefficients q and r of neighbouring gaps reach 1e9 with opposite
signs, and the flux itself is then no measure of a sum's rounding).

Opacity derivative: R_alpha in 80 bits against Richardson-extrapolated central differences of the 80-bit flux, h = 1e-3 in ln alpha[k].
The condition |analytic - extrapolated| <= |FD(h) - FD(h/2)| is evaluated as the project evaluates every formal-solution criterion
(formal_solution_truth.per_class): per class of columns, each column's largest value over depth on the scale of its emergent flux,
the largest of the class on either side.  Element by element it cannot hold: where the flux does not depend on a row at all (below a
layer with c = 0) both differences are exactly 0 and the analytic value is 1e-30 of the flux, and near tau = 5e-4 the cancellation
of the mid-branch weights puts the 80-bit flux's own rounding, divided by h, above a truncation error that is tiny at three depth
points (measured: 4.5e-7 against 5.6e-7 of the flux in `straddle_small` at (3, 1), the closest case)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import formal_solution_truth as T
import response_truth as R
from conftest import ROOT
from test_kernel_resources_cpu import HIPCC, resources  # noqa: F401  (the module-scoped fixture: one resource build)

from stardis_amd import _lib, ops

L = T.L
needs_extended = pytest.mark.skipif(not T.EXTENDED, reason="no extended-precision long double on this host")
ENTRIES = {"sdx_response_dev": 16, "sdx_response_f64": 12, "sdx_response_project_dev": 10}
GPU_SHAPES = [(2, 1, 4), (3, 5, 4), (9, 7, 16), (56, 20, 8), (40, 64, 2)]  # tests/test_gpu_response.py
FD_SHAPES = [(3, 1), (9, 7), (24, 20)]
H = 1e-3


# ---- the definitions -------------------------------------------------------------------------------------------------------------
@needs_extended
@pytest.mark.parametrize("n_depth,n_theta", FD_SHAPES + [(2, 1), (56, 20)])
def test_source_identity(n_depth, n_theta):
    r = R.responses(n_depth, n_theta, 4)
    c = r.case
    missed = []
    for label, d, eps in (("truth", r.truth, np.finfo(L).eps), ("restatement", r.restated, np.finfo(np.float64).eps)):
        with np.errstate(all="ignore"):
            terms = d["Rs"] * d["S"]
            diff = np.abs(terms.sum(axis=0) - d["F"])
            scale = np.abs(d["F"]) if label == "truth" else np.abs(terms).sum(axis=0)
        ok = np.isfinite(diff) & np.isfinite(scale)
        assert ok[np.isin(c.cls, R.OPAQUE)].all()  # an opaque column has a value everywhere
        for name in c.classes:
            cols = c.columns(name) & ok
            if not cols.any():
                continue
            assert np.array_equal(diff[cols & (scale == 0)], np.zeros(int((cols & (scale == 0)).sum())))  # no flux: exactly none
            cols &= scale > 0
            worst = float((diff[cols] / scale[cols]).max() / eps) if cols.any() else 0.0
            print(f"{label} {n_depth}/{n_theta} {name}: {worst:.2f} eps of {8 * (n_depth - 1)}")
            if not worst <= 8 * (n_depth - 1):
                missed.append((label, name, worst))
    assert not missed, missed


def _central_differences(c, h):
    out = np.zeros((c.n_depth, c.n_nu), dtype=L)
    for k in range(c.n_depth):
        up, down = c.alphas.astype(L), c.alphas.astype(L)
        up[k] *= np.exp(L(h))
        down[k] *= np.exp(-L(h))
        out[k] = (c.truth(up)[0][-1] - c.truth(down)[0][-1]) / (2 * L(h))
    return out


@needs_extended
@pytest.mark.parametrize("n_depth,n_theta", FD_SHAPES)
def test_opacity_response_is_the_derivative_of_the_flux(n_depth, n_theta):
    r = R.responses(n_depth, n_theta, 4)
    c = r.case
    coarse, fine = _central_differences(c, H), _central_differences(c, H / 2)
    extrapolated = (4 * fine - coarse) / 3
    flux = np.abs(c.truth()[0][-1])
    with np.errstate(all="ignore"):  # (the transparent classes: not judged)
        error = np.abs(r.truth["Ra"] - extrapolated).max(axis=0) / flux
        truncation = np.abs(coarse - fine).max(axis=0) / flux
    missed = []
    for name in R.OPAQUE:
        cols = c.columns(name)
        e, b = float(error[cols].max()), float(truncation[cols].max())
        print(f"{n_depth}/{n_theta} {name}: analytic - extrapolated {e:.2e}, FD(h) - FD(h/2) {b:.2e}")
        if not e <= b:
            missed.append((name, e, b))
    assert not missed, missed


@needs_extended
@pytest.mark.parametrize("n_depth,n_theta,per_class", GPU_SHAPES)
@pytest.mark.parametrize("source_seed", [None, 5])
def test_few_columns_are_excluded(n_depth, n_theta, per_class, source_seed):
    """What the GPU tests drop from a class: columns flagged by near_threshold, and columns in which the double-precision restatement
    loses a value the definition has (not finite where the 80-bit truth is).  At most one column in eight of any class.  Where the
    definition itself has no value — the reference divides by zero above a transparent row — there is nothing to exclude."""
    for order in ("grouped", "interleaved"):
        r = R.responses(n_depth, n_theta, per_class, order, source_seed)
        c = r.case
        for key in ("Ra", "Rs"):
            lost = ~r.keep | (np.isfinite(r.truth[key]) & ~np.isfinite(r.restated[key])).any(axis=0)
            for name in c.classes:
                assert lost[c.columns(name)].mean() <= R.EXCLUDED_AT_MOST, (key, name, order)
            defined = np.isfinite(r.restated[key]).any(axis=0)
            for name in R.OPAQUE + ("leading_transparent", "transparent"):  # (no division by zero in these)
                assert defined[c.columns(name)].all(), (key, name, order)


# ---- the build ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        declared = [("int64_t" in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ctypes.c_int for a in m.group(1).split(",")]
        assert declared == list(args), name


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_response_dev(None, 4, 1, 1, None, None, None, None, None, 1, None, 0, None, 0, None, 0) == -1
    assert b"response" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_response_f64(None, 4, 1, 1, None, None, None, None, None, None, None, None) == -1
    assert lib.sdx_response_project_dev(None, 4, 1, None, 1, None, 1, None, 1, None) == -1
    assert b"response_project" in lib.sdx_last_error_string()


def test_response_kernels_do_not_spill(resources):  # noqa: F811
    for kernel in ("k_response", "k_response_project"):
        found = [v for name, v in resources.items() if name == kernel]
        assert len(found) == 1, sorted(resources)
        print(kernel, found[0])
        assert found[0]["spill"] == 0, (kernel, found[0])
        assert found[0]["lds"] == 0, (kernel, found[0])  # no static LDS: the launch's byte count (RtResponse::bytes()) is all there is


LAYOUT_PROBE = r"""
#include "sdx_rt_layout.h"
#include <cstdio>
int main()
{
    const int shapes[][2] = {{20, 56}, {1, 2}, {5, 3}, {7, 9}, {64, 40}, {64, 117}, {64, 118}, {20, 366}, {20, 367}, {1, 9000}};
    for (auto& s : shapes) {
        const int gpw = rt_fit_gpw<RtResponse>(s[0], s[1]);
        std::printf("%d %d %d %zu %u\n", s[0], s[1], gpw, gpw ? RtResponse(s[0], s[1], gpw).bytes() : (size_t)0, gpw ? response_blocks(1000, gpw) : 0u);
    }
    return 0;
}
"""


def test_lds_bytes_are_what_the_layout_says(tmp_path):
    """the host's launch shape from RtResponse (compiled for the host alone): pairs + one stashed double per (ray, gap) + two batches of
    terms per wave, one wave per workgroup; the benchmark's shape fits at three frequencies per wave; the first depth that does not fit"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(LAYOUT_PROBE)
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "stardis_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True, timeout=600)
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {(G, nd): (gpw, nbytes, blocks) for G, nd, gpw, nbytes, blocks in rows}

    def expect(G, nd):
        for gpw in range(64 // G, 0, -1):
            doubles = 2 * gpw * nd + (nd - 1) * gpw * G + 2 * 4 * gpw * G
            doubles += doubles & 1
            if 8 * doubles <= 64 * 1024:
                return gpw, 8 * doubles, -(-1000 // gpw)
        return 0, 0, 0

    for key, value in got.items():
        assert value == expect(*key), (key, value, expect(*key))
    assert got[(20, 56)][0] == 3 and got[(20, 56)][1] == 8 * (336 + 55 * 60 + 480)
    assert got[(64, 117)][0] == 1 and got[(64, 118)][0] == 0 and got[(20, 366)][0] == 1 and got[(20, 367)][0] == 0 and got[(1, 9000)][0] == 0


# ---- validation on the host -----------------------------------------------------------------------------------------------------
class NoDevice:
    """a context that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_validation_needs_no_device():
    from stardis_amd.engine import SpectralSynthesizer
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    # keep_total cannot be switched off under keep_response; the results are refused when nothing was kept
    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.keep_contribution, syn.keep_response, syn._keep_total, syn.d_total = NoDevice(), False, True, True, object()
    syn.n_depth, syn.count, syn.d_Ra, syn.d_Rs = 4, 6, object(), object()
    syn.graph = syn.graph_classify = syn.graph_batch = syn.plan = None
    with pytest.raises(ValueError, match="keep_response"):
        syn.keep_total = False
    assert syn.keep_total is True
    for bad in (np.zeros((4, 5)), np.zeros((3, 6)), np.zeros(24)):
        with pytest.raises(ValueError, match="alpha_part"):
            syn.flux_derivative(bad)
    syn.keep_response = False
    for ask in (lambda: syn.response_opacity, lambda: syn.response_source, lambda: syn.flux_derivative(np.zeros((4, 6)))):
        with pytest.raises(RuntimeError, match="keep_response=True"):
            ask()
    # a spherical model
    with pytest.raises(NotImplementedError, match="plane-parallel"):
        rfs.response_functions(types.SimpleNamespace(spherical=True), None)
    # wrong shapes
    nus, temps, w = np.linspace(7e14, 4e14, 5), np.linspace(4000.0, 9000.0, 4), np.array([0.5, 0.5])
    ray, alphas = np.ones((3, 2)), np.ones((4, 5))
    for kw in (dict(ray_distances=np.ones((3, 3))), dict(ray_distances=np.ones((2, 2))), dict(total_alphas=np.ones((4, 4))),
               dict(total_alphas=np.ones((5, 4))), dict(source=np.ones((4, 6))), dict(want_opacity=False, want_source=False)):
        args = dict(tracing_nus=nus, temperatures=temps, ray_distances=ray, theta_weights=w, total_alphas=alphas, ctx=NoDevice())
        args.update(kw)
        with pytest.raises(ValueError):
            ops.response(**args)
