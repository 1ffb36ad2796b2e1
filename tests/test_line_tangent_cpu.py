"""The tangent of the line-opacity sum without a GPU: the ABI surface, the restatement of tests/line_tangent_reference.py against the
two adjoints' restatements (the dot identity) and against the reference's own planes, the Python-side refusals, the delegation of
chi2_joint_gradient and the registers of the new kernels.

Every figure is printed before it is asserted."""
import ctypes
import os
import re

import numpy as np
import pytest

import line_adjoint_truth as A
import line_param_truth as T
import line_tangent_reference as R
from conftest import ROOT
from test_kernel_resources_cpu import resources  # noqa: F401  (the module-scoped fixture: its `make resources` parsing)
from test_response_cpu import NoDevice

from stardis_amd import _lib, ops

ENTRIES = {"sdx_line_tangent_dev": 19, "sdx_line_tangent_f64": 16}


def test_entry_points_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    assert "k_line_tangent" in text and "ascending" in text
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
    # the line tables as the adjoints take them
    assert _lib.PROTOTYPES["sdx_line_tangent_dev"][1][:12] == _lib.PROTOTYPES["sdx_line_adjoint_dev"][1][:12]
    assert _lib.PROTOTYPES["sdx_line_tangent_f64"][1][:10] == _lib.PROTOTYPES["sdx_line_adjoint_f64"][1][:10]


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_line_tangent_dev(None, 4, 1, None, 0, 1, 1, None, None, None, 4, None, None, None, None, None, 1, None, 1) == -1
    assert b"line_tangent" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_line_tangent_f64(None, 4, 1, None, 1, None, None, None, 4, None, None, None, None, None, 1, None) == -1
    assert b"line_tangent" in lib.sdx_last_error_string()


@pytest.mark.parametrize("name", ["small", "odd"])
def test_reference_plane_is_the_transpose_of_the_restated_adjoints(name):
    """sum W d alpha = sum (a S0 + g damping + b doppler + n centre) between the plane and the per-item restatements"""
    m = A.model(name)
    s0, par = A.restated(name), T.restated(name)
    for per_depth in (False, True):
        dirs = R.directions(name, per_depth)
        ref = R.plane(name, **dirs)
        item = {k: R.per_item(m, v) for k, v in dirs.items()}
        left = float((m.W.astype(R.LD) * ref.value).sum())
        left_bound = float((np.abs(m.W) * A.bound(ref.scale, ref.n_cover)).sum())
        right, right_bound = R.LD(0), 0.0
        for key, q in (("strength", s0), ("damping", par.damping), ("doppler", par.doppler), ("centre", par.centre)):
            right += (item[key].astype(R.LD) * q.s_ld).sum()
            right_bound += float((np.abs(item[key]) * A.bound(q.scale_ld, q.terms_ld)).sum())
        diff = abs(left - float(right))
        print(f"{name}, per_depth={per_depth}: plane {left:.6e}, items {float(right):.6e}, |difference| {diff:.2e}, "
              f"bounds {left_bound:.2e} + {right_bound:.2e}: ratio {diff / (left_bound + right_bound):.2e}")
        assert np.isfinite(left) and left != 0.0
        assert diff <= left_bound + right_bound


@pytest.mark.parametrize("name", ["small", "odd"])
def test_reference_strength_one_is_the_sum_of_the_lines_own_planes(name):
    ref = R.plane(name, strength=1.0)
    own = A.planes(name).sum(axis=0)
    ratio = R.worst_ratio(own, ref)
    print(f"{name}: sum of the reference's one-line planes against the plane along strength = 1: worst |difference| / bound {ratio:.2e}")
    assert ratio <= 1.0
    assert np.array_equal(ref.n_cover > 0, own != 0)
    # a mask: only the masked lines' terms, and nothing where only the others cover
    mask = R.species_mask(name)
    part = R.plane(name, strength=mask)
    ratio = R.worst_ratio(A.planes(name)[mask == 1].sum(axis=0), part)
    only_others = (part.scale == 0) & (ref.scale > 0)
    print(f"{name}: the same for a 0 / 1 mask of {int(mask.sum())} lines: {ratio:.2e}; {int(only_others.sum())} elements only the other lines cover")
    assert ratio <= 1.0 and 0 < mask.sum() < mask.size
    if name == "small":
        assert only_others.any()


def test_validation_needs_no_device():
    from stardis_amd.engine import SpectralSynthesizer

    nus = np.linspace(7e14, 4e14, 5)
    ln, dw, g, al = np.array([5e14, 6e14]), np.ones((2, 4)), np.ones((2, 4)), np.ones((2, 4))
    good = dict(no_of_depth_points=4, nus=nus, line_nus=ln, doppler_widths=dw, gammas=g, alphas=al, strength=np.ones(2),
                ctx=NoDevice())
    for kw in (dict(strength=None), dict(strength=np.ones(3)), dict(damping=np.ones((2, 3))), dict(centre=np.ones((4, 2))), dict(doppler=np.ones((2, 4, 1))),
               dict(gammas=np.ones((2, 3))), dict(shard=(2, 4)), dict(shard=(-1, 2))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.line_tangent(**args)
    with pytest.raises(AssertionError, match="the device was asked for"):  # (a valid call does reach the context)
        ops.line_tangent(**good)
    dirs, cols = ops.line_directions(2, 4, strength=2.0, doppler=np.ones((2, 4)))
    assert cols == 4 and dirs[1] is None and dirs[3] is None and dirs[0].shape == (2, 4) and (dirs[0] == 2.0).all() and dirs[0].flags.c_contiguous
    dirs, cols = ops.line_directions(2, 4, centre=[1.0, 2.0])
    assert cols == 1 and dirs[3].shape == (2, 1)

    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.keep_response, syn.n_depth, syn.count, syn.n_lines, syn.instrument = NoDevice(), True, 4, 6, 2, None
    for ask in (lambda: syn.line_tangent(), lambda: syn.line_tangent(strength=np.ones(3)), lambda: syn.flux_tangent(damping=np.ones((2, 5))),
                lambda: syn.flux_tangent()):
        with pytest.raises(ValueError, match="direction"):
            ask()
    with pytest.raises(RuntimeError, match="no instrument"):
        syn.observed_line_jacobian({"fe": dict(strength=np.ones(2))})
    with pytest.raises(RuntimeError, match="no instrument"):
        syn.chi2_joint_gradient(np.zeros(3), np.ones(3), line_directions={"fe": dict(strength=np.ones(2))})
    syn.keep_response = False
    for ask in (lambda: syn.flux_tangent(strength=np.ones(2)), lambda: syn.microturbulence_tangent(1e5), lambda: syn.microturbulence_tangent(0.0)):
        with pytest.raises(RuntimeError, match="keep_response=True"):
            ask()
    syn.instrument = object()
    with pytest.raises(RuntimeError, match="keep_response=True"):
        syn.observed_line_jacobian({"fe": dict(strength=np.ones(2))})


def test_joint_gradient_without_line_directions_is_the_instrument_gradient():
    """with no line direction chi2_joint_gradient hands its arguments to chi2_instrument_gradient and returns its answer untouched"""
    from stardis_amd.engine import SpectralSynthesizer

    syn = object.__new__(SpectralSynthesizer)
    syn.ctx = NoDevice()
    seen = []
    answer = object()

    def recorder(*args):
        seen.append(args)
        return answer

    syn.chi2_instrument_gradient = recorder
    data, ivar = np.zeros(3), np.ones(3)
    assert syn.chi2_joint_gradient(data, ivar, ("v_rad", "lsf"), None, True, True) is answer
    assert syn.chi2_joint_gradient(data, ivar, instrument_wrt="v_rad", line_directions={}) is answer
    assert len(seen) == 2 and seen[0][0] is data and seen[0][1] is ivar and seen[0][2:] == (("v_rad", "lsf"), True, True)
    assert seen[1][2:] == ("v_rad", False, False)


def test_tangent_kernels_do_not_spill(resources):  # noqa: F811
    """no spilled vector registers in the new kernels; what the compiler reports is recorded in the output"""
    new = {name: v for name, v in resources.items() if name.startswith("k_line_tangent")}
    assert set(new) == {"k_line_tangent<false>", "k_line_tangent<true>", "k_line_tangent_plan", "k_line_tangent_scan", "k_line_tangent_list"}, sorted(new)
    for name, v in sorted(new.items()):
        print(f"{name}: {v['vgpr']} VGPRs, {v['spill']} spilled, LDS {v['lds']} bytes, occupancy {v['occ']} waves / SIMD")
        assert v["spill"] == 0, (name, v)
