"""The scattering adjoint without a GPU: the restatement of the definitions (tests/scattering_adjoint_reference.py) is the transpose
of the dense operator, its three response planes are the derivatives of the emergent flux of the scattering solution (Richardson
quotients in extended precision), the fp64 restatement keeps nearly all hostile columns of the judged classes, the new kernels use
no scratch, and the entry points are declared, exported, mirrored and refuse bad arguments with a message."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import formal_solution_truth as T
import response_truth as RT
import scattering_adjoint_reference as A
import scattering_reference as R
import test_gpu_scattering as F  # the forward test's shapes, grids and grid_problem: imported, not edited
from conftest import ROOT
from test_kernel_resources_cpu import HIPCC

from stardis_amd import _lib, ops

L = T.L
ENTRIES = {"sdx_mean_intensity_adjoint_dev": 18, "sdx_scatter_response_dev": 33, "sdx_mean_intensity_adjoint_f64": 13, "sdx_scatter_response_f64": 24}
needs_extended = pytest.mark.skipif(not T.EXTENDED, reason="no extended-precision long double on this host")
# The classes the GPU test judges one application in: those in which every row is opaque (ln alpha can be perturbed), less the four at
# the ends of the double range that the sdx_response_dev header puts outside the contract (tiny, underflow, huge, overflow: not in
# response_truth.CLASSES to begin with).
JUDGED = RT.OPAQUE
PER_CLASS = F.PER_CLASS


def one_application(n_depth, n_theta, z_seed=3, source_seed=5):
    """the hostile columns of a shape (the forward test's Case), a seeded z and source plane, and Lt and G of both restatements"""
    a = F.application(n_depth, n_theta, PER_CLASS, source_seed)
    if not hasattr(a, "Lt80"):
        c = a.case
        a.z = np.random.default_rng(z_seed).uniform(-1.0, 1.0, (n_depth, c.n_nu))
        for tag, dt in (("80", L), ("64", np.float64)):
            op = R.operator(c.alphas, c.ray, a.m, dt)
            Lt, G = A.transposed(op, a.z), A.gradient(op, a.z, a.source)
            for x in (Lt, G):
                x.setflags(write=False)
            setattr(a, "Lt" + tag, Lt)
            setattr(a, "G" + tag, G)
            setattr(a, "op" + tag, op)
    return a


# ---- 1. the dense transpose ------------------------------------------------------------------------------------------------------------
@needs_extended
@pytest.mark.parametrize("n,n_theta,lo,hi", F.GRIDS[:5])
def test_restated_transpose_is_the_dense_transpose(n, n_theta, lo, hi):
    """The walk against the sweeps against matrix().T @ z, both in 80-bit arithmetic: the same products summed in another order, so the
    two differ by rounding alone — (terms per row: 3 n_theta per sweep through chains of n steps) 2^-64 of the column's largest value;
    1e-16 is a thousand times that at these shapes and a millionth of any error in the formulas."""
    p = F.grid_problem(n, n_theta, lo, hi)
    alphas = p.alphas * np.random.default_rng(n).uniform(0.5, 2.0, p.alphas.shape)  # (rough columns: a, q, r of unequal gaps)
    op = R.operator(alphas, p.ray, p.m, L)
    z = np.random.default_rng(n + 1).uniform(-1.0, 1.0, (n, p.n_nu)).astype(L)
    dense = np.einsum("kji,ki->ji", op.matrix(), z)
    walk = A.transposed(op, z)
    d = T.distance(walk, dense, np.ones(walk.shape, dtype=bool))
    print(n, n_theta, d)
    assert (d <= 1e-16).all()
    # and the dot identity z . (Lambda x) = (Lambda^T z) . x
    x = np.random.default_rng(n + 2).uniform(0.5, 2.0, (n, p.n_nu)).astype(L)
    lhs, rhs = (z * op.J(x)).sum(axis=0), (walk * x).sum(axis=0)
    assert (np.abs(lhs - rhs) <= 1e-16 * (np.abs(z) * np.abs(op.J(x))).sum(axis=0)).all()


# ---- 2. difference quotients -----------------------------------------------------------------------------------------------------------
@needs_extended
@pytest.mark.parametrize("n,n_theta,lo,hi", F.GRIDS)
def test_responses_are_the_derivatives_of_the_scattered_flux(n, n_theta, lo, hi):
    """The 80-bit restatement against the Richardson quotient of the 80-bit direct_solve flux with step 1e-4: truncation h^4 / 30 of a
    fifth derivative (1e-17) and the quotient's rounding 2^-64 / h = 5e-16 of the flux, against the sum of |R[k] p[k]| — which the flux
    exceeds by the cancellation between layers — and the flux itself, the unit of a derivative to a relative change.  1e-10 leaves two decades and is ten decades
    below an error in a formula.  The fp64 restatement's gap against its own fp64 quotient with step 1e-2, the forward solve iterated to
    tol = 1e-13 — the procedure of the GPU test, whose quotient no fp64 evaluation can form to the 80-bit gap — is printed: it is that
    test's yardstick (scattering_adjoint_reference.restated_gaps)."""
    p = F.grid_problem(n, n_theta, lo, hi)
    key = (n, n_theta, lo, hi)
    truth = A.restated_gaps(p, key, L, A.H_TRUTH)
    yard = A.restated_gaps(p, key, np.float64, A.H_DEVICE, tol=A.TOL_DEVICE)
    for name in A.QUANTITIES:
        print(f"{n}/{n_theta} {name}: 80-bit gap {truth[name]}  fp64 gap at h = {A.H_DEVICE} {yard[name]}")
    for name in A.QUANTITIES:
        assert (truth[name] <= 1e-10).all(), (name, truth[name])


# ---- 3. how many columns the restatement leaves out ------------------------------------------------------------------------------------
@needs_extended
@pytest.mark.parametrize("n_depth,n_theta,n_nu", F.SHAPES)
def test_few_columns_are_excluded(n_depth, n_theta, n_nu):
    """What the GPU test drops from a judged class: columns in which the fp64 restatement is finite nowhere, or loses a value the 80-bit
    truth has.  (No column of a Case lies near a threshold of the weights: hostile_columns draws those again.)"""
    a = one_application(n_depth, n_theta)
    c = a.case
    assert not T.near_threshold(c.alphas, c.ray).any()
    for key in ("Lt", "G"):
        truth, restated = getattr(a, key + "80"), getattr(a, key + "64")
        lost = ~np.isfinite(restated).any(axis=0) | (np.isfinite(truth) & ~np.isfinite(restated)).any(axis=0)
        for name in JUDGED:
            print(key, n_depth, n_theta, name, lost[c.columns(name)].mean())
            assert lost[c.columns(name)].mean() <= RT.EXCLUDED_AT_MOST, (key, name)


# ---- 4. resources ----------------------------------------------------------------------------------------------------------------------
def test_the_kernels_use_no_scratch():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    proc = subprocess.run(["make", "-C", os.path.join(ROOT, "stardis_amd", "csrc"), "resources"], capture_output=True, text=True, timeout=900)
    text = proc.stdout + proc.stderr
    assert "Function Name" in text, text[-2000:]
    cur, table = None, {}
    for line in text.splitlines():
        if "Function Name:" in line:
            cur = line.split("Function Name:")[1].split()[0]
            table[cur] = {}
        for key in ("VGPRs:", "VGPRs Spill:", "ScratchSize [bytes/lane]:", "LDS Size [bytes/block]:"):
            if cur and key in line:
                table[cur][key] = int(line.split(key)[1].split()[0])
    family = {k: v for k, v in table.items() if "16k_lambda_adjointILb" in k}
    print(family)
    assert len(family) == 2
    for k, v in family.items():
        assert v["ScratchSize [bytes/lane]:"] == 0 and v["VGPRs Spill:"] == 0 and v["LDS Size [bytes/block]:"] == 0 and v["VGPRs:"] <= 512, (k, v)
    # k_lambda, k_response keep their figures' names: the new family is none of theirs
    assert sum("8k_lambdaILb" in k for k in table) == 2 and sum("10k_responseE" in k for k in table) == 1
    record = open(os.path.join(ROOT, "profiles", "scattering_adjoint_resources.txt")).read()
    for v in family.values():
        assert f"VGPRs: {v['VGPRs:']}" in record


# ---- 5. the ABI and the validation -----------------------------------------------------------------------------------------------------
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
        declared = [("int64_t" in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ("double" in a and ctypes.c_double) or ctypes.c_int
                    for a in m.group(1).split(",")]
        assert declared == list(args), name
    header = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    assert "(n_theta + 10) n_depth + 3 n_theta" in header and "not of the truncated" in header


def test_null_context_and_bad_loop_arguments_are_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_mean_intensity_adjoint_dev(None, 4, 1, 1, None, None, None, None, None, 1, None, 1, None, 0, None, 0, None, 0) == -1
    assert b"mean_intensity_adjoint" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1
    assert lib.sdx_scatter_response_dev(None, 4, 1, 1, None, None, None, None, None, 1, None, 0, None, 0, None, 1, None, 1, None, 0, 1e-12, 10, None, 0, None, 0,
                                        None, 0, None, 0, None, None, None) == -1
    assert b"scatter_response" in lib.sdx_last_error_string()
    assert lib.sdx_mean_intensity_adjoint_f64(None, 4, 1, 1, None, None, None, None, None, None, None, None, None) == -1
    assert lib.sdx_scatter_response_f64(None, 4, 1, 1, None, None, None, None, None, None, 0, None, None, None, None, 1e-12, 10, None, None, None, None, None,
                                        None, None) == -1


class NoDevice:
    """a context that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_validation_needs_no_device():
    from stardis_amd.radiation_field import radiation_field_solvers as rfs

    with pytest.raises(NotImplementedError, match="plane-parallel"):
        rfs.scattering_response(types.SimpleNamespace(spherical=True), None)
    nus, temps, m = np.linspace(7e14, 4e14, 5), np.linspace(4000.0, 9000.0, 4), np.array([0.25, 0.25])
    ray, plane = np.ones((3, 2)), np.ones((4, 5))
    base = dict(tracing_nus=nus, temperatures=temps, ray_distances=ray, mean_weights=m, total_alphas=plane, z=plane, ctx=NoDevice())
    for kw in (dict(ray_distances=np.ones((3, 3))), dict(total_alphas=np.ones((4, 4))), dict(z=np.ones((4, 6))), dict(z=None), dict(source=np.ones((5, 5))),
               dict(want_Lt=False, want_G=False), dict(mean_weights=np.full(65, 1 / 130), ray_distances=np.ones((3, 65)))):
        with pytest.raises(ValueError):
            ops.mean_intensity_adjoint(**dict(base, **kw))
    del base["z"]
    base.update(alpha_scatter=np.ones(4), S=plane, cotangent=plane)
    for kw in (dict(ray_distances=np.ones((3, 3))), dict(total_alphas=np.ones((4, 4))), dict(thermal=np.ones((4, 6))), dict(S=np.ones((4, 6))), dict(S=None),
               dict(cotangent=None), dict(cotangent=np.ones((3, 5))), dict(direct=np.ones((4, 4))), dict(alpha_scatter=np.ones(5)),
               dict(alpha_scatter=np.ones((4, 4))), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=0),
               dict(mean_weights=np.full(65, 1 / 130), ray_distances=np.ones((3, 65)))):
        with pytest.raises(ValueError):
            ops.scatter_response(**dict(base, **kw))
