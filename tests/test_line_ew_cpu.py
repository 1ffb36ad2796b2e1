"""Isolated-line equivalent widths without a GPU: the entry point is declared, exported and mirrored, a null context is refused with a
message, the Python-side validation raises before any device is asked for, the CPU restatement the GPU tests judge by
(tests/line_ew_reference.py) is what it claims to be, and curve_of_growth.solve inverts an analytic curve and the restated one."""
import ctypes
import os
import re

import numpy as np
import pytest

import line_adjoint_truth as A
import line_ew_reference as E
from conftest import ROOT
from test_response_cpu import NoDevice

from stardis_amd import _lib, curve_of_growth, ops

ENTRIES = {"sdx_line_equivalent_widths_dev": 25}


def test_entry_point_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "stardis_hip.h")).read()
    assert "r(i) = (F_B(i) - F(i)) / F_B(i)" in text and "h(i) = 1/2 (|x[i+1] - x[i]| [i+1 in U]" in text  # the definition stands above it
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        declared = [("int64_t" in a and "*" not in a and ctypes.c_int64) or ("*" in a and ctypes.c_void_p) or ctypes.c_int for a in m.group(1).split(",")]
        assert declared == list(args), name
    # the line tables stand where sdx_line_adjoint_dev has them, behind the abscissa
    assert _lib.PROTOTYPES["sdx_line_equivalent_widths_dev"][1][7:13] == _lib.PROTOTYPES["sdx_line_adjoint_dev"][1][6:12]


def test_null_context_is_refused_with_a_message():
    lib = _lib.load()
    assert lib.sdx_line_equivalent_widths_dev(None, 4, 1, None, 0, 1, None, 1, None, None, None, 4, None, 1, None, 1, None, None, 1, 1, None, None, None, None, None) == -1
    assert b"line_equivalent_widths" in lib.sdx_last_error_string() and lib.sdx_last_error_code() == -1


def test_validation_needs_no_device():
    from stardis_amd.engine import SpectralSynthesizer

    nus = np.linspace(7e14, 4e14, 5)
    ln, dw, g, al = np.array([5e14, 6e14]), np.ones((2, 4)), np.ones((2, 4)), np.ones((2, 4))
    good = dict(no_of_depth_points=4, nus=nus, line_nus=ln, doppler_widths=dw, gammas=g, alphas=al, background=np.ones((4, 5)), temperatures=np.ones(4),
                ray_distances=np.ones((3, 2)), theta_weights=np.ones(2), ctx=NoDevice())
    for kw in (dict(background=np.ones((4, 4))), dict(background=np.ones(20)), dict(gammas=np.ones((2, 3))), dict(shard=(2, 4)), dict(shard=(-1, 2)),
               dict(lines=[0, 2]), dict(lines=[-1]), dict(ln_strength=np.zeros((3, 2))), dict(ln_strength=np.zeros((2, 0))), dict(x=np.ones(4)),
               dict(temperatures=np.ones(3)), dict(ray_distances=np.ones((4, 2))), dict(lines=[1, 1, 0], ln_strength=np.zeros((2, 2)))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.equivalent_widths(**args)
    for kw in ({}, dict(lines=[1, 1, 0], ln_strength=np.zeros((3, 2))), dict(ln_strength=0.5), dict(ln_strength=[0.0, 1.0])):
        with pytest.raises(AssertionError, match="the device was asked for"):  # (a valid call does reach the context)
            ops.equivalent_widths(**dict(good, **kw))
    index, scale = ops.line_selection(3, [2, 0, 2], [0.0, np.log(2.0)])
    assert index.dtype == np.int64 and index.tolist() == [2, 0, 2] and scale.shape == (3, 2) and np.array_equal(scale[:, 0], np.ones(3))
    assert ops.line_selection(3)[0] is None and np.array_equal(ops.line_selection(3)[1], np.ones((3, 1)))

    syn = object.__new__(SpectralSynthesizer)
    syn.ctx, syn.n_depth, syn.count, syn.n_lines, syn._has_continuum, syn._ew = NoDevice(), 4, 6, 2, False, None
    with pytest.raises(ValueError, match="continuum="):
        syn.equivalent_widths()
    with pytest.raises(ValueError, match="lines"):
        syn.equivalent_widths(lines=[2], background=np.ones((4, 6)))
    with pytest.raises(ValueError, match="continuum="):
        syn.fit_equivalent_widths(np.ones(2))


@pytest.mark.parametrize("name, n_theta, lines", [("odd", 1, None), ("inner", 4, None), ("small", 4, (0, 7, 19, 33)), ("ragged", 20, (0, 5))])
def test_restatement(name, n_theta, lines):
    """the fp64 restatement stays far inside the judge (so the bound is the kernels' to use), the depths span what the docstring says, and
    the shards of a restated width add to the whole"""
    m = A.model(name)
    r = E.restated(name, n_theta, lines)
    ratio_W = np.abs(r.W64.astype(E.L) - r.W80).astype(np.float64) / r.bound_W
    ratio_d = np.abs(r.depth64.astype(E.L) - r.depth80).astype(np.float64) / r.bound_depth
    print(f"{name} at {n_theta} angles: fp64 restatement over its bound: W {ratio_W.max():.3e}, depth {ratio_d.max():.3e}; depths "
          f"{r.depth64.min():.2e} .. {r.depth64.max():.2e}; points {r.points.min()} .. {r.points.max()}")
    assert (ratio_W <= 0.25).all() and (ratio_d <= 0.25).all()
    assert (r.W64 > 0).all() and (r.depth64 > 1e-12).all() and (r.depth64 < 0.7).all()
    assert (np.diff(r.W64, axis=1) > 0).all()  # stronger is wider
    if name == "inner":  # the multi-segment path: unions of more than 4096 points that begin and end inside the grid
        inside = [(it.uhi - it.ulo > 4096) and it.ulo > 0 and it.uhi < m.n_nu for it in (E.item(name, n_theta, l, 1.0) for l in range(m.n_lines))]
        assert sum(inside) >= 3
    cuts = [0, m.n_nu // 3, m.n_nu // 3 + 1, (2 * m.n_nu) // 3, m.n_nu]
    parts = [E.restated(name, n_theta, lines, shard=(b, e - b)) for b, e in zip(cuts[:-1], cuts[1:])]
    total = sum(p.W64 for p in parts)
    assert (np.abs(total - r.W64) <= 8 * r.points * 2.0**-53 * r.terms).all()
    assert np.array_equal(np.max([np.where(p.points > 0, p.depth64, -np.inf) for p in parts], axis=0), r.depth64)
    assert sum(p.points for p in parts).tolist() == r.points.tolist()


def test_a_line_without_strength_is_exactly_zero():
    m = A.model("odd")
    saved = m.lines["alphas"][2].copy()
    try:
        m.lines["alphas"][2] = 0.0
        E.item.cache_clear()
        r = E.restated("odd", 1, [2], (1.0, 10.0))
        assert np.array_equal(r.W64, np.zeros((1, 2))) and np.array_equal(r.depth64, np.zeros((1, 2)))
        assert (r.points == 20).all()  # the floor window still stands
    finally:
        m.lines["alphas"][2] = saved
        E.item.cache_clear()


def test_solve_on_an_analytic_curve():
    true = np.array([-1.7, -0.3, 0.0, 0.9, 1.99])
    calls = []

    def evaluate(ln_s):
        calls.append(ln_s.shape)
        s = np.exp(ln_s)
        return s / np.sqrt(1.0 + s)

    s_true = 10.0**true
    W_obs = s_true / np.sqrt(1.0 + s_true)
    sol = curve_of_growth.solve(evaluate, W_obs)
    print("analytic curve: recovered - true (dex)", sol.delta_log_gf - true, "passes", len(calls) - 1)
    assert sol.converged.all() and (np.abs(sol.delta_log_gf - true) <= 1e-3).all()
    assert ((sol.bracket[:, 0] <= sol.delta_log_gf) & (sol.delta_log_gf <= sol.bracket[:, 1])).all()
    assert ((sol.bracket[:, 0] <= true) & (true <= sol.bracket[:, 1])).all() and (sol.bracket[:, 1] - sol.bracket[:, 0] < 1e-3).all()
    assert (np.abs(sol.W / W_obs - 1) <= 1e-5).all()
    assert all(shape == (5, 5) for shape in calls[:-1]) and calls[-1] == (5, 1) and len(calls) <= 9
    # outside the span, above and below; a curve that is not monotone
    out = curve_of_growth.solve(evaluate, np.array([W_obs[1], 1e3, 1e-9]))
    assert out.converged.tolist() == [True, False, False] and np.isnan(out.delta_log_gf[1:]).all()
    assert not curve_of_growth.solve(lambda ln_s: np.sin(3 * ln_s) + 2, np.array([2.0])).converged[0]
    with pytest.raises(ValueError):
        curve_of_growth.solve(evaluate, W_obs, points=1)


def test_solve_on_the_restated_curve():
    """W_obs from the restatement of `odd` at seeded offsets: every offset comes back inside its reported bracket"""
    lines = [0, 3, 6]
    rng = np.random.default_rng(5)
    true = rng.uniform(-1.0, 1.0, len(lines))

    def evaluate(ln_s):
        return np.stack([E.restated("odd", 1, [l], tuple(np.exp(ln_s[j]))).W64[0] for j, l in enumerate(lines)])

    W_obs = evaluate((true * curve_of_growth.LN10)[:, None])[:, 0]
    sol = curve_of_growth.solve(evaluate, W_obs, points=4, tol=2e-2)
    print("restated curve of odd: recovered - true (dex)", sol.delta_log_gf - true, "brackets", sol.bracket.tolist())
    assert sol.converged.all()
    assert ((sol.bracket[:, 0] <= sol.delta_log_gf) & (sol.delta_log_gf <= sol.bracket[:, 1])).all()
    assert ((sol.bracket[:, 0] <= true) & (true <= sol.bracket[:, 1])).all() and (np.abs(sol.delta_log_gf - true) <= 2e-2).all()
    far = curve_of_growth.solve(evaluate, W_obs * 1e6, points=4, tol=2e-2)
    assert not far.converged.any()
