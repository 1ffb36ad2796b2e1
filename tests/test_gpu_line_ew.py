"""Isolated-line equivalent widths on the device (sdx_line_equivalent_widths_dev, ops.equivalent_widths,
SpectralSynthesizer.equivalent_widths / fit_equivalent_widths).

The kernels are judged by the 80-bit restatement of tests/line_ew_reference.py (tests/test_line_ew_cpu.py checks what that rests on):
|W - W_80| <= 2 formal_solution_truth.bound(d, N_d) span + 2e-12 |W_80|, the depth likewise without the span.  Every test prints its
figures before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import formal_solution_truth as T
import line_ew_reference as E
from conftest import ROOT
from stardis_amd import _lib, curve_of_growth, ops
from stardis_amd.engine import SpectralSynthesizer
from test_gpu_response import profiled, small_model, synthesizer

pytestmark = pytest.mark.gpu

HIPCC = "/opt/rocm/bin/hipcc"
EPS = 2.0**-53


@pytest.fixture(autouse=True)
def extended_precision():
    if not T.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def widths(ctx, S, lines=None, scale=E.SCALES, shard=None, want="both", n_theta=None, n_depth=None, index_dtype=np.int64):
    """sdx_line_equivalent_widths_dev on a setup of the reference -> (W, depth) as host arrays (n_sel, K); scale: a tuple of factors for
    every line, an (n_sel, K) array, or None (the NULL pointer, K = 1)"""
    m = S.m
    Ls = m.lines
    b, n = (0, m.n_nu) if shard is None else shard
    n_sel = m.n_lines if lines is None else len(lines)
    sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (n_sel, np.shape(scale)[-1])))
    k = 1 if sc is None else sc.shape[1]
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (m.nus, S.x, Ls["line_nus"], Ls["doppler_widths"], Ls["gammas"], Ls["alphas"], S.B[:, b:b + n],
                                                      S.temps, S.ray, S.weights)]
    d_idx = None if lines is None else ctx.upload(np.asarray(lines, dtype=index_dtype), index_dtype)
    d_sc = None if sc is None else ctx.upload(sc)
    o_w = ctx.zeros((n_sel, k)) if want in ("both", "W") else None
    o_d = ctx.zeros((n_sel, k)) if want in ("both", "depth") else None
    ctx.call("sdx_line_equivalent_widths_dev", m.n_depth if n_depth is None else n_depth, m.n_nu, d[0].ptr, b, n, d[1].ptr, m.n_lines, d[2].ptr, d[3].ptr,
             d[4].ptr, Ls["gammas"].shape[1], d[5].ptr, n_sel, _lib.ptr_of(d_idx), k, _lib.ptr_of(d_sc), d[6].ptr, n, S.n_theta if n_theta is None else n_theta,
             d[7].ptr, d[8].ptr, d[9].ptr, _lib.ptr_of(o_w), _lib.ptr_of(o_d))
    ctx.synchronize()
    return (None if o_w is None else np.array(o_w.numpy())), (None if o_d is None else np.array(o_d.numpy()))


# ---- 1. against the 80-bit truth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n_theta, lines", [("odd", 1, None), ("small", 1, None), ("small", 4, None), ("small", 20, None),
                                                  ("ragged", 20, tuple(range(8))), ("inner", 4, None)])
def test_against_truth(ctx, name, n_theta, lines):
    S = E.setup(name, n_theta)
    ref = E.restated(name, n_theta, lines)
    W, depth = widths(ctx, S, lines)
    E.judge(f"{name} at {n_theta} angles", W, depth, ref)
    if name == "inner":  # the multi-segment path: unions of more than 4096 points that begin and end inside the grid
        assert ((ref.points > 4096) & (ref.points < S.m.n_nu)).sum() >= 4  # (at ten times the strength three of them take the whole grid)
    # one output at a time: the same bits
    assert np.array_equal(widths(ctx, S, lines, want="W")[0], W) and np.array_equal(widths(ctx, S, lines, want="depth")[1], depth)
    if name == "odd":  # the array-level function: lambda in Angstrom, exp(ln 1) = 1
        m = S.m
        Wo, do = ops.equivalent_widths(m.n_depth, m.nus, m.lines["line_nus"], m.lines["doppler_widths"], m.lines["gammas"], m.lines["alphas"], S.B, S.temps,
                                       S.ray, S.weights, ctx=ctx)
        assert np.array_equal(Wo[:, 0], W[:, 1]) and np.array_equal(do[:, 0], depth[:, 1])


# ---- 2. edges -----------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    S = E.setup("small", 4)
    W, depth = widths(ctx, S, scale=(0.0, 1.0))
    assert np.array_equal(W[:, 0], np.zeros(S.m.n_lines)) and np.array_equal(depth[:, 0], np.zeros(S.m.n_lines))  # no strength: exactly 0
    assert (W[:, 1] > 0).all() and (depth[:, 1] > 0).all()
    # scale = NULL is scale = 1.0
    W1, d1 = widths(ctx, S, scale=None)
    assert np.array_equal(W1[:, 0], W[:, 1]) and np.array_equal(d1[:, 0], depth[:, 1])
    # lines centred beyond either end of the grid whose windows reach in
    Se = E.setup("edge", 4)
    ref = E.restated("edge", 4)
    assert [E.item("edge", 4, l, 1.0).ulo for l in (0, 1)][1] == 0 and E.item("edge", 4, 0, 1.0).uhi == Se.m.n_nu and (ref.points >= 10).all()
    E.judge("edge", *widths(ctx, Se), ref)
    # lines wholly outside the shard
    it = [E.item("small", 4, l, 1.0) for l in range(S.m.n_lines)]
    outside = [l for l in range(S.m.n_lines) if it[l].ulo >= 60]
    assert len(outside) >= 5
    Ws, ds = widths(ctx, S, outside, scale=(1.0,), shard=(0, 60))
    assert np.array_equal(Ws, np.zeros((len(outside), 1))) and np.array_equal(ds, np.zeros((len(outside), 1)))


# ---- 3. frequency shards ------------------------------------------------------------------------------------------------------------
def test_shards_add(ctx):
    S = E.setup("small", 4)
    m = S.m
    strong = int(np.argmax(m.lines["alphas"].max(axis=1)))
    core = int(m.n_nu - np.searchsorted(m.nus[::-1], m.lines["line_nus"][strong]))  # the first point below the line's frequency
    cuts = sorted({0, 97, core, core + 1, 211, m.n_nu})
    W, depth = widths(ctx, S)
    ref = E.restated("small", 4)
    parts = [widths(ctx, S, shard=(b, e - b)) for b, e in zip(cuts[:-1], cuts[1:])]
    total = sum(p[0] for p in parts)
    error = np.abs(total - W)
    bound = ref.points * EPS * ref.terms
    print(f"shards {cuts}: worst |sum of shards - whole| / (n 2^-53 sum |h r|) = {(error / bound).max():.3e}")
    assert (error <= bound).all()
    assert np.array_equal(np.max([p[1] for p in parts], axis=0), depth)  # (every line absorbs: some r >= 0, the max is exact)
    # each shard against its own restatement
    for (b, e), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        r = E.restated("small", 4, shard=(b, e - b))
        hit = r.points > 0
        assert np.array_equal(p[0][~hit], np.zeros(int((~hit).sum()))) and np.array_equal(p[1][~hit], np.zeros(int((~hit).sum())))
        assert (np.abs(p[0].astype(E.L) - r.W80)[hit] <= r.bound_W[hit]).all() and (np.abs(p[1].astype(E.L) - r.depth80)[hit] <= r.bound_depth[hit]).all()


# ---- 4. a row depends on its own line and strength alone ----------------------------------------------------------------------------------
def test_independence(ctx):
    S = E.setup("small", 4)
    W, depth = widths(ctx, S)
    pick = [5, 3, 3, 0]
    Wp, dp = widths(ctx, S, pick)
    assert np.array_equal(Wp, W[pick]) and np.array_equal(dp, depth[pick])
    for k in range(3):
        W1, d1 = widths(ctx, S, scale=(E.SCALES[k],))
        assert np.array_equal(W1[:, 0], W[:, k]) and np.array_equal(d1[:, 0], depth[:, k])
    again = widths(ctx, S)
    assert np.array_equal(again[0], W) and np.array_equal(again[1], depth)
    # more items than the prefix sum has threads (several items per thread of k_ew_scan), in a shuffled order
    many = np.random.default_rng(3).permutation(np.tile(np.arange(S.m.n_lines), 30))
    Wm, dm = widths(ctx, S, many)
    assert many.size * 3 > 2048 and np.array_equal(Wm, W[many]) and np.array_equal(dm, depth[many])
    # strengths per line
    sc = np.array([[0.1, 10.0]] * S.m.n_lines)
    sc[::2] = [1.0, 0.1]
    W2, _ = widths(ctx, S, scale=sc)
    assert np.array_equal(W2[1::2, 0], W[1::2, 0]) and np.array_equal(W2[1::2, 1], W[1::2, 2]) and np.array_equal(W2[::2, 0], W[::2, 1])


# ---- 5. the layout: either side of the first lowered points per wave, and the refusals -----------------------------------------------
LAYOUT_PROBE = r"""
#include "sdx_rt_layout.h"
#include <cstdio>
int main()
{
    int first = 0;
    for (int nd = 2; nd < 4000 && !first; ++nd)
        if (rt_fit_gpw<EwColumns>(20, nd) < 3) first = nd;
    int deep = 0;
    for (int nd = 2; nd < 9000 && !deep; ++nd)
        if (rt_fit_gpw<EwColumns>(1, nd) == 0) deep = nd;
    std::printf("%d %d %d %d\n", first, rt_fit_gpw<EwColumns>(20, first - 1), rt_fit_gpw<EwColumns>(20, first), deep);
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """(the first depth count at which EwColumns lowers the points per wave at 20 angles, the first that fits no wave at one angle),
    from the struct itself, compiled for the host"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("ew_layout")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(LAYOUT_PROBE)
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "stardis_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True, timeout=600)
    first, before, at, deep = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert before == 3 and at == 2 and deep > first
    return first, deep


@pytest.mark.parametrize("side", [-1, 0])
def test_either_side_of_a_lowered_group(ctx, layout, side):
    n_depth = layout[0] + side
    name = f"deep{n_depth}"
    S = E.setup(name, 20)
    E.judge(f"{n_depth} depth points at 20 angles", *widths(ctx, S), E.restated(name, 20))


def refused(ctx, match, call):
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        with pytest.raises(ValueError, match=match):
            call()
        assert ctx.profile("k_line_ew")[0] == 0  # nothing was launched
    finally:
        ctx.call("sdx_profile_enable", 0)


def test_refusals_before_any_launch(ctx, layout):
    S = E.setup("odd", 1)
    m = S.m
    before = widths(ctx, S)
    refused(ctx, "n_theta <= 64", lambda: widths(ctx, S, n_theta=65))
    assert ctx.lib.sdx_last_error_code() == -1  # SDX_ERR_ARG
    refused(ctx, "models this deep", lambda: widths(ctx, S, n_depth=layout[1]))  # (the refusal comes before any pointer is read)
    refused(ctx, "n_depth >= 2", lambda: widths(ctx, S, n_depth=1))
    refused(ctx, "no output", lambda: widths(ctx, S, want="none"))
    ctx.set_option("mixed_precision", 1)
    try:
        refused(ctx, "mixed_precision", lambda: widths(ctx, S))
    finally:
        ctx.set_option("mixed_precision", 0)
    args = (m.n_depth, m.nus, m.lines["line_nus"], m.lines["doppler_widths"], m.lines["gammas"], m.lines["alphas"], S.B, S.temps, S.ray, S.weights)
    for bad in ([m.n_lines], [0, -1]):  # the indices are checked on the host, before anything is uploaded
        refused(ctx, "lines must index", lambda: ops.equivalent_widths(*args, lines=bad, ctx=ctx))
    # an empty selection and an empty shard: nothing is launched, no error
    with profiled(ctx):
        widths(ctx, S, lines=[])
        widths(ctx, S, shard=(5, 0))
        assert ctx.profile("k_line_ew")[0] == 0
    # the context is still usable, and computes what it computed before
    after = widths(ctx, S)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------
STAGES = ("k_raytrace", "k_line_opacity", "k_line_prepass", "k_total_alphas", "k_dnu_partial", "k_line_adjoint", "k_line_ew")


@pytest.fixture(scope="module")
def engine_model():
    return small_model()


def test_engine(ctx, engine_model):
    m = engine_model
    syn = synthesizer(ctx, m)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        first = {k: ctx.profile(k)[0] for k in STAGES}
    F1 = np.array(syn.F_nu())
    assert first["k_line_ew"] == 0 and syn._ew is None and sum(first.values()) > 0
    with profiled(ctx):
        W, depth = syn.equivalent_widths(ln_strength=[0.0, 1.0])
        ctx.synchronize()
        assert ctx.profile("k_line_ew")[0] == 1 and ctx.profile("k_raytrace")[0] == 0
    W, depth = W.numpy(), depth.numpy()
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        second = {k: ctx.profile(k)[0] for k in STAGES}
    assert second == first and np.array_equal(syn.F_nu(), F1)
    # ops.equivalent_widths on the continuum plane of sdx_total_alphas_dev
    nd, n = syn.n_depth, syn.n_nu
    d_plane = ctx.empty((nd, n))
    ctx.call("sdx_total_alphas_dev", nd, n, syn.d_nus.ptr, 0, n, C.byref(syn.cont), None, 0, d_plane.ptr, n)
    ray = np.asarray(m.atm["dist"]).reshape(-1, 1) / np.cos(m.thetas)
    Wo, do = ops.equivalent_widths(nd, m.nus, m.lines["line_nus"], m.lines["doppler_widths"], m.lines["gammas"], m.lines["alphas"], d_plane,
                                   m.atm["temperatures"], ray, m.weights, ln_strength=[0.0, 1.0], ctx=ctx)
    assert np.array_equal(Wo, W) and np.array_equal(do, depth) and (W > 0).all() and (np.diff(W, axis=1) > 0).all()
    # a caller's plane, a selection in the caller's order, and a synthesizer without a continuum
    Wb, _ = syn.equivalent_widths(lines=[7, 2], background=d_plane)
    assert np.array_equal(Wb.numpy()[:, 0], W[[7, 2], 0])
    syn.close()
    bare = SpectralSynthesizer(m.nus, m.atm["temperatures"], m.atm["dist"], m.thetas, m.weights, m.lines, None, ctx=ctx, track_evaluations=False)
    with pytest.raises(ValueError, match="continuum="):
        bare.equivalent_widths()
    bare.close()


# ---- 7. against the product's own path: a one-line synthesis with the continuum flux, integrated on the host ------------------------
def test_against_one_line_syntheses(ctx, engine_model):
    m = engine_model
    full = synthesizer(ctx, m)
    lines = [int(v) for v in m.x_lines[:3]]
    W = full.equivalent_widths(lines=lines)[0].numpy()[:, 0]
    full.close()
    lam = E.K.nu_to_angstrom(m.nus)
    for j, l in enumerate(lines):
        one = {k: np.ascontiguousarray(v[l:l + 1]) for k, v in m.lines.items()}
        syn = synthesizer(ctx, m, one, keep_continuum_flux=True)
        syn.step()
        ctx.synchronize()
        F, Fc = np.array(syn.F_nu()[-1]), np.array(syn.emergent_continuum)
        syn.close()
        lo, hi = ops.line_windows(m.atm["temperatures"].size, m.nus, one["line_nus"], one["doppler_widths"], one["gammas"], one["alphas"], ctx=ctx)
        ulo, uhi = int(lo.min()), int(hi.max())
        cols = np.arange(ulo, uhi)
        h = E.node_weights(lam, ulo, uhi, cols, np.float64)
        host = float((h * ((Fc - F) / Fc)[cols]).sum())
        span = abs(float(lam[uhi - 1] - lam[ulo]))
        print(f"line {l}: W = {W[j]:.6e} A, one-line synthesis integrated on the host {host:.6e} A, |dW| / span = {abs(W[j] - host) / span:.3e}")
        assert abs(W[j] - host) <= 2e-10 * span


# ---- 8. the fit ---------------------------------------------------------------------------------------------------------------------
def test_fit(ctx, engine_model):
    m = engine_model
    syn = synthesizer(ctx, m)
    lines = [1, 4, 9, 16, 25, 36]
    true = np.random.default_rng(8).uniform(-1.0, 1.0, len(lines))
    W_obs = syn.equivalent_widths(lines=lines, ln_strength=(true * curve_of_growth.LN10)[:, None])[0].numpy()[:, 0]
    sol = syn.fit_equivalent_widths(W_obs, lines=lines)
    syn.close()
    print("fit: recovered - true (dex)", sol.delta_log_gf - true, "bracket widths", sol.bracket[:, 1] - sol.bracket[:, 0], "converged", sol.converged)
    assert sol.converged.all()
    assert ((sol.bracket[:, 0] <= true) & (true <= sol.bracket[:, 1])).all()
    assert ((sol.bracket[:, 0] <= sol.delta_log_gf) & (sol.delta_log_gf <= sol.bracket[:, 1])).all()
    assert (np.abs(sol.delta_log_gf - true) <= 1e-3).all()
