"""The cell-integrated rotation profile on the device (k_rotate_integrated, k_rotate_integrated_adjoint, k_rotate_moments;
Instrument(rotation="integrated"); the "v_rot" column of parameter_tangents, observed_jacobian and chi2_instrument_gradient) against
50-digit mpmath, against its restatement (tests/rotation_integrated_reference.py), by the dot identity and against Richardson quotients
of the device's own forward, whose allowance is twice the restatement's own gap for the same steps
(tests/test_rotation_integrated_cpu.py records it).  Every comparison also requires the compared quantity to exceed ten times its
allowance somewhere, so a zero cannot pass; figures are printed before they are asserted."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import macroturbulence_reference as mref
import observe_tangent_reference as tref
import rotation_integrated_reference as iref
import rotation_reference as rref
from rotation_integrated_reference import DERIV_TOL, LD, MOMENT_TOL, ROT_TOL, SUM_TOL
from stardis_amd import _lib, ops
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from test_gpu_observe_tangent import ENGINE_EDGES, EPS, V_MAC, V_RAD, V_ROT, capture, model  # noqa: F401  (model: the module-scoped fixture)
from test_gpu_response import profiled, synthesizer
from test_observe_tangent_cpu import IRREGULAR, TWO_DENSITY
from test_rotation_integrated_cpu import (EDGE_GRID, EDGE_V, LNV_STEP, QUOTIENT_CASES, QUOTIENT_GRIDS, SLICE, SUB_SPACING_V, V_STAR, flux_of,
                                          moment_cells)

pytestmark = pytest.mark.gpu

GRIDS = {"slice": SLICE, "irregular": IRREGULAR, "two-density": np.ascontiguousarray(TWO_DENSITY[:3000]), "edge": EDGE_GRID}
WHOLE_GRID_V = 2500.0  # reach = 54 A: every window covers the slice's 19 A
FIELDS = ("out", "dlnv", "deps")


def vectors(lam, seed=11):
    """-> flux, reference, u (signed), u_reference (signed)"""
    rng = np.random.default_rng(seed)
    return 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0), rng.standard_normal(lam.size), rng.standard_normal(lam.size)


def dev_rotate(ctx, lam, flux, V, eps, reference=None, derivatives=True):
    """sdx_rotate_integrated_dev on uploaded arrays, the pair through device memory -> {out, dlnv, deps[, *_reference]} as host arrays"""
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_f, d_g, d_rot = up(lam), up(flux), up(reference), up(np.array([V, eps]))
    outs = {k + tag: ctx.empty((lam.size,)) for k in (FIELDS if derivatives else FIELDS[:1]) for tag in (("", "_reference") if reference is not None else ("",))}
    order = ("out", "out_reference", "dlnv", "dlnv_reference", "deps", "deps_reference")
    ctx.call("sdx_rotate_integrated_dev", lam.size, d_lam.ptr, d_f.ptr, _lib.ptr_of(d_g), d_rot.ptr, *(_lib.ptr_of(outs.get(k)) for k in order))
    ctx.synchronize()
    return {k: np.array(a.numpy()) for k, a in outs.items()}


def dev_adjoint(ctx, lam, u, V, eps, u_reference=None, nus=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_u, d_ur, d_nus, d_rot = up(lam), up(u), up(u_reference), up(nus), up(np.array([V, eps]))
    w, w_ref = ctx.empty((lam.size,)), None if u_reference is None else ctx.empty((lam.size,))
    ctx.call("sdx_rotate_integrated_adjoint_dev", lam.size, d_lam.ptr, d_rot.ptr, d_u.ptr, _lib.ptr_of(d_ur), _lib.ptr_of(d_nus), w.ptr, _lib.ptr_of(w_ref))
    ctx.synchronize()
    return np.array(w.numpy()), None if w_ref is None else np.array(w_ref.numpy())


def held(tag, got, ref, scale, tol, nonzero=True):
    err, allow = np.abs(got.astype(LD) - ref).astype(np.float64), tol * scale.astype(np.float64)
    print(f"{tag}: {ref.size} points, worst |device - restatement| / allowance {float(np.max(err / allow)):.3e}, largest |value| / allowance "
          f"{float(np.max(np.abs(ref).astype(np.float64) / allow)):.3e}")
    assert np.all(np.isfinite(got)) and np.all(allow > 0)
    assert np.all(err <= allow)
    assert not nonzero or np.any(np.abs(ref).astype(np.float64) > 10 * allow)


# ---- 1: the moments against mpmath -------------------------------------------------------------------------------------------------------
def test_moments_against_mpmath(ctx):
    """sdx_rotate_moments_dev on cells 1e-6 to 2 wide, touching -1 and +1, in one half and across 0, relative to |M|: MOMENT_TOL
    (tests/rotation_integrated_reference.py).  A difference of antiderivatives in fp64 would miss it by 1e-16 / width."""
    mpmath.mp.dps = 50
    ya, yb = moment_cells()
    worst = [0.0, 0.0]
    for eps in (0.0, 0.6, 1.0):
        m0, m1 = ops.rotate_moments(ya, yb, eps, ctx=ctx)
        d = [ctx.upload(a) for a in (ya, yb, np.full(ya.size, eps))]
        o = [ctx.empty((ya.size,)), ctx.empty((ya.size,))]
        ctx.call("sdx_rotate_moments_dev", ya.size, d[0].ptr, d[1].ptr, d[2].ptr, o[0].ptr, o[1].ptr)
        assert np.array_equal(o[0].numpy(), m0) and np.array_equal(o[1].numpy(), m1)  # the device entry and the host-buffer twin
        for k in range(ya.size):
            e0, e1 = iref.mp_moments(ya[k], yb[k], eps)
            assert e0 > 0 and m0[k] > 0
            worst[0] = max(worst[0], float(abs(mpmath.mpf(float(m0[k])) - e0) / e0))
            if e1 == 0:
                assert m1[k] == 0, (ya[k], yb[k])
            else:
                worst[1] = max(worst[1], float(abs(mpmath.mpf(float(m1[k])) - e1) / abs(e1)))
    print(f"distance from 50 digits over {ya.size} cells x 3 eps: M0 {worst[0]:.3e}, M1 {worst[1]:.3e}, allowed {MOMENT_TOL:.3e}")
    assert 0 < worst[0] <= MOMENT_TOL and 0 < worst[1] <= MOMENT_TOL
    assert ops.rotate_moments(2.0, 3.0, ctx=ctx) == (0.0, 0.0) and ops.rotate_moments(0.5, 0.5, ctx=ctx) == (0.0, 0.0)  # empty cells


# ---- 2: forward and derivatives against the restatement ------------------------------------------------------------------------------
def check_forward(ctx, tag, lam, V, epsilons=(0.0, 0.6, 1.0), nonzero=True):
    f, g, _, _ = vectors(lam)
    for eps in epsilons:
        got = dev_rotate(ctx, lam, f, V, eps, reference=g)
        alone = dev_rotate(ctx, lam, f, V, eps)
        plain = dev_rotate(ctx, lam, f, V, eps, reference=g, derivatives=False)
        r = iref.rotate(lam, f, V, eps, reference=g)
        for tagged in ("", "_reference"):
            held(f"{tag}, V = {V:.4g}, eps = {eps}: out{tagged}", got["out" + tagged], r["out" + tagged], r["scale" + tagged], ROT_TOL)
            # (eps = 1 is the profile's own limb: d / d eps keeps its size; d / d ln V of the smooth reference is small but not zero)
            held(f"{tag}, V = {V:.4g}, eps = {eps}: dout_lnv{tagged}", got["dlnv" + tagged], r["dlnv" + tagged], r["dlnv_terms" + tagged], DERIV_TOL, nonzero)
            held(f"{tag}, V = {V:.4g}, eps = {eps}: dout_eps{tagged}", got["deps" + tagged], r["deps" + tagged], r["deps_terms" + tagged], DERIV_TOL, nonzero)
        # the flux does not depend on whether a reference or a derivative goes along: the same bits from both kernels
        assert all(np.array_equal(alone[k], got[k]) for k in FIELDS) and all(np.array_equal(plain[k], got[k]) for k in plain)


@pytest.mark.parametrize("V", [2.0, 10.0, 100.0])
def test_forward_on_the_slice(ctx, V):
    """7, 34 and 335 cells per window: eight lanes per point, then a wave per point on the other side of kObsShort"""
    expected = 2 * V / K.C_KMS * SLICE * (SLICE.size - 1) / (SLICE[-1] - SLICE[0])
    print(f"V = {V}: the mapping's estimate {expected.min():.2f} .. {expected.max():.2f} points per window")
    assert (expected.max() <= 32) == (V == 2.0) and (expected.min() > 32) == (V != 2.0)
    check_forward(ctx, "slice", SLICE, V)


@pytest.mark.parametrize("V", SUB_SPACING_V + (WHOLE_GRID_V,))
def test_forward_below_one_spacing_and_across_the_whole_grid(ctx, V):
    """three windows narrower than a cell (three weights each; the sampled sum is the identity there), and one that covers the grid
    from every point (every window truncated at both ends: the end terms of d / d ln V)"""
    lam = SLICE if V != WHOLE_GRID_V else SLICE[:700]
    check_forward(ctx, "slice", lam, V, epsilons=(0.6,))
    f = vectors(lam)[0]
    if V == WHOLE_GRID_V:
        assert np.all(lam * (1 - V / K.C_KMS) < lam[0]) and np.all(lam * (1 + V / K.C_KMS) > lam[-1])
    else:
        out = dev_rotate(ctx, lam, f, V, 0.6)["out"]
        sampled = np.empty(lam.size)
        ctx.call("sdx_rotate_f64", lam.size, lam.ctypes.data, f.ctypes.data, None, V, 0.6, sampled.ctypes.data, None)
        # (the sampled window is the point alone: (K h F) / (K h), two roundings)
        assert np.max(np.abs(sampled / f - 1)) <= 3e-16 and np.max(np.abs(out / f - 1)) > 1e-4


@pytest.mark.parametrize("grid,V", [("irregular", 10.0), ("irregular", 100.0), ("two-density", 10.0), ("two-density", 100.0)])
def test_forward_on_other_grids(ctx, grid, V):
    """the mean-spacing estimate is wrong locally; either mapping must serve any point"""
    check_forward(ctx, grid, GRIDS[grid], V, epsilons=(0.6,))


def test_forward_with_a_node_on_the_edge_and_on_grids_of_two_and_three_points(ctx):
    """clear_of_profile_edge is false for the edge grid and no exemption is needed: ROT_TOL, where the sampled sum is held to 1e-7"""
    for V in EDGE_V:
        assert not rref.clear_of_profile_edge(EDGE_GRID, V, 1e-8) and rref.profile_edge_margin(EDGE_GRID, V) < 1e-15
        check_forward(ctx, "node on the edge", EDGE_GRID, V, epsilons=(0.0, 0.6))
    for n in (2, 3):
        lam = 6560.0 + 0.013 * np.arange(n) ** 1.1
        for V in (0.3, 40.0):  # a window narrower than the cell; every window truncated
            check_forward(ctx, f"n = {n}", lam, V, epsilons=(0.6,))


def test_zero_velocity_is_a_copy_with_zero_derivatives(ctx):
    f, g, u, _ = vectors(SLICE)
    for V in (0.0, -5.0, np.nan):
        got = dev_rotate(ctx, SLICE, f, V, 0.6, reference=g)
        assert np.array_equal(got["out"], f) and np.array_equal(got["out_reference"], g), V
        assert all(not got[k + tag].any() for k in ("dlnv", "deps") for tag in ("", "_reference")), V
        assert np.array_equal(dev_adjoint(ctx, SLICE, u, V, 0.6)[0], u), V


# ---- 3: the adjoint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,V", [("slice", 2.0), ("slice", 10.0), ("slice", 100.0), ("slice", 0.3), ("slice-whole", WHOLE_GRID_V), ("irregular", 23.7),
                                    ("two-density", 100.0), ("edge", EDGE_V[0]), ("edge", EDGE_V[1])])
def test_adjoint_against_the_restatement_and_the_dot_identity(ctx, grid, V):
    """per node to ROT_TOL of its peak terms; <rotate(f), u> = <f, adjoint(u)> to SUM_TOL of dot_terms — also with a node on the edge and
    with truncated windows (every window of slice-whole, the ends of every other grid)"""
    lam = SLICE[:700] if grid == "slice-whole" else GRIDS[grid]
    f, g, u, u_ref = vectors(lam)
    nus = K.C_KMS * 1e13 / lam
    for eps in (0.0, 0.6, 1.0) if grid == "slice" and V == 10.0 else (0.6,):
        w, w_ref = dev_adjoint(ctx, lam, u, V, eps, u_reference=u_ref)
        alone, _ = dev_adjoint(ctx, lam, u, V, eps)
        r_w, r_wref, scale, scale_ref = iref.adjoint(lam, u, V, eps, u_reference=u_ref)
        held(f"{grid}, V = {V:.4g}, eps = {eps}: w", w, r_w, scale, ROT_TOL)
        held(f"{grid}, V = {V:.4g}, eps = {eps}: w_reference", w_ref, r_wref, scale_ref, ROT_TOL)
        assert np.array_equal(alone, w)
        out = dev_rotate(ctx, lam, f, V, eps, derivatives=False)["out"]
        terms = iref.dot_terms(lam, u, f, V, eps)
        lhs, rhs = float(np.sum(out.astype(LD) * u)), float(np.sum(w.astype(LD) * f))
        print(f"{grid}, V = {V:.4g}, eps = {eps}: <rotate(f), u> = {lhs:.15e}, <f, adjoint(u)> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * terms):.3e}")
        assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms
        with_nus, _ = dev_adjoint(ctx, lam, u, V, eps, nus=nus)
        assert np.max(np.abs(with_nus - w * nus / lam) / np.abs(w * nus / lam)) <= 4e-16
        assert np.array_equal(ops.rotate_integrated_adjoint(lam, u, V, eps, u_reference=u_ref, ctx=ctx)[1], w_ref)  # the host-buffer twin


# ---- 4: d / d ln V against quotients of the device's own forward --------------------------------------------------------------------------
@pytest.mark.parametrize("grid,V", QUOTIENT_CASES)
def test_derivative_against_richardson_quotients_of_the_device_forward(ctx, grid, V):
    """the allowance is twice the restatement's own gap between the same Richardson value and its analytic derivative (the margin of two
    for the device's rounding in the quotient); at V* every window of the log-uniform grid gains a node, where the sampled sum's one-sided
    quotients (printed, not asserted) disagree with each other"""
    lam = QUOTIENT_GRIDS[grid]
    f = flux_of(lam)
    gap, size = iref.quotient_gap(lam, f, V, 0.6, LNV_STEP)
    forward = lambda v: dev_rotate(ctx, lam, f, float(v), 0.6, derivatives=False)["out"].astype(LD)  # noqa: E731
    quotient = iref.richardson(forward, V, LNV_STEP)
    got = dev_rotate(ctx, lam, f, V, 0.6)["dlnv"]
    err = float(np.max(np.abs(got - quotient)))
    print(f"{grid}, V = {V:.6f}: worst |dout_lnv - Richardson of the device's forward| {err:.3e}, allowed 2 x {gap:.3e}; largest |dout_lnv| {size:.3e}")
    if V == V_STAR:
        def sampled(v):
            out = np.empty(lam.size)
            ctx.call("sdx_rotate_f64", lam.size, lam.ctypes.data, f.ctypes.data, None, float(v), 0.6, out.ctypes.data, None)
            return out.astype(LD)
        h = 1e-4
        up, down = (sampled(V * np.exp(h)) - sampled(V)) / h, (sampled(V) - sampled(V * np.exp(-h))) / h
        mine_up, mine_down = (forward(V * np.exp(h)) - forward(V)) / h, (forward(V) - forward(V * np.exp(-h))) / h
        inner = slice(40, -40)
        print(f"one-sided quotients at V* (h = {h}), max over interior points of |up - down|: sampled {float(np.max(np.abs(up - down)[inner])):.3e}, "
              f"integrated {float(np.max(np.abs(mine_up - mine_down)[inner])):.3e}; largest |quotient|: sampled {float(np.max(np.abs(up)[inner])):.3e}, "
              f"integrated {float(np.max(np.abs(mine_up)[inner])):.3e}")
    assert err <= 2 * gap and size > 10 * 2 * gap


# ---- 5: bits ----------------------------------------------------------------------------------------------------------------------------
def test_same_bits_eager_replayed_and_from_the_host_twin_and_a_graph_follows_set_rotation(ctx):
    lam = SLICE
    f, g, u, u_ref = vectors(lam)
    inst = Instrument(np.linspace(lam[100], lam[-100], 401), resolving_power=5.0e4, ctx=ctx, v_rot=10.0, limb_darkening=0.6, rotation="integrated")
    d_lam, d_f, d_g, d_u = (ctx.upload(a) for a in (lam, f, g, u))
    outs = [ctx.empty((lam.size,)) for _ in range(6)]
    w = ctx.empty((lam.size,))

    def run():
        ctx.call("sdx_rotate_integrated_dev", lam.size, d_lam.ptr, d_f.ptr, d_g.ptr, inst.d_rot.ptr, *(o.ptr for o in outs))
        ctx.call("sdx_rotate_integrated_adjoint_dev", lam.size, d_lam.ptr, inst.d_rot.ptr, d_u.ptr, None, None, w.ptr, None)

    result = lambda: [np.array(o.numpy()) for o in outs + [w]]  # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    run()
    eager0 = result()
    run()
    assert same(eager0, result()) and all(a.any() for a in eager0)
    inst.set_rotation(23.7, 0.3)
    run()
    eager1 = result()
    assert not any(np.array_equal(x, y) for x, y in zip(eager0, eager1))
    inst.set_rotation(10.0, 0.6)
    graph = capture(ctx, run)  # (the adjoint's scratch was sized by the eager runs: the capture allocates nothing)
    try:
        for o in outs + [w]:
            o.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        inst.set_rotation(23.7, 0.3)  # no new capture: the kernels read the pair from device memory
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    assert same(replay0, eager0) and same(replay1, eager1)
    twin = ops.rotate_integrated(lam, f, 23.7, 0.3, reference=g, derivatives=True, ctx=ctx)
    assert same(twin, eager1[:6]) and np.array_equal(ops.rotate_integrated_adjoint(lam, u, 23.7, 0.3, ctx=ctx), eager1[6])
    assert np.array_equal(ops.rotate_integrated(lam, f, 23.7, 0.3, ctx=ctx), eager1[0])
    assert same(inst.rotate_host(lam, f, g), eager1[:2])


def test_the_default_mode_is_the_sampled_one_bit_for_bit(ctx):
    """Instrument(v_rot=10) and Instrument(v_rot=10, rotation="sampled") launch k_rotate and give identical bits; the integrated mode
    launches k_rotate_integrated instead and gives other bits"""
    lam = SLICE
    f, g, _, _ = vectors(lam)
    edges = np.linspace(lam[100], lam[-100], 401)
    d_lam, d_f, d_g, d_c = (ctx.upload(a) for a in (lam, f, g, np.random.default_rng(1).standard_normal(400)))
    stages = ("k_rotate", "k_rotate_adjoint", "k_rotate_integrated", "k_rotate_integrated_adjoint")
    res = {}
    for tag, kw in (("default", {}), ("sampled", dict(rotation="sampled")), ("integrated", dict(rotation="integrated"))):
        inst = Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=10.0, **kw)
        with profiled(ctx):
            obs = np.array(inst.observe(d_lam, d_f, lam.size, d_g).numpy())
            adj = np.array(inst.adjoint(d_lam, lam.size, d_c).numpy())
            ctx.synchronize()
            counts = [ctx.profile(k)[0] for k in stages]
        print(f"{tag}: launches {dict(zip(stages, counts))}")
        assert counts == ([0, 0, 1, 1] if tag == "integrated" else [1, 1, 0, 0])
        res[tag] = (obs, adj, inst.observe_host(lam, f, g), inst.adjoint_host(lam, d_c.numpy()))
        assert np.array_equal(res[tag][0], res[tag][2], equal_nan=True) and np.array_equal(res[tag][1], res[tag][3])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res["default"], res["sampled"]))
    assert not np.array_equal(res["default"][0], res["integrated"][0], equal_nan=True) and not np.array_equal(res["default"][1], res["integrated"][1])
    close = np.nanmax(np.abs(res["default"][0] - res["integrated"][0]))
    print(f"sampled against integrated at 34 points per window: largest difference of the normalised pixels {close:.3e}")
    assert close < 1e-3


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_serving(ctx):
    lib = ctx.lib
    lam = np.ascontiguousarray(SLICE[:500])
    f, g, u, _ = vectors(lam)
    n = lam.size
    expect = dev_rotate(ctx, lam, f, 10.0, 0.6)
    d, r, r2, r3 = ctx.upload(lam), ctx.empty((n,)), ctx.empty((n,)), ctx.empty((n,))
    with profiled(ctx):
        # (ctx, n, lambdas, flux, reference, rot_dev, out, out_reference, dout_lnv, dout_lnv_reference, dout_eps, dout_eps_reference)
        for args in ((1, d.ptr, d.ptr, None, d.ptr, r.ptr, None, None, None, None, None),  # n < 2
                     (n, None, d.ptr, None, d.ptr, r.ptr, None, None, None, None, None), (n, d.ptr, None, None, d.ptr, r.ptr, None, None, None, None, None),
                     (n, d.ptr, d.ptr, None, None, r.ptr, None, None, None, None, None), (n, d.ptr, d.ptr, None, d.ptr, None, None, r2.ptr, None, None, None),
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, r.ptr, None, None, None, None, None),  # reference without out_reference
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, r2.ptr, None, None, None, None),  # out_reference without reference
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, r2.ptr, r3.ptr, None, None),  # dout_lnv_reference without reference
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, None, None, r2.ptr, r3.ptr),  # dout_eps_reference without reference
                     (n, d.ptr, d.ptr, None, d.ptr, d.ptr, None, None, None, None, None),  # out is an input
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, d.ptr, None, None, None),  # dout_lnv is an input
                     (n, d.ptr, d.ptr, None, d.ptr, r.ptr, None, r2.ptr, None, r2.ptr, None)):  # two outputs in one buffer
            assert lib.sdx_rotate_integrated_dev(ctx.handle, *args) == -1 and b"rotate_integrated" in lib.sdx_last_error_string(), args
        # (ctx, n, lambdas, rot_dev, u, u_reference, nus, w, w_reference)
        for args in ((1, d.ptr, d.ptr, d.ptr, None, None, r.ptr, None), (n, None, d.ptr, d.ptr, None, None, r.ptr, None), (n, d.ptr, None, d.ptr, None, None, r.ptr, None),
                     (n, d.ptr, d.ptr, None, None, None, r.ptr, None), (n, d.ptr, d.ptr, d.ptr, None, None, None, None),
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, None, r.ptr, None), (n, d.ptr, d.ptr, d.ptr, None, None, r.ptr, r2.ptr)):
            assert lib.sdx_rotate_integrated_adjoint_dev(ctx.handle, *args) == -1 and b"rotate_integrated_adjoint" in lib.sdx_last_error_string(), args
        # the twins check what the kernels cannot, before any copy
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = np.full(n, -7.0)
        for tag, kw in dict(lambdas=dict(lam=np.ascontiguousarray(lam[::-1])), v_rot=dict(V=3000.0), limb_darkening=dict(eps=1.5)).items():
            a = dict(dict(lam=lam, V=10.0, eps=0.6), **kw)
            rc = lib.sdx_rotate_integrated_f64(ctx.handle, n, p(a["lam"]), p(f), None, a["V"], a["eps"], p(out), None, None, None, None, None)
            msg = lib.sdx_last_error_string().decode()
            rc2 = lib.sdx_rotate_integrated_adjoint_f64(ctx.handle, n, p(a["lam"]), a["V"], a["eps"], p(u), None, None, p(out), None)
            print(f"{tag}: rc {rc}, '{msg}'; adjoint rc {rc2}, '{lib.sdx_last_error_string().decode()}'")
            assert rc == -1 and rc2 == -1 and np.all(out == -7.0) and tag in msg and tag in lib.sdx_last_error_string().decode()
        ctx.synchronize()
        assert ctx.profile("k_rotate_integrated")[0] == 0 and ctx.profile("k_rotate_integrated_adjoint")[0] == 0
        again = dev_rotate(ctx, lam, f, 10.0, 0.6)
        assert all(np.array_equal(again[k], expect[k]) for k in expect) and ctx.profile("k_rotate_integrated")[0] == 1


# ---- 7: the Instrument, alone and through the synthesizer ----------------------------------------------------------------------------
def chain(lam, f, g, inst, V, eps, zeta):
    """the restatement chain rotate -> macroturbulence -> observe with the tangent d / dV -> (observed, d observed / dV, its terms)"""
    r = iref.rotate(lam, f, V, eps, reference=g)
    b = {k: r[k].astype(np.float64) for k in ("out", "out_reference", "dlnv", "dlnv_reference")}
    m = {k: mref.macroturbulence(lam, b[k], zeta)["out"].astype(np.float64) for k in b}
    t = tref.observe_tangent(lam, m["out"], inst.edges, inst.sigma, inst.doppler, reference=m["out_reference"], dflux=m["dlnv"], dreference=m["dlnv_reference"])
    return t["out"], t["flux"] / LD(V), t["flux_terms"] / LD(V)


def test_instrument_parameter_tangents_with_v_rot(ctx):
    """parameter_tangents(wrt="v_rot") equals the host twin bit for bit and matches the restatement chain to the tangent file's FLUX_TOL
    of the sum of absolute terms; wrt=None ends with "v_rot", and "limb_darkening" comes from the same launch"""
    lam = np.ascontiguousarray(SLICE)
    edges = np.linspace(lam[150], lam[-150], 301)
    f, g = flux_of(lam), vectors(lam)[1]
    V, eps, zeta = 10.0, 0.5, 3.2
    inst = Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=V, limb_darkening=eps, v_mac=zeta, rotation="integrated")
    inst.set_radial_velocity(12.0)
    d_lam, d_f, d_g = (ctx.upload(a) for a in (lam, f, g))
    with profiled(ctx):
        cols = {k: np.array(v.numpy()) for k, v in inst.parameter_tangents(d_lam, lam.size, d_f, reference=d_g).items()}
        ctx.synchronize()
        launches = {k: ctx.profile(k)[0] for k in ("k_rotate_integrated", "k_rotate_tangent", "k_rotate")}
    print(f"launches of one parameter_tangents call with every column: {launches}")
    assert list(cols) == ["v_rad", "lsf", "v_mac", "limb_darkening", "v_rot"] and launches == {"k_rotate_integrated": 1, "k_rotate_tangent": 0, "k_rotate": 0}
    host = inst.parameter_tangents_host(lam, f, reference=g)
    assert all(np.array_equal(host[k], cols[k], equal_nan=True) for k in cols)
    one = np.array(inst.parameter_tangents(d_lam, lam.size, d_f, reference=d_g, wrt="v_rot")["v_rot"].numpy())
    assert np.array_equal(one, cols["v_rot"], equal_nan=True)
    expect_obs, expect, terms = chain(lam, f, g, inst, V, eps, zeta)
    ok = ~np.isnan(expect.astype(np.float64))
    assert np.array_equal(np.isnan(cols["v_rot"]), ~ok) and ok.sum() == 300
    err, allow = np.abs(cols["v_rot"][ok] - expect[ok]).astype(np.float64), (tref.FLUX_TOL * terms[ok]).astype(np.float64)
    print(f"v_rot column: {int(ok.sum())} pixels, worst |column - restatement chain| / allowance {np.max(err / allow):.3e}, largest |column| / allowance "
          f"{np.max(np.abs(expect[ok]).astype(np.float64) / allow):.3e}")
    assert np.all(err <= allow) and np.any(np.abs(expect[ok]).astype(np.float64) > 10 * allow)
    with pytest.raises(ValueError, match='rotation="integrated"'):
        Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=V).parameter_tangents(d_lam, lam.size, d_f, wrt="v_rot")


def test_engine_jacobian_and_chi2_with_v_rot(ctx, model):  # noqa: F811
    m = model
    lam = K.nu_to_angstrom(m.nus)
    inst = Instrument(ENGINE_EDGES, sigma=0.05, ctx=ctx, v_rot=V_ROT, limb_darkening=EPS, v_mac=V_MAC, rotation="integrated")
    inst.set_radial_velocity(V_RAD)
    syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=inst)
    names = ("v_rad", "lsf", "v_mac", "limb_darkening", "v_rot")
    syn.step()
    edge = inst.edge_affected(lam)
    rng = np.random.default_rng(8)
    f_lam = np.array(syn.d_Flam.numpy())
    for norm in (False, True):
        obs = np.array((syn.observed_normalized if norm else syn.observed).numpy())
        jac = {k: np.array(v.numpy()) for k, v in syn.observed_jacobian(names, normalized=norm).items()}
        assert list(jac) == list(names)
        data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(27))
        ivar = rng.uniform(0.5, 2.0, 27) / np.nanmax(np.abs(obs)) ** 2
        ivar[5] = 0.0
        used = ~np.isnan(obs) & (ivar != 0) & ~edge
        chi2, grad, Hm = syn.chi2_instrument_gradient(data, ivar, names, normalized=norm, curvature=True)
        resid, w = np.where(used, data, 0.0) - np.where(used, obs, 0.0), np.where(used, ivar, 0.0)
        assert used.sum() == 23 and chi2 == float(np.sum(w * resid * resid)) and list(grad) == list(names) and Hm.shape == (5, 5)
        J = np.stack([np.where(used, jac[k], 0.0) for k in names], axis=1)
        expect_g, terms_g = J.T @ (-2.0 * w * resid), np.abs(J).T @ np.abs(2.0 * w * resid)
        expect_H, terms_H = 2.0 * (J * w[:, None]).T @ J, 2.0 * (np.abs(J) * w[:, None]).T @ np.abs(J)
        got_g = np.array([grad[k] for k in names])
        print(f"normalized = {norm}: chi2 {chi2!r}, worst |gradient - numpy| / terms {np.max(np.abs(got_g - expect_g) / terms_g):.3e}, worst |H - numpy| / terms "
              f"{np.max(np.abs(Hm - expect_H) / terms_H):.3e}")
        assert np.all(np.abs(got_g - expect_g) <= SUM_TOL * terms_g) and np.all(np.abs(got_g) > 10 * SUM_TOL * terms_g)
        assert np.array_equal(Hm, Hm.T) and np.all(np.abs(Hm - expect_H) <= SUM_TOL * terms_H) and np.all(np.diag(Hm) > 0)
        assert syn.chi2_instrument_gradient(data, ivar, "v_rot", normalized=norm) == (chi2, {"v_rot": grad["v_rot"]})

        # the central difference of chi-square of two whole steps that "v_rot" replaces, within twice the restatement's gap for that step:
        # the restatement's own chi-square quotient against its own analytic gradient, on the step's F_lambda
        h = 0.01 * V_ROT
        def chi2_at(v):
            inst.set_rotation(v)
            syn.step()
            o = np.array((syn.observed_normalized if norm else syn.observed).numpy())
            r = np.where(used, data, 0.0) - np.where(used, o, 0.0)
            return LD(np.sum((w * r).astype(LD) * r))
        central = float((chi2_at(V_ROT + h) - chi2_at(V_ROT - h)) / (2 * h))
        inst.set_rotation(V_ROT)
        syn.step()
        g_lam = np.array(syn.d_Fclam.numpy()) if norm else None

        def restated(v):
            o, d, _ = chain(lam, f_lam, g_lam, inst, v, EPS, V_MAC) if norm else chain_plain(lam, f_lam, inst, v, EPS, V_MAC)
            r = np.where(used, data, 0.0).astype(LD) - np.where(used, o, 0)
            return np.sum(w * r * r), np.sum(-2 * w * r * np.where(used, d, 0))
        gap = abs(float((restated(V_ROT + h)[0] - restated(V_ROT - h)[0]) / (2 * h) - restated(V_ROT)[1]))
        print(f"normalized = {norm}: d chi2 / d v_rot by the tangent {grad['v_rot']:+.12e}, by two whole steps {central:+.12e}, difference "
              f"{abs(grad['v_rot'] - central):.3e}, allowed 2 x {gap:.3e}")
        assert abs(grad["v_rot"] - central) <= 2 * gap and abs(grad["v_rot"]) > 20 * gap
    with pytest.raises(ValueError, match="v_rad, lsf, v_mac, limb_darkening"):
        syn.observed_jacobian(("v_rad", "v_sin_i"))
    syn.close()


def chain_plain(lam, f, inst, V, eps, zeta):
    r = iref.rotate(lam, f, V, eps)
    b = {k: r[k].astype(np.float64) for k in ("out", "dlnv")}
    m = {k: mref.macroturbulence(lam, b[k], zeta)["out"].astype(np.float64) for k in b}
    t = tref.observe_tangent(lam, m["out"], inst.edges, inst.sigma, inst.doppler, dflux=m["dlnv"])
    return t["out"], t["flux"] / LD(V), t["flux_terms"] / LD(V)
