"""The transpose and the V-derivative of the disk integration on the device (sdx_disk_integrate_adjoint_dev / _f64,
sdx_disk_integrate_deriv_dev / _f64, ops.disk_integrate(derivative=True), ops.disk_integrate_adjoint) against their longdouble restatement
(tests/disk_adjoint_reference.py, itself pinned by tests/test_disk_adjoint_cpu.py).

Tolerances, each taken against the sum of the ABSOLUTE terms of the quantity compared (the restatement returns it):
  the adjoint's rows and the dot identity: 1e-11 (rotation_reference.ROT_TOL, the project's tolerance for the integrated rotation);
  dout_lnv: 1e-10 (the tolerance k_rotate_integrated's derivatives have);
  dout_lnv against Richardson quotients of the DEVICE's forward: the device's worst gap over a case's points within twice the
    restatement's worst gap to the same quotients (a quotient of fp64 forward values is uncertain by 2^-52 scale / step; both gaps are that).
Every comparison prints its worst figure in units of its allowance before it asserts.  For the derivative every truncated (point, ring) is
asserted to keep 1 - |y_end| >= 1e-5, the derivative's contract.  V = 0, out of the <true> launch, two calls, a graph replay and the
host-buffer twin are compared bit for bit."""
import numpy as np
import pytest

import disk_adjoint_reference as A
import disk_integration_reference as D
from stardis_amd import ops
from test_gpu_disk_integration import jittered, rings, spectra, uniform
from test_gpu_observe_tangent import capture

pytestmark = pytest.mark.gpu

LD = D.LD
DERIV_TOL = 1e-10
MARGIN = 1e-5


@pytest.fixture(autouse=True)
def extended_precision():
    if not D.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def weights_over(n, seed, points=None):
    """u over the broadened points (zero outside `points`)"""
    u = np.random.default_rng(seed).standard_normal(n)
    if points is not None:
        keep = np.zeros(n, dtype=bool)
        keep[np.asarray(points)] = True
        u = np.where(keep, u, 0.0)
    return u


def adjoint_against_restatement(ctx, label, lam, I, scale, w, V, points=None, with_nus=True, seed=11):
    """the rows W (with and without nus, with u_reference) and the dot identity against the device's forward"""
    u, ur = weights_over(lam.size, seed, points), weights_over(lam.size, seed + 1, points)
    W, Wr = ops.disk_integrate_adjoint(lam, u, scale, w, V, u_reference=ur, ctx=ctx)
    worst = 0.0
    for got, uu in ((W, u), (Wr, ur)):
        want, terms = A.adjoint_rows(lam, uu, scale, w, V, points=points)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        assert np.all(got[terms == 0] == 0)
        some = terms > 0
        worst = max(worst, float((np.abs(got.astype(LD) - want)[some] / (D.ROT_TOL * terms[some])).max()))
    if with_nus:
        nus = 2.99792458e18 / lam
        Wn = ops.disk_integrate_adjoint(lam, u, scale, w, V, nus=nus, ctx=ctx)
        want, terms = A.adjoint_rows(lam, u, scale, w, V, nus=nus, points=points)
        some = terms > 0
        worst = max(worst, float((np.abs(Wn.astype(LD) - want)[some] / (D.ROT_TOL * terms[some])).max()))
    out = ops.disk_integrate(lam, I, scale, w, V, ctx=ctx)
    lhs, rhs = (u.astype(LD) * out.astype(LD)).sum(), (W.astype(LD) * I.astype(LD)).sum()
    _, terms = A.adjoint_rows(lam, u, scale, w, V, points=points)
    dot = float(abs(lhs - rhs) / (D.ROT_TOL * (terms * np.abs(I)).sum()))
    print(f"{label}: n={lam.size} rings={scale.size} V={V}: adjoint rows worst / allowance = {worst:.3e}, dot identity / allowance = {dot:.3e}")
    assert worst <= 1.0 and dot <= 1.0


def derivative_against_restatement(ctx, label, lam, I, scale, w, V, points=None, reference=None, h=2.0 ** -10):
    got = ops.disk_integrate(lam, I, scale, w, V, reference=reference, derivative=True, ctx=ctx)
    plain = ops.disk_integrate(lam, I, scale, w, V, reference=reference, ctx=ctx)
    if reference is None:
        assert np.array_equal(got[0], plain)
        pairs = [(got[1], I)]
    else:
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        pairs = [(got[2], I), (got[3], reference)]
    sel = slice(None) if points is None else np.asarray(points)
    worst = 0.0
    for d, planes in pairs:
        assert d.shape == lam.shape and np.all(np.isfinite(d))
        want, terms, margin = A.disk_derivative(lam, planes, scale, w, V, points)
        assert margin.min() >= MARGIN, f"a truncated window's end within {margin.min():.1e} of a ring's edge: outside the derivative's contract"
        assert np.all(terms > 0)
        worst = max(worst, float((np.abs(d[sel].astype(LD) - want) / (DERIV_TOL * terms)).max()))
    # Richardson quotients of the device's own forward (V (1 +- h / 4) is exact in fp64 for the V used here)
    forward = lambda v: ops.disk_integrate(lam, I, scale, w, float(v), ctx=ctx)[sel].astype(LD)  # noqa: E731
    assert all(float(LD(V) * (1 + s * LD(h) / 4)) == V * (1 + s * h / 4) for s in (-1, 1))
    quot, _ = A.richardson_lnv(forward, V, h)
    want, terms, _ = A.disk_derivative(lam, I, scale, w, V, points)
    gap_dev = float(np.abs(pairs[0][0][sel].astype(LD) - quot).max())
    gap_ref = float(np.abs(want - quot).max())
    print(f"{label}: n={lam.size} rings={scale.size} V={V}: dout_lnv worst / allowance = {worst:.3e}; against quotients of the device's "
          f"forward: device {gap_dev:.3e}, restatement {gap_ref:.3e}, ratio / 2 = {gap_dev / (2 * gap_ref):.3f}")
    assert worst <= 1.0 and gap_dev <= 2.0 * gap_ref


@pytest.mark.parametrize("n", [2, 3])
def test_shortest_grids(ctx, n):
    lam = uniform(n, 6564.0, 6564.0 + 0.2 * (n - 1))
    scale, w = rings(3)
    I = spectra(lam, scale) * np.linspace(1.0, 2.0, n)[None, :]
    for V in (0.5, 9.0, 40.0):  # under one spacing, about one spacing, over
        adjoint_against_restatement(ctx, "shortest", lam, I, scale, w, V)
        derivative_against_restatement(ctx, "shortest", lam, I, scale, w, V, reference=I[::-1].copy())


def test_one_ring_and_a_ring_at_the_centre(ctx):
    lam = jittered(150)
    f = spectra(lam, np.array([0.7]))
    adjoint_against_restatement(ctx, "one ring", lam, f, np.array([0.7]), np.array([1.3]), 25.0)
    derivative_against_restatement(ctx, "one ring", lam, f, np.array([0.7]), np.array([1.3]), 25.0)
    scale, w = np.array([0.0, 0.4, 1.0]), np.array([0.2, 0.5, 0.3])
    I = spectra(lam, scale, seed=1)
    adjoint_against_restatement(ctx, "ring_scale = 0", lam, I, scale, w, 25.0)
    derivative_against_restatement(ctx, "ring_scale = 0", lam, I, scale, w, 25.0)
    # the ring at the centre passes w_r u through, and contributes nothing to the derivative
    u = weights_over(150, 3)
    W = ops.disk_integrate_adjoint(lam, u, scale, w, 25.0, ctx=ctx)
    assert np.array_equal(W[0], w[0] * u)
    _, d = ops.disk_integrate(lam, I, scale, np.array([1.0, 0.0, 0.0]), 25.0, derivative=True, ctx=ctx)
    assert np.all(d == 0)


def test_every_window_truncated_at_both_ends(ctx):
    lam = jittered(120)
    scale, w = rings(4)
    I = spectra(lam, scale, seed=3)
    V = 2900.0
    assert D.reaches(lam, V, scale.min()).min() > 0.5 * (lam[-1] - lam[0])
    adjoint_against_restatement(ctx, "truncated", lam, I, scale, w, V)
    derivative_against_restatement(ctx, "truncated", lam, I, scale, w, V, reference=2.0 - I)
    # a truncated window is renormalised by its own sum: a constant spectrum stays constant, its derivative is rounding
    _, d = ops.disk_integrate(lam, np.ones_like(I), scale, w, V, derivative=True, ctx=ctx)
    _, terms, _ = A.disk_derivative(lam, np.ones_like(I), scale, w, V)
    assert np.all(np.abs(d) <= DERIV_TOL * terms.astype(np.float64))


@pytest.mark.parametrize("shift", [-1, 0, 1], ids=["inside", "on", "outside"])
def test_a_node_on_a_rings_edge(ctx, shift):
    """as tests/test_gpu_disk_integration.py: the first node beyond point i's window for the ring of scale 1 one ulp inside, on, and one
    ulp outside the window's edge — the transpose alone (the singular density makes this the derivative's excluded case)"""
    lam = uniform(101)
    V, i = 30.0, 50
    edge = lam[i] + D.reaches(lam, V, 1.0)[i]
    j = int(np.searchsorted(lam, edge))
    lam[j] = edge if shift == 0 else np.nextafter(edge, np.inf if shift > 0 else -np.inf)
    assert lam[j - 1] < lam[j] < lam[j + 1]
    scale, w = np.array([1.0, 0.5]), np.array([0.6, 0.4])
    I = spectra(lam, scale, seed=4)
    adjoint_against_restatement(ctx, f"edge node ({shift:+d} ulp)", lam, I, scale, w, V)
    if shift >= 0:  # what lies beyond the edge does not reach point i: a weight on point i alone leaves node j + 1 of that ring untouched
        u = np.zeros(101)
        u[i] = 1.0
        W = ops.disk_integrate_adjoint(lam, u, scale, w, V, ctx=ctx)
        assert W[0, j + 1] == 0.0 and W[0, j - 1] != 0.0


@pytest.mark.parametrize("n_rings", [20, 64])
def test_short_windows_eight_lanes_per_point(ctx, n_rings):
    """n = 300, about 30 points in the widest window: the eight-lanes-per-point mapping; non-uniform grid"""
    lam = jittered(300)
    scale, w = rings(n_rings)
    I = spectra(lam, scale, seed=5)
    V = 22.0  # reach 0.48 A = 14.5 spacings
    points = list(range(300)) if n_rings == 20 else list(range(0, 300, 3)) + [298, 299]
    adjoint_against_restatement(ctx, "short windows", lam, I, scale, w, V, points=None if n_rings == 20 else points, with_nus=n_rings == 20)
    derivative_against_restatement(ctx, "short windows", lam, I, scale, w, V, points=points,
                                   reference=I[:, ::-1].copy() if n_rings == 20 else None)


def test_long_windows_a_wave_per_point(ctx):
    """n = 1200, about 400 points in the widest window: the wave-per-point mapping (the restatement on every 9th point and the ends: the
    adjoint's u is zero elsewhere, every node still gathers)"""
    lam = jittered(1200)
    scale, w = rings(20)
    I = spectra(lam, scale, seed=6)
    V = 76.0  # reach 1.66 A = 200 spacings
    points = sorted(set(range(0, 1200, 9)) | {1, 2, 1197, 1198, 1199})
    adjoint_against_restatement(ctx, "long windows", lam, I, scale, w, V, points=points, with_nus=False)
    derivative_against_restatement(ctx, "long windows", lam, I, scale, w, V, points=points)


def test_v_zero(ctx):
    lam = jittered(77)
    for n_rings in (1, 2, 5, 20, 64):
        scale, w = rings(n_rings)
        I = spectra(lam, scale, seed=n_rings)
        out, ref, d, dr = ops.disk_integrate(lam, I, scale, w, 0.0, reference=2.0 * I, derivative=True, ctx=ctx)
        assert np.array_equal(out, D.flux_order_sum(I, w)) and np.array_equal(ref, D.flux_order_sum(2.0 * I, w))
        assert np.all(d == 0) and np.all(dr == 0)
        u, ur = weights_over(77, 1), weights_over(77, 2)
        W, Wr = ops.disk_integrate_adjoint(lam, u, scale, w, 0.0, u_reference=ur, ctx=ctx)
        assert np.array_equal(W, w[:, None] * u[None, :]) and np.array_equal(Wr, w[:, None] * ur[None, :])
        nus = 2.99792458e18 / lam
        Wn = ops.disk_integrate_adjoint(lam, u, scale, w, 0.0, nus=nus, ctx=ctx)
        assert np.array_equal(Wn, (w[:, None] * u[None, :]) * nus[None, :] / lam[None, :])


def test_same_bits_twice_replayed_and_from_the_host_twin_and_a_graph_follows_the_velocity(ctx):
    lam = jittered(300)
    scale, w = rings(20)
    I, G = spectra(lam, scale, seed=8), spectra(lam, scale, seed=9)
    u, ur = weights_over(300, 4), weights_over(300, 5)
    n, ld = lam.size, lam.size + 4
    d_lam, d_s, d_w, d_I, d_G, d_u, d_ur = (ctx.upload(np.ascontiguousarray(a)) for a in (lam, scale, w, I, G, u, ur))
    d_rot = ctx.upload(np.array([10.0, 0.6]))
    out, out_ref, dl, dl_ref = (ctx.empty((n,)) for _ in range(4))
    W, W_ref = ctx.empty((20, ld)), ctx.empty((20, ld))

    def run():
        ctx.call("sdx_disk_integrate_deriv_dev", n, d_lam.ptr, 20, d_s.ptr, d_w.ptr, d_I.ptr, n, d_G.ptr, d_rot.ptr, out.ptr, out_ref.ptr, dl.ptr,
                 dl_ref.ptr)
        ctx.call("sdx_disk_integrate_adjoint_dev", n, d_lam.ptr, 20, d_s.ptr, d_w.ptr, d_rot.ptr, d_u.ptr, d_ur.ptr, None, W.ptr, ld, W_ref.ptr)

    result = lambda: [np.array(a.numpy()) for a in (out, out_ref, dl, dl_ref)] + [np.array(a.numpy())[:, :n] for a in (W, W_ref)]  # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    W.zero(), W_ref.zero()
    run()
    eager0 = result()
    assert np.all(np.array(W.numpy())[:, n:] == 0)  # (the padding of a row is not written)
    run()
    assert same(eager0, result())
    d_rot.set(np.array([23.7, 0.1]))
    run()
    eager1 = result()
    assert not any(np.array_equal(x, y) for x, y in zip(eager0, eager1))
    d_rot.set(np.array([10.0, 0.6]))
    graph = capture(ctx, run)
    try:
        for a in (out, out_ref, dl, dl_ref, W, W_ref):
            a.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        d_rot.set(np.array([23.7, 0.9]))  # no new capture: the kernels read V from device memory, and nothing but V
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    assert same(replay0, eager0) and same(replay1, eager1)
    host = list(ops.disk_integrate(lam, I, scale, w, 23.7, reference=G, derivative=True, ctx=ctx))
    host += list(ops.disk_integrate_adjoint(lam, u, scale, w, 23.7, u_reference=ur, ctx=ctx))
    assert same(host, eager1)
    assert np.array_equal(ops.disk_integrate(lam, I, scale, w, 10.0, ctx=ctx), eager0[0])


def test_refusals(ctx):
    lam = jittered(20)
    scale, w = rings(3)
    I = spectra(lam, scale)
    d_lam, d_s, d_w, d_I, d_u = (ctx.upload(np.ascontiguousarray(a)) for a in (lam, scale, w, I, weights_over(20, 0)))
    d_rot, out, dl, dl2 = ctx.upload(np.array([10.0, 0.6])), ctx.empty((20,)), ctx.empty((20,)), ctx.empty((20,))
    W, W2 = ctx.empty((3, 20)), ctx.empty((3, 20))
    L, S, Wt, Ip, R, O, U = d_lam.ptr, d_s.ptr, d_w.ptr, d_I.ptr, d_rot.ptr, out.ptr, d_u.ptr
    deriv = lambda *a: ctx.call("sdx_disk_integrate_deriv_dev", *a)  # noqa: E731
    deriv(20, L, 3, S, Wt, Ip, 20, None, R, O, None, dl.ptr, None)
    for bad in ((1, L, 3, S, Wt, Ip, 20, None, R, O, None, dl.ptr, None),        # n < 2
                (20, L, 0, S, Wt, Ip, 20, None, R, O, None, dl.ptr, None),       # no ring
                (20, L, 65, S, Wt, Ip, 20, None, R, O, None, dl.ptr, None),      # too many rings
                (20, L, 3, None, Wt, Ip, 20, None, R, O, None, dl.ptr, None),    # a null required pointer
                (20, L, 3, S, Wt, Ip, 20, None, None, O, None, dl.ptr, None),
                (20, L, 3, S, Wt, Ip, 20, None, R, O, None, None, None),         # no dout_lnv
                (20, L, 3, S, Wt, Ip, 19, None, R, O, None, dl.ptr, None),       # I_ld < n
                (20, L, 3, S, Wt, Ip, 20, Ip, R, O, None, dl.ptr, None),         # a reference without its output
                (20, L, 3, S, Wt, Ip, 20, None, R, O, None, dl.ptr, dl2.ptr),    # dout_lnv_reference without a reference
                (20, L, 3, S, Wt, Ip, 20, None, R, Ip, None, dl.ptr, None),      # in place
                (20, L, 3, S, Wt, Ip, 20, None, R, O, None, O, None),            # two outputs in one buffer
                (20, L, 3, S, Wt, Ip, 20, None, R, O, None, L, None)):
        with pytest.raises(ValueError):
            deriv(*bad)
    adj = lambda *a: ctx.call("sdx_disk_integrate_adjoint_dev", *a)  # noqa: E731
    adj(20, L, 3, S, Wt, R, U, None, None, W.ptr, 20, None)
    for bad in ((1, L, 3, S, Wt, R, U, None, None, W.ptr, 20, None),             # n < 2
                (20, L, 0, S, Wt, R, U, None, None, W.ptr, 20, None),            # no ring
                (20, L, 65, S, Wt, R, U, None, None, W.ptr, 20, None),           # too many rings
                (20, L, 3, S, None, R, U, None, None, W.ptr, 20, None),          # a null required pointer
                (20, L, 3, S, Wt, None, U, None, None, W.ptr, 20, None),
                (20, L, 3, S, Wt, R, None, None, None, W.ptr, 20, None),
                (20, L, 3, S, Wt, R, U, None, None, None, 20, None),
                (20, L, 3, S, Wt, R, U, None, None, W.ptr, 19, None),            # W_ld < n
                (20, L, 3, S, Wt, R, U, U, None, W.ptr, 20, None),               # a reference input without its output
                (20, L, 3, S, Wt, R, U, None, None, W.ptr, 20, W2.ptr),          # and the reverse
                (20, L, 3, S, Wt, R, U, None, None, U, 20, None),                # in place
                (20, L, 3, S, Wt, R, U, None, L, L, 20, None),
                (20, L, 3, S, Wt, R, U, U, None, W.ptr, 20, W.ptr)):             # two outputs in one buffer
        with pytest.raises(ValueError):
            adj(*bad)
    p = lambda a: a.ctypes.data  # noqa: E731
    res, res2, resW, u = np.empty(20), np.empty(20), np.empty((3, 20)), weights_over(20, 0)
    for lam_bad, scale_bad, v in ((lam[::-1].copy(), scale, 10.0), (lam, np.array([0.1, 0.5, 1.5]), 10.0), (lam, scale, -1.0)):
        with pytest.raises(ValueError):  # (the host twins' own checks, before any copy)
            ctx.call("sdx_disk_integrate_deriv_f64", 20, p(lam_bad), 3, p(scale_bad), p(w), p(I), None, v, p(res), None, p(res2), None)
        with pytest.raises(ValueError):
            ctx.call("sdx_disk_integrate_adjoint_f64", 20, p(lam_bad), 3, p(scale_bad), p(w), v, p(u), None, None, p(resW), None)
    with pytest.raises(ValueError):
        ops.disk_integrate_adjoint(lam, u[:-1], scale, w, 10.0, ctx=ctx)
