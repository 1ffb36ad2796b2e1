"""Disk integration with rigid rotation on the device (sdx_disk_integrate_dev, sdx_disk_integrate_f64, ops.disk_integrate) against its
longdouble restatement (tests/disk_integration_reference.py, itself pinned by tests/test_disk_integration_cpu.py).

Tolerance: 1e-11 of sum_r |w_r| max_window |I_r| per point — the project's tolerance for k_rotate_integrated (rotation_reference.ROT_TOL)
carried over the ring sum.  Every comparison prints its worst figure in units of that allowance before it asserts.  V = 0, two calls, a
graph replay and the host-buffer twin are compared bit for bit."""
import numpy as np
import pytest

import disk_integration_reference as D
import formal_solution_truth as T
from stardis_amd import constants as K
from stardis_amd import ops, synth
from test_gpu_observe_tangent import capture

pytestmark = pytest.mark.gpu

LD = D.LD


@pytest.fixture(autouse=True)
def extended_precision():
    if not D.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def uniform(n, lo=6560.0, hi=6570.0):
    return np.linspace(lo, hi, n)


def jittered(n, seed=7):
    rng = np.random.default_rng(seed)
    return np.sort(6560.0 + 10.0 * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n)


def rings(n_rings):
    """the field's own angles: Gauss-Legendre nodes in theta -> (ring_scale = sin theta, flux weights)"""
    thetas, weights = synth.thetas_and_weights(n_rings)
    return np.sin(thetas), np.asarray(weights, dtype=np.float64)


def spectra(lam, scale, seed=0):
    """per-ring spectra that differ in continuum, line depth and line width: limb-darkened continuum, lines that weaken to the limb"""
    rng = np.random.default_rng(seed)
    mu = np.sqrt((1.0 - scale) * (1.0 + scale))[:, None]
    mid, span = 0.5 * (lam[0] + lam[-1]), lam[-1] - lam[0]
    x = (lam[None, :] - mid) / span
    return (0.4 + 0.6 * mu) * (1.0 - (0.3 + 0.4 * mu) * np.exp(-0.5 * (x / (0.02 + 0.01 * mu)) ** 2)
                               - 0.2 * np.exp(-0.5 * ((x - 0.11) / 0.035) ** 2)) * (1.0 + 1e-3 * rng.standard_normal((scale.size, lam.size)))


def against_restatement(ctx, label, lam, I, scale, w, V, reference=None, points=None):
    got = ops.disk_integrate(lam, I, scale, w, V, reference=reference, ctx=ctx)
    pairs = [(got, I)] if reference is None else [(got[0], I), (got[1], reference)]
    worst = 0.0
    for out, planes in pairs:
        assert out.shape == lam.shape and np.all(np.isfinite(out))
        want, allow = D.disk_integrate(lam, planes, scale, w, V, points)
        sel = slice(None) if points is None else np.asarray(points)
        err = np.abs(out[sel].astype(LD) - want) / (D.ROT_TOL * allow)
        worst = max(worst, float(err.max()))
    print(f"{label}: n={lam.size} rings={scale.size} V={V}: worst |device - restatement| / allowance = {worst:.3e}")
    assert worst <= 1.0
    return worst


@pytest.mark.parametrize("n", [2, 3])
def test_shortest_grids(ctx, n):
    lam = uniform(n, 6564.0, 6564.0 + 0.2 * (n - 1))
    scale, w = rings(3)
    I = spectra(lam, scale) * np.linspace(1.0, 2.0, n)[None, :]
    for V in (0.5, 9.0, 40.0):  # under one spacing, about one spacing, every window truncated
        against_restatement(ctx, "shortest", lam, I, scale, w, V, reference=I[::-1].copy())


def test_one_ring_and_a_ring_at_the_centre(ctx):
    lam = jittered(150)
    f = spectra(lam, np.array([0.7]))
    against_restatement(ctx, "one ring", lam, f, np.array([0.7]), np.array([1.3]), 25.0)
    scale, w = np.array([0.0, 0.4, 1.0]), np.array([0.2, 0.5, 0.3])
    I = spectra(lam, scale, seed=1)
    against_restatement(ctx, "ring_scale = 0", lam, I, scale, w, 25.0)
    # the ring at the centre is a copy: with all the weight on it the result is its spectrum bit for bit
    assert np.array_equal(ops.disk_integrate(lam, I, scale, np.array([1.0, 0.0, 0.0]), 25.0, ctx=ctx), I[0])


def test_windows_under_one_spacing_and_continuity(ctx):
    lam = jittered(200)
    scale, w = rings(5)
    I = spectra(lam, scale, seed=2)
    flat = ops.disk_integrate(lam, I, scale, w, 0.0, ctx=ctx)
    gaps = []
    for V in (0.5, 5e-2, 5e-3, 5e-4):  # the smallest spacing is 0.02 A = 0.9 km/s: every window under one spacing, three weights each
        against_restatement(ctx, "under one spacing", lam, I, scale, w, V)
        gaps.append(float(np.max(np.abs(ops.disk_integrate(lam, I, scale, w, V, ctx=ctx) - flat))))
    print("distance from the flux sum as V shrinks:", gaps)
    assert gaps[0] > gaps[1] > gaps[2] > gaps[3] > 0 and gaps[3] <= 2e-3 * gaps[0]  # (linear in V under one spacing)


def test_every_window_truncated_at_both_ends(ctx):
    lam = jittered(120)
    scale, w = rings(4)
    I = spectra(lam, scale, seed=3)
    V = 2900.0  # reach 63 A at scale 1, 10 A of grid; the innermost ring (scale 0.11) still reaches 7 A: truncated for most points
    assert D.reaches(lam, V, scale.min()).min() > 0.5 * (lam[-1] - lam[0])
    against_restatement(ctx, "truncated", lam, I, scale, w, V, reference=2.0 - I)
    # a truncated window is renormalised by its own sum: a constant spectrum stays constant
    out = ops.disk_integrate(lam, np.ones_like(I), scale, w, V, ctx=ctx)
    assert np.max(np.abs(out - w.sum())) <= 1e-13 * w.sum()


@pytest.mark.parametrize("shift", [-1, 0, 1], ids=["inside", "on", "outside"])
def test_a_node_on_a_rings_edge(ctx, shift):
    """the first node beyond point i's window for the ring of scale 1 is moved onto the window's edge: one ulp inside, exactly on, one ulp
    outside.  The arcsine density is singular there — the ulp inside already holds sqrt(2 ulp / reach) / pi = 5e-7 of the mass —, the
    cell beyond the edge has zero length."""
    lam = uniform(101)
    V, i = 30.0, 50
    edge = lam[i] + D.reaches(lam, V, 1.0)[i]
    j = int(np.searchsorted(lam, edge))
    lam[j] = edge if shift == 0 else np.nextafter(edge, np.inf if shift > 0 else -np.inf)
    assert lam[j - 1] < lam[j] < lam[j + 1]
    scale, w = np.array([1.0, 0.5]), np.array([0.6, 0.4])
    I = spectra(lam, scale, seed=4)
    against_restatement(ctx, f"edge node ({shift:+d} ulp)", lam, I, scale, w, V)
    if shift >= 0:  # what lies beyond the edge does not reach point i: a spike on the next node changes nothing there
        spiked = I.copy()
        spiked[0, j + 1] += 100.0
        a, b = (ops.disk_integrate(lam, x, scale[:1], w[:1], V, ctx=ctx) for x in (I[:1], spiked[:1]))
        assert a[i] == b[i] and a[i + 2] != b[i + 2]


def test_linear_spectrum_is_reproduced(ctx):
    lam = jittered(160)
    scale, w = rings(6)
    slope = np.linspace(-0.3, 0.4, 6)[:, None]
    I = 2.0 + slope * (lam[None, :] - 6565.0)
    V = 20.0
    out = ops.disk_integrate(lam, I, scale, w, V, ctx=ctx)
    reach = D.reaches(lam, V, 1.0)
    interior = (lam - reach >= lam[0]) & (lam + reach <= lam[-1])
    want = (w[:, None] * I).sum(axis=0)
    err = np.abs(out - want)[interior] / (np.abs(w)[:, None] * np.abs(I)).sum(axis=0)[interior]
    print(f"linear spectra at {int(interior.sum())} interior points: {err.max():.3e}")
    assert interior.sum() > 100 and err.max() <= D.ROT_TOL


@pytest.mark.parametrize("n_rings", [20, 64])
def test_short_windows_eight_lanes_per_point(ctx, n_rings):
    """n = 300, about 30 points in the widest window: the eight-lanes-per-point mapping; non-uniform grid; with and without reference"""
    lam = jittered(300)
    scale, w = rings(n_rings)
    I = spectra(lam, scale, seed=5)
    V = 22.0  # reach 0.48 A = 14.5 spacings
    points = list(range(300)) if n_rings == 20 else list(range(0, 300, 3)) + [298, 299]
    against_restatement(ctx, "short windows", lam, I, scale, w, V, points=points)
    if n_rings == 20:
        against_restatement(ctx, "short windows, reference", lam, I, scale, w, V, reference=I[:, ::-1].copy(), points=list(range(0, 300, 5)))


def test_long_windows_a_wave_per_point(ctx):
    """n = 1200, about 400 points in the widest window: the wave-per-point mapping (the restatement on every 9th point and the ends)"""
    lam = jittered(1200)
    scale, w = rings(20)
    I = spectra(lam, scale, seed=6)
    V = 76.0  # reach 1.66 A = 200 spacings
    points = sorted(set(range(0, 1200, 9)) | {1, 2, 1197, 1198, 1199})
    against_restatement(ctx, "long windows", lam, I, scale, w, V, reference=1.0 + 0.0 * I, points=points)


def test_v_zero_is_the_flux_sum_bit_for_bit(ctx):
    lam = jittered(77)
    for n_rings in (1, 2, 5, 20, 64):
        scale, w = rings(n_rings)
        I = spectra(lam, scale, seed=n_rings)
        out, ref = ops.disk_integrate(lam, I, scale, w, 0.0, reference=2.0 * I, ctx=ctx)
        assert np.array_equal(out, D.flux_order_sum(I, w)) and np.array_equal(ref, D.flux_order_sum(2.0 * I, w))


def test_v_zero_on_emergent_intensities_is_the_flux_of_the_plain_kernel(ctx):
    c = T.case(5, 20, per_class=4)
    ctx.set_option("segmented_raytrace", 0)
    try:
        F, _ = ops.raytrace_arrays(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx)
    finally:
        ctx.set_option("segmented_raytrace", -1)
    I = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx)
    d = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (K.nu_to_angstrom(c.nus), np.sin(c.thetas), c.weights, I, [0.0, 0.0])]
    out = ctx.empty((c.n_nu,))
    ctx.call("sdx_disk_integrate_dev", c.n_nu, d[0].ptr, 20, d[1].ptr, d[2].ptr, d[3].ptr, c.n_nu, None, d[4].ptr, out.ptr, None)
    got = out.numpy()
    print(f"{c.n_nu} hostile columns, {int(np.isfinite(F[-1]).sum())} with a finite flux")
    assert np.array_equal(got, F[-1], equal_nan=True) and np.isfinite(F[-1]).any() and np.any(F[-1][np.isfinite(F[-1])] != 0)


def test_same_bits_twice_replayed_and_from_the_host_twin_and_a_graph_follows_the_velocity(ctx):
    lam = jittered(300)
    scale, w = rings(20)
    I, G = spectra(lam, scale, seed=8), spectra(lam, scale, seed=9)
    n = lam.size
    d_lam, d_s, d_w, d_I, d_G = (ctx.upload(np.ascontiguousarray(a)) for a in (lam, scale, w, I, G))
    d_rot = ctx.upload(np.array([10.0, 0.6]))
    out, out_ref = ctx.empty((n,)), ctx.empty((n,))
    run = lambda: ctx.call("sdx_disk_integrate_dev", n, d_lam.ptr, 20, d_s.ptr, d_w.ptr, d_I.ptr, n, d_G.ptr, d_rot.ptr, out.ptr, out_ref.ptr)  # noqa: E731
    result = lambda: (np.array(out.numpy()), np.array(out_ref.numpy()))  # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    run()
    eager0 = result()
    run()
    assert same(eager0, result())
    d_rot.set(np.array([23.7, 0.1]))  # (as Instrument.set_rotation rewrites the pair)
    run()
    eager1 = result()
    assert not any(np.array_equal(x, y) for x, y in zip(eager0, eager1))
    d_rot.set(np.array([10.0, 0.6]))
    graph = capture(ctx, run)
    try:
        out.zero(), out_ref.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        d_rot.set(np.array([23.7, 0.9]))  # no new capture: the kernel reads V from device memory, and nothing but V
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    assert same(replay0, eager0) and same(replay1, eager1)
    assert same(ops.disk_integrate(lam, I, scale, w, 23.7, reference=G, ctx=ctx), eager1)
    assert np.array_equal(ops.disk_integrate(lam, I, scale, w, 10.0, ctx=ctx), eager0[0])


def test_refusals(ctx):
    lam = jittered(20)
    scale, w = rings(3)
    I = spectra(lam, scale)
    d_lam, d_s, d_w, d_I = (ctx.upload(np.ascontiguousarray(a)) for a in (lam, scale, w, I))
    d_rot, out = ctx.upload(np.array([10.0, 0.6])), ctx.empty((20,))
    call = lambda *a: ctx.call("sdx_disk_integrate_dev", *a)  # noqa: E731
    call(20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, out.ptr, None)
    for bad in ((1, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, out.ptr, None),       # n < 2
                (20, d_lam.ptr, 0, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, out.ptr, None),      # no ring
                (20, d_lam.ptr, 65, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, out.ptr, None),     # too many rings
                (20, d_lam.ptr, 3, None, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, out.ptr, None),         # a null required pointer
                (20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, None, out.ptr, None),
                (20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 19, None, d_rot.ptr, out.ptr, None),      # I_ld < n
                (20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, d_I.ptr, d_rot.ptr, out.ptr, None),   # a reference without its output
                (20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, None, d_rot.ptr, d_I.ptr, None),      # in place
                (20, d_lam.ptr, 3, d_s.ptr, d_w.ptr, d_I.ptr, 20, d_I.ptr, d_rot.ptr, out.ptr, out.ptr)):
        with pytest.raises(ValueError):
            call(*bad)
    p = lambda a: a.ctypes.data  # noqa: E731
    res = np.empty(20)
    for lam_bad, scale_bad, v in ((lam[::-1].copy(), scale, 10.0), (lam, np.array([0.1, 0.5, 1.5]), 10.0), (lam, scale, -1.0)):
        with pytest.raises(ValueError):  # (the host twin's own checks, before any copy; ops.disk_integrate repeats them in Python)
            ctx.call("sdx_disk_integrate_f64", 20, p(lam_bad), 3, p(scale_bad), p(w), p(I), None, v, p(res), None)
