"""Rotational broadening on the device (k_rotate, k_rotate_adjoint_den, k_rotate_adjoint) against its longdouble restatement
(tests/rotation_reference.py): forward to ROT_TOL = 1e-11 of max |F| over the window, the adjoint per point to ROT_TOL of the sum of its
peak terms, the device's own dot identity to SUM_TOL of the sum of the absolute terms — every comparison also requires the compared
quantity to exceed ten times its allowance somewhere, so a zero cannot pass.  Then V = 0, a point exactly on the profile's edge, bits
across eager runs, graph replays and the host-buffer twins, the refusals, the Instrument with rotation, and the chain through
SpectralSynthesizer down to every line.  Figures are printed before they are asserted.  tests/test_rotation_cpu.py checks that every
grid / V pair below keeps clear of the profile's square-root edge."""
import ctypes as C

import numpy as np
import pytest

import line_adjoint_truth as A
import observe_adjoint_reference as aref
import observe_reference as oref
import rotation_reference as rref
from observe_reference import FLUX_TOL
from rotation_reference import LD, ROT_TOL, SUM_TOL
from stardis_amd import _lib, ops, synth
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from stardis_amd.postprocess import DeviceSpectrum
from test_gpu_response import FLUX_PARITY, H, profiled, scaled, small_model, synthesizer, thicken

pytestmark = pytest.mark.gpu

LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform
IRREGULAR = np.sort(np.random.default_rng(7).uniform(6500.0, 6600.0, 3000))
TWO_DENSITY = np.r_[np.linspace(6500.0, 6550.0, 500, endpoint=False), np.linspace(6550.0, 6600.0, 4000)]
GRIDS = {"S-c2": LAM, "irregular": IRREGULAR, "two-density": TWO_DENSITY}
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)


def vectors(lam, seed=11):
    """-> flux, reference, u (signed), u_reference (signed)"""
    rng = np.random.default_rng(seed)
    return 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0), rng.standard_normal(lam.size), rng.standard_normal(lam.size)


def dev_rotate(ctx, lam, flux, V, eps, reference=None):
    """sdx_rotate_dev on uploaded arrays, the pair through device memory -> (out, out_reference or None) as host arrays"""
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_f, d_g, d_rot = up(lam), up(flux), up(reference), up(np.array([V, eps]))
    out, out_ref = ctx.empty((lam.size,)), None if reference is None else ctx.empty((lam.size,))
    ctx.call("sdx_rotate_dev", lam.size, d_lam.ptr, d_f.ptr, _lib.ptr_of(d_g), d_rot.ptr, out.ptr, _lib.ptr_of(out_ref))
    ctx.synchronize()
    return np.array(out.numpy()), None if out_ref is None else np.array(out_ref.numpy())


def dev_adjoint(ctx, lam, u, V, eps, u_reference=None, nus=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_u, d_ur, d_nus, d_rot = up(lam), up(u), up(u_reference), up(nus), up(np.array([V, eps]))
    w, w_ref = ctx.empty((lam.size,)), None if u_reference is None else ctx.empty((lam.size,))
    ctx.call("sdx_rotate_adjoint_dev", lam.size, d_lam.ptr, d_rot.ptr, d_u.ptr, _lib.ptr_of(d_ur), _lib.ptr_of(d_nus), w.ptr, _lib.ptr_of(w_ref))
    ctx.synchronize()
    return np.array(w.numpy()), None if w_ref is None else np.array(w_ref.numpy())


def held(tag, got, ref, scale, tol=ROT_TOL):
    err, allow = np.abs(got.astype(LD) - ref).astype(np.float64), tol * scale.astype(np.float64)
    print(f"{tag}: {ref.size} points, worst |device - restatement| / allowance {float(np.max(err / allow)):.3e}, largest |value| / allowance "
          f"{float(np.max(np.abs(ref).astype(np.float64) / allow)):.3e}")
    assert np.all(np.isfinite(got)) and np.all(allow > 0)
    assert np.all(err <= allow)
    assert np.any(np.abs(ref).astype(np.float64) > 10 * allow)


def check_forward(ctx, tag, lam, V, epsilons=(0.0, 0.6, 1.0)):
    f, g, _, _ = vectors(lam)
    for eps in epsilons:
        out, out_ref = dev_rotate(ctx, lam, f, V, eps, reference=g)
        alone, _ = dev_rotate(ctx, lam, f, V, eps)
        r_out, r_ref, scale, scale_ref = rref.rotate(lam, f, V, eps, reference=g)
        held(f"{tag}, V = {V}, eps = {eps}: out", out, r_out, scale)
        held(f"{tag}, V = {V}, eps = {eps}: out_reference", out_ref, r_ref, scale_ref)
        assert np.array_equal(alone, out)  # the flux does not depend on whether a reference goes along


# ---- 1: forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [0.2, 2.0, 9.0, 9.6, 9.7, 19.3, 211.0])
def test_forward_on_the_sc2_grid(ctx, V):
    """windows of 1, 7, <= 32 (eight lanes), 33 (the estimate straddles the switch within the grid at 9.6 and lies just past it at
    9.7), 65 (one trip past a wave) and 704 points (11 trips per lane)"""
    n = rref.window_lengths(LAM, V)
    expected = 2 * V / K.C_KMS * LAM * (LAM.size - 1) / (LAM[-1] - LAM[0])
    print(f"V = {V}: windows of {n.min()} .. {n.max()} points, the mapping's estimate {expected.min():.2f} .. {expected.max():.2f}")
    assert n.max() == {0.2: 1, 2.0: 7, 9.7: 33, 19.3: 65, 211.0: 704}.get(V, n.max()) and (V != 9.0 or n.max() <= 32)
    if V == 9.0:
        assert expected.max() <= 32  # eight lanes per point everywhere
    if V == 9.6:
        assert expected.min() <= 32 < expected.max()  # both mappings in one launch
    if V == 9.7:
        assert 32 < expected.min() < 33  # a wave per point, just past the switch
    check_forward(ctx, "S-c2", LAM, V)
    if V == 0.2:  # every window is the point alone: (K h F) / (K h), two roundings
        f = vectors(LAM)[0]
        out, _ = dev_rotate(ctx, LAM, f, V, 0.6)
        assert np.max(np.abs(out / f - 1)) <= 3e-16


@pytest.mark.parametrize("grid", ["irregular", "two-density"])
@pytest.mark.parametrize("V", [23.7, 100.0])
def test_forward_on_other_grids(ctx, grid, V):
    """the mean-spacing estimate is wrong locally; either mapping must serve any point"""
    lam = GRIDS[grid]
    n = rref.window_lengths(lam, V)
    expected = 2 * V / K.C_KMS * lam * (lam.size - 1) / (lam[-1] - lam[0])
    print(f"{grid}, V = {V}: windows of {n.min()} .. {n.max()} points against an estimate of {expected.min():.1f} .. {expected.max():.1f}")
    check_forward(ctx, grid, lam, V, epsilons=(0.6,))


def test_forward_on_small_grids(ctx):
    """n = 2, 3, 9 with every window truncated at an end (or both), and n that is no multiple of the group of 8"""
    cases = [(f"n = {n}, every window truncated", 6560.0 + 0.013 * np.arange(n) ** 1.1, 40.0) for n in (2, 3, 9)]
    cases += [(f"n = {n}", 6560.0 * np.exp(np.arange(n) / 4.1e5), V) for n, V in ((13, 3.0), (77, 9.0), (1001, 30.0))]
    for tag, lam, V in cases:
        assert rref.clear_of_profile_edge(lam, V, 1e-8), tag
        n = rref.window_lengths(lam, V)
        if "truncated" in tag:
            assert np.all((lam * (1 - V / K.C_KMS) < lam[0]) | (lam * (1 + V / K.C_KMS) > lam[-1])) and n.max() == lam.size
        check_forward(ctx, tag, lam, V, epsilons=(0.0, 0.6))


# ---- 2: no rotation ------------------------------------------------------------------------------------------------------------------
def test_zero_velocity_is_a_copy_and_no_rotation_launches_nothing(ctx):
    f, g, u, _ = vectors(LAM)
    for V in (0.0, -5.0, np.nan):
        out, out_ref = dev_rotate(ctx, LAM, f, V, 0.6, reference=g)
        assert np.array_equal(out, f) and np.array_equal(out_ref, g), V
        assert np.array_equal(dev_adjoint(ctx, LAM, u, V, 0.6)[0], u), V
    plain, still = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx), Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_rot=0.0)
    assert not plain.rotates and still.rotates and not hasattr(plain, "d_rot") and plain._scratch is None
    d_lam, d_f, d_g, d_c = (ctx.upload(a) for a in (LAM, f, g, np.random.default_rng(1).standard_normal(2048)))
    with profiled(ctx):
        a = np.array(plain.observe(d_lam, d_f, LAM.size, d_g).numpy())
        wa = np.array(plain.adjoint(d_lam, LAM.size, d_c).numpy())
        ctx.synchronize()
        counts = {k: ctx.profile(k)[0] for k in ("k_rotate", "k_rotate_adjoint", "k_observe", "k_observe_adjoint")}
        print(f"an instrument without v_rot: {counts}")
        assert counts == {"k_rotate": 0, "k_rotate_adjoint": 0, "k_observe": 1, "k_observe_adjoint": 1}
        b = np.array(still.observe(d_lam, d_f, LAM.size, d_g).numpy())
        wb = np.array(still.adjoint(d_lam, LAM.size, d_c).numpy())
        ctx.synchronize()
        assert ctx.profile("k_rotate")[0] == 1 and ctx.profile("k_rotate_adjoint")[0] == 1
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(wa, wb) and not np.isnan(a).all() and wa.any()
    assert np.array_equal(ops.observe(LAM, f, SC2_EDGES, plain.sigma, ctx=ctx), ops.observe(LAM, f, SC2_EDGES, plain.sigma, ctx=ctx, v_rot=0.0), equal_nan=True)
    with pytest.raises(RuntimeError, match="no rotation"):
        plain.set_rotation(5.0)
    with pytest.raises(RuntimeError, match="no rotation"):
        plain.rotate(d_lam, d_f, LAM.size)


# ---- 3: a point on the edge ----------------------------------------------------------------------------------------------------------
def test_a_point_exactly_on_the_profile_edge(ctx):
    """an EXACTLY log-uniform grid — 4096 (1 + 2^-8)^i, seven points whose products are exact in fp64 — and V = c ((1 + 2^-8)^m - 1), so
    that lam_{i+m} = hi_i up to the rounding of V / c for every i: whether that point is included hinges on one rounding, and its term is
    sqrt(few ulp) ~ 2e-8 of the peak when it is — so the forward is held to 1e-7 of max |F| only; the dot identity still holds to
    SUM_TOL, because the adjoint includes a pair exactly when the forward did"""
    lam = 4096.0 * (1.0 + 2.0 ** -8) ** np.arange(7)
    assert np.array_equal(lam[1:].astype(LD), lam[:-1].astype(LD) * (1 + LD(2.0) ** -8))  # exact
    for m in (1, 2):
        V = float(((1.0 + 2.0 ** -8) ** m - 1.0) * K.C_KMS)
        margin = rref.profile_edge_margin(lam, V)
        print(f"m = {m}, V = {V!r}: margin {margin:.2e}")
        assert margin < 1e-15 and V < 3000.0
        on_the_edge(ctx, lam, V)


def on_the_edge(ctx, lam, V):
    f, g, u, u_ref = vectors(lam)
    for eps in (0.0, 0.6):
        out, _ = dev_rotate(ctx, lam, f, V, eps)
        r_out, _, scale, _ = rref.rotate(lam, f, V, eps)
        held(f"on the edge, eps = {eps}", out, r_out, scale, tol=1e-7)
        w, _ = dev_adjoint(ctx, lam, u, V, eps)
        terms = rref.dot_terms(lam, u, f, V, eps)
        lhs, rhs = float(np.sum(out.astype(LD) * u)), float(np.sum(w.astype(LD) * f))
        print(f"on the edge, eps = {eps}: <rotate(f), u> = {lhs:.15e}, <f, adjoint(u)> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * terms):.3e}")
        assert abs(lhs - rhs) <= SUM_TOL * terms and abs(lhs) > 10 * SUM_TOL * terms


# ---- 4: the adjoint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,V", [("S-c2", 2.0), ("S-c2", 9.0), ("S-c2", 9.7), ("S-c2", 19.3), ("S-c2", 211.0), ("irregular", 23.7), ("irregular", 100.0),
                                    ("two-density", 23.7), ("two-density", 100.0)])
def test_adjoint(ctx, grid, V):
    lam, eps = GRIDS[grid], 0.6
    f, g, u, u_ref = vectors(lam)
    nus = K.C_CGS * 1.0e8 / lam
    out, out_ref = dev_rotate(ctx, lam, f, V, eps, reference=g)
    terms, terms_ref = rref.dot_terms(lam, u, f, V, eps), rref.dot_terms(lam, u_ref, g, V, eps)
    r_w, r_wr, scale, scale_ref = rref.adjoint(lam, u, V, eps, u_reference=u_ref)
    k = (nus / lam).astype(LD)
    for nus_on in (False, True):
        mode = f"{grid}, V = {V}{', nus' if nus_on else ''}"
        w, w_ref = dev_adjoint(ctx, lam, u, V, eps, u_reference=u_ref, nus=nus if nus_on else None)
        alone, _ = dev_adjoint(ctx, lam, u, V, eps, nus=nus if nus_on else None)
        assert np.array_equal(alone, w)
        held(mode + ": w", w, r_w * k if nus_on else r_w, scale * k if nus_on else scale)
        held(mode + ": w_reference", w_ref, r_wr * k if nus_on else r_wr, scale_ref * k if nus_on else scale_ref)
        back = (lam / nus if nus_on else np.ones(lam.size)).astype(LD)
        for tag, o, uu, ww, ff, tt in (("flux", out, u, w, f, terms), ("reference", out_ref, u_ref, w_ref, g, terms_ref)):
            lhs, rhs = float(np.sum(o.astype(LD) * uu)), float(np.sum(ww.astype(LD) * ff * back))
            print(f"{mode}, {tag}: <rotate(f), u> = {lhs:.15e}, <f, adjoint(u)> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * tt):.3e}")
            assert abs(lhs - rhs) <= SUM_TOL * tt and abs(lhs) > 10 * SUM_TOL * tt
    # every point lies in a window, its own: weights of one sign give a weight at every point
    positive, _ = dev_adjoint(ctx, lam, np.abs(u) + 0.1, V, eps)
    assert np.all(positive > 0)


# ---- 5: determinism, graphs, the host-buffer twins, the refusals -----------------------------------------------------------------------
def capture(ctx, run):
    ctx.call("sdx_graph_begin")
    try:
        run()
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    return graph


def test_bits_repeat_and_graphs_follow_rotation_and_velocity(ctx):
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_rot=19.3)
    f, g, _, _ = vectors(LAM)
    c = np.random.default_rng(5).standard_normal(2048)
    d_lam, d_c, d_f, d_g, d_nus = (ctx.upload(a) for a in (LAM, c, f, g, K.C_CGS * 1.0e8 / LAM))
    pix, w, w_ref = ctx.empty((2048,)), ctx.empty((LAM.size,)), ctx.empty((LAM.size,))

    def run():
        inst.observe(d_lam, d_f, LAM.size, reference=d_g, out=pix)
        inst.adjoint(d_lam, LAM.size, d_c, flux=d_f, reference=d_g, nus=d_nus, out=w, out_reference=w_ref)

    def result():
        return tuple(np.array(a.numpy()) for a in (pix, w, w_ref))

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    def at(v_rot, eps, v_rad):
        inst.set_rotation(v_rot, eps)
        inst.set_radial_velocity(v_rad)

    run()
    eager0 = result()
    run()
    assert same(eager0, result()) and all(np.nan_to_num(a).any() for a in eager0)
    at(55.0, 0.3, 30.0)
    run()
    eager1 = result()
    assert not np.array_equal(eager1[0], eager0[0], equal_nan=True) and not np.array_equal(eager1[1], eager0[1])
    at(19.3, 0.6, 0.0)
    graph = capture(ctx, run)  # (the scratch was sized by the eager runs: the capture allocates nothing)
    try:
        for a in (pix, w, w_ref):
            a.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        at(55.0, 0.3, 30.0)  # no new capture: the kernels read the pair and the factor from device memory
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    print(f"replay against eager: {[int(np.sum(a != b)) for a, b in zip(replay0, eager0)]} values differ, after set_rotation and "
          f"set_radial_velocity {[int(np.sum(a != b)) for a, b in zip(replay1, eager1)]} (NaN pixels count)")
    assert same(replay0, eager0) and same(replay1, eager1)
    # the host-buffer twins, stage by stage and through the instrument
    twin = inst.rotate_host(LAM, f, g)
    stage = dev_rotate(ctx, LAM, f, 55.0, 0.3, reference=g)
    assert np.array_equal(twin[0], stage[0]) and np.array_equal(twin[1], stage[1]) and np.array_equal(ops.rotate(LAM, f, 55.0, 0.3, ctx=ctx), stage[0])
    assert np.array_equal(inst.observe_host(LAM, f, g), eager1[0], equal_nan=True)
    host = inst.adjoint_host(LAM, c, flux=f, reference=g, nus=K.C_CGS * 1.0e8 / LAM)
    assert np.array_equal(host[0], eager1[1]) and np.array_equal(host[1], eager1[2])
    assert np.array_equal(ops.observe(LAM, f, SC2_EDGES, inst.sigma, v_rad=30.0, reference=g, ctx=ctx, v_rot=55.0, limb_darkening=0.3), eager1[0], equal_nan=True)
    assert np.array_equal(ops.observe_adjoint(LAM, c, SC2_EDGES, inst.sigma, v_rad=30.0, flux=f, reference=g, nus=K.C_CGS * 1.0e8 / LAM, ctx=ctx, v_rot=55.0,
                                              limb_darkening=0.3)[0], eager1[1])


def test_refusals_leave_the_context_serving(ctx):
    lib = ctx.lib
    lam = LAM[:500]
    f, g, u, _ = vectors(lam)
    n = lam.size
    expect, _ = dev_rotate(ctx, lam, f, 9.0, 0.6)
    expect_w, _ = dev_adjoint(ctx, lam, u, 9.0, 0.6)
    d = ctx.upload(lam)
    o = ctx.empty((n,))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with profiled(ctx):
        # (ctx, n, lambdas, flux, reference, rot_dev, out, out_reference)
        for args in ((1, d.ptr, d.ptr, None, d.ptr, o.ptr, None), (n, None, d.ptr, None, d.ptr, o.ptr, None), (n, d.ptr, None, None, d.ptr, o.ptr, None),
                     (n, d.ptr, d.ptr, None, None, o.ptr, None), (n, d.ptr, d.ptr, None, d.ptr, None, None), (n, d.ptr, d.ptr, None, d.ptr, d.ptr, None),
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, o.ptr, None), (n, d.ptr, d.ptr, None, d.ptr, o.ptr, o.ptr)):
            assert lib.sdx_rotate_dev(ctx.handle, *args) == -1 and b"rotate" in lib.sdx_last_error_string(), args
        # (ctx, n, lambdas, rot_dev, u, u_reference, nus, w, w_reference)
        for args in ((1, d.ptr, d.ptr, d.ptr, None, None, o.ptr, None), (n, None, d.ptr, d.ptr, None, None, o.ptr, None), (n, d.ptr, None, d.ptr, None, None, o.ptr, None),
                     (n, d.ptr, d.ptr, None, None, None, o.ptr, None), (n, d.ptr, d.ptr, d.ptr, None, None, None, None), (n, d.ptr, d.ptr, d.ptr, d.ptr, None, o.ptr, None),
                     (n, d.ptr, d.ptr, d.ptr, None, None, o.ptr, o.ptr)):
            assert lib.sdx_rotate_adjoint_dev(ctx.handle, *args) == -1 and b"rotate_adjoint" in lib.sdx_last_error_string(), args
        # the twins check what the kernels cannot, before any copy
        out = np.full(n, -7.0)
        for tag, kw in dict(lambdas=dict(lam=np.ascontiguousarray(lam[::-1])), nan_lambda=dict(lam=np.r_[lam[:-1], np.nan]), v_rot=dict(V=-1.0), fast=dict(V=3000.0),
                            nan_v=dict(V=np.nan), limb_darkening=dict(eps=1.01), negative_eps=dict(eps=-0.01), nan_eps=dict(eps=np.nan)).items():
            a = dict(dict(lam=lam, V=9.0, eps=0.6), **kw)
            rc = lib.sdx_rotate_f64(ctx.handle, n, p(a["lam"]), p(f), None, a["V"], a["eps"], p(out), None)
            msg = lib.sdx_last_error_string().decode()
            print(f"{tag}: rc {rc}, '{msg}'")
            assert rc == -1 and np.all(out == -7.0) and {"nan_lambda": "lambdas", "fast": "v_rot", "nan_v": "v_rot", "negative_eps": "limb_darkening",
                                                         "nan_eps": "limb_darkening"}.get(tag, tag) in msg
            assert lib.sdx_rotate_adjoint_f64(ctx.handle, n, p(a["lam"]), a["V"], a["eps"], p(u), None, None, p(out), None) == -1 and np.all(out == -7.0)
        ctx.synchronize()
        assert ctx.profile("k_rotate")[0] == 0 and ctx.profile("k_rotate_adjoint")[0] == 0
        assert np.array_equal(dev_rotate(ctx, lam, f, 9.0, 0.6)[0], expect) and np.array_equal(dev_adjoint(ctx, lam, u, 9.0, 0.6)[0], expect_w)
        assert ctx.profile("k_rotate")[0] == 1 and ctx.profile("k_rotate_adjoint")[0] == 1
    assert lib.sdx_rotate_f64(ctx.handle, n, p(lam), p(f), None, 9.0, 0.6, p(out), None) == 0 and np.array_equal(out, expect)


# ---- 6: the instrument ---------------------------------------------------------------------------------------------------------------
def test_instrument_with_rotation(ctx):
    lam = LAM[(LAM > 6530.0) & (LAM < 6570.0)]
    edges = np.linspace(6531.0, 6569.0, 401)
    f, g, _, _ = vectors(lam)
    c = np.random.default_rng(6).standard_normal(400)
    nus = K.C_CGS * 1.0e8 / lam
    V, eps, v_rad = 40.0, 0.6, 25.0
    assert rref.clear_of_profile_edge(lam, V, 1e-8)
    inst = Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=V, limb_darkening=eps)
    inst.set_radial_velocity(v_rad)
    assert oref.clear_of_grid_ends(lam, edges, inst.sigma, inst.doppler)
    rf, rg, _, _ = rref.rotate(lam, f, V, eps, reference=g)
    rf, rg = rf.astype(np.float64), rg.astype(np.float64)
    edge = inst.edge_affected(lam)
    for ref_on in (False, True):
        got = inst.observe_host(lam, f, g if ref_on else None)
        expect = oref.observe(lam, rf, edges, inst.sigma, inst.doppler, reference=rg if ref_on else None)
        ok = ~np.isnan(expect)
        err = np.abs(got[ok] - expect[ok]) / np.abs(expect[ok])
        print(f"observe_host{', reference' if ref_on else ''}: {ok.sum()} pixels, {int((ok & ~edge).sum())} clear of the grid's ends, worst relative difference {err.max():.3e}")
        assert np.array_equal(np.isnan(got), ~ok) and (ok & ~edge).sum() > 300 and edge.sum() > (~ok).sum()
        assert np.all(err[~edge[ok]] <= FLUX_TOL)
        # the transpose through both stages: <observe(rotate(f)), c> = <f, adjoint(c)>
        w = inst.adjoint_host(lam, c, flux=f if ref_on else None, reference=g if ref_on else None, nus=nus)
        w = w[0] if ref_on else w
        terms = aref.dot_terms(lam, c, rref.rotate(lam, np.abs(f), V, eps)[0].astype(np.float64), edges, inst.sigma, inst.doppler, reference=rg if ref_on else None)
        lhs, rhs = float(np.sum(c[ok] * got[ok])), float(np.sum(w.astype(LD) * f * lam / nus))
        print(f"adjoint_host{', normalised' if ref_on else ''}: <observe(f), c> = {lhs:.15e}, <f, adjoint(c)> = {rhs:.15e}, difference / allowance "
              f"{abs(lhs - rhs) / (2 * SUM_TOL * terms):.3e}")
        assert abs(lhs - rhs) <= 2 * SUM_TOL * terms and abs(lhs) > 20 * SUM_TOL * terms  # (two stages of reordered sums)


# ---- 7: the engine -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(ctx):
    """the small model of tests/test_gpu_response.py: 12 depths, 300 points, 40 lines, and species X's difference quotients"""
    m = thicken(ctx, small_model())
    flux = {}
    for h in (H, -H, H / 2, -H / 2):
        syn = synthesizer(ctx, m, scaled(m, np.exp(h)))
        syn.step()
        ctx.synchronize()
        flux[h] = np.array(syn.F_nu()[-1])
        syn.close()
    m.coarse, m.fine = (flux[H] - flux[-H]) / (2 * H), (flux[H / 2] - flux[-H / 2]) / H
    return m


def engine_instrument(ctx, v=12.0, v_rot=10.0):
    """one pixel that the 6560 - 6570 A grid covers but whose window comes within the rotation's reach of the grid's blue end, 24
    pixels clear of both ends, one off the red end; v_rot = 10 km/s is about 13 points per window"""
    inst = Instrument(np.r_[6560.75, np.linspace(6562.0, 6568.0, 25), 6571.0], sigma=0.05, ctx=ctx, v_rot=v_rot)
    inst.set_radial_velocity(v)
    return inst


STAGES = ("k_rotate", "k_rotate_adjoint", "k_observe", "k_observe_adjoint", "k_flux_nu_to_lambda", "k_line_adjoint", "k_response_weight", "k_raytrace")


def counts(ctx):
    ctx.synchronize()
    return {k: ctx.profile(k)[0] for k in STAGES}


def test_engine_chain_with_rotation(ctx, model):
    m = model
    n_depth, n_nu, n_lines, n_pix = 12, 300, 40, 26
    lam = K.nu_to_angstrom(m.nus)
    n_win = rref.window_lengths(lam, 10.0)
    assert 12 <= n_win.max() <= 14 and rref.clear_of_profile_edge(lam, 10.0, 1e-8)
    inst, plain = engine_instrument(ctx), engine_instrument(ctx, v_rot=None)
    edge = inst.edge_affected(lam)
    assert edge.tolist() == [True] + [False] * 24 + [True]
    syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=inst)
    ref_syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=plain)
    with profiled(ctx):
        ref_syn.step()
        before = counts(ctx)
    with profiled(ctx):
        syn.step()
        after = counts(ctx)
        print(f"launches of a step without rotation {before}\n                   with rotation {after}")
        assert after == dict(before, k_rotate=1) and before["k_rotate"] == 0 and after["k_observe"] == 2 and after["k_rotate_adjoint"] == 0
        c = np.random.default_rng(5).standard_normal(n_pix)
        c[-1] = np.nan  # the pixel off the grid's end: never read
        sens = syn.observed_line_sensitivities(c)
        on_demand = counts(ctx)
        assert on_demand["k_rotate_adjoint"] == 1 and on_demand["k_observe_adjoint"] == 1 and on_demand["k_line_adjoint"] == 1 and on_demand["k_rotate"] == 1
    sens = np.array(sens.numpy())

    # observed and observed_normalized against the restatements
    F, Fc = np.array(syn.F_nu()[-1]), np.array(syn.F_nu_continuum[-1])
    f_lam, g_lam = F * m.nus / lam, Fc * m.nus / lam
    rf, rg, _, _ = rref.rotate(lam, f_lam, 10.0, 0.6, reference=g_lam)
    rf, rg = rf.astype(np.float64), rg.astype(np.float64)
    observed, normalized = np.array(syn.observed.numpy()), np.array(syn.observed_normalized.numpy())
    for tag, got, expect in (("observed", observed, oref.observe(lam, rf, inst.edges, inst.sigma, inst.doppler)),
                             ("observed_normalized", normalized, oref.observe(lam, rf, inst.edges, inst.sigma, inst.doppler, reference=rg))):
        ok = ~np.isnan(expect)
        err = np.abs(got[ok] - expect[ok]) / np.abs(expect[ok])
        print(f"engine, {tag}: worst relative difference {err.max():.3e}")
        assert ok.tolist() == [True] * 25 + [False] and np.array_equal(np.isnan(got), ~ok) and np.all(err <= FLUX_TOL)
    assert not np.array_equal(observed, np.array(ref_syn.observed.numpy()), equal_nan=True)  # the rotation really ran
    spec = DeviceSpectrum(syn)
    assert np.array_equal(spec.observed(inst).numpy(), observed, equal_nan=True)
    assert np.array_equal(spec.observed(inst, normalized=True).numpy(), normalized, equal_nan=True)

    # per line against the forward chain c . inst.observe(flux_derivative(single-line plane) nu / lambda), the rotation inside observe: the bound
    # of test_gpu_observe_adjoint.test_engine_chain and one more SUM_TOL for the rotation's reordered sums
    c0 = np.where(np.isnan(c), 0.0, c)
    w_abs = np.array(syn.pixel_weights_to_grid(np.abs(c0)).numpy())
    assert np.all(w_abs >= 0) and w_abs.any()
    Ra, total = np.array(syn.response_opacity.numpy()), np.array(syn.total_alphas())
    d_lam = ctx.upload(lam)
    push = lambda a: np.array(inst.observe(d_lam, ctx.upload(np.ascontiguousarray(a)), n_nu, out=ctx.empty((n_pix,))).numpy())[:-1]  # noqa: E731
    worst, seen = 0.0, False
    for l in range(n_lines):
        one = [np.ascontiguousarray(m.lines[k][l:l + 1]) for k in ("line_nus", "doppler_widths", "gammas", "alphas")]
        plane = ops.calc_alan_entries(n_depth, m.nus, *one, ctx=ctx)
        expect = float(np.sum(c0[:-1] * push(np.array(syn.flux_derivative(plane).numpy()) * m.nus / lam)))
        allowed = (2 * A.OPACITY_RTOL + n_depth * n_nu * A.EPS + 2 * SUM_TOL) * float(np.abs(w_abs[None, :] * Ra * (plane / total)).sum())
        assert abs(sens[l] - expect) <= allowed, (l, sens[l], expect, allowed)
        worst = max(worst, abs(sens[l] - expect) / allowed) if allowed > 0 else worst
        seen |= abs(sens[l]) > 10 * allowed
    print(f"observed_line_sensitivities against the forward chain per line: worst difference / bound {worst:.3e}")
    assert seen

    # species X against difference quotients of whole syntheses, pushed through the rotating instrument
    extrapolated = float(np.sum(c0[:-1] * (4 * push(m.fine * m.nus / lam) - push(m.coarse * m.nus / lam)) / 3))
    allowance = float(np.sum(np.abs(c0[:-1]) * push((np.abs(m.coarse - m.fine) + FLUX_PARITY * np.abs(F).max() / H) * m.nus / lam)))
    value = float(sens[m.x_lines].sum())
    print(f"species X: sum of its lines' sensitivities {value:+.6e}, Richardson value of the difference quotients {extrapolated:+.6e}, allowance {allowance:.3e}")
    assert abs(value - extrapolated) <= allowance and abs(value) > 10 * allowance

    # chi-square: the NaN pixel, the pixel without weight AND the edge-affected pixel are left out
    rng = np.random.default_rng(8)
    for norm_on in (False, True):
        obs = normalized if norm_on else observed
        data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(n_pix))
        ivar = rng.uniform(0.5, 2.0, n_pix) / np.nanmax(np.abs(obs)) ** 2
        ivar[3] = 0.0
        use = ~np.isnan(obs) & (ivar != 0) & ~edge
        assert use.sum() == 23 and not np.isnan(obs[0]) and ivar[0] != 0
        chi2, grad = syn.chi2_line_gradient(data, ivar, normalized=norm_on)
        r, w = np.where(use, data, 0.0) - np.where(use, obs, 0.0), np.where(use, ivar, 0.0)
        expect = float(np.sum(w * r * r))
        print(f"normalized = {norm_on}: chi2 {chi2!r} against numpy {expect!r}")
        assert chi2 == expect and chi2 > 0
        assert np.array_equal(grad.numpy(), syn.observed_line_sensitivities(-2.0 * w * r, normalized=norm_on).numpy()) and np.array(grad.numpy()).any()
    # the normalised weights through both stages: their dot identity on the device
    cn = rng.standard_normal(n_pix)
    wn = np.array(syn.pixel_weights_to_grid(cn, normalized=True).numpy())
    terms = aref.dot_terms(lam, cn, rref.rotate(lam, np.abs(f_lam), 10.0, 0.6)[0].astype(np.float64), inst.edges, inst.sigma, inst.doppler, reference=rg)
    lhs, rhs = float(np.sum(cn[:-1] * normalized[:-1])), float(wn @ F)
    print(f"normalised: <observed_normalized, c> = {lhs:.15e}, <F_nu, weights> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (2 * SUM_TOL * terms):.3e}")
    assert abs(lhs - rhs) <= 2 * SUM_TOL * terms and abs(lhs) > 20 * SUM_TOL * terms
    # a captured step replays the rotation and follows set_rotation
    syn.capture()
    try:
        syn.d_observed.zero()
        syn.step()
        assert np.array_equal(syn.observed.numpy(), observed, equal_nan=True)
        inst.set_rotation(25.0)
        syn.step()
        moved = np.array(syn.observed.numpy())
    finally:
        syn._destroy_graphs()
    expect = oref.observe(lam, rref.rotate(lam, f_lam, 25.0, 0.6)[0].astype(np.float64), inst.edges, inst.sigma, inst.doppler)
    assert not np.array_equal(moved, observed, equal_nan=True) and np.all(np.abs(moved[:-1] - expect[:-1]) <= FLUX_TOL * np.abs(expect[:-1]))
    syn.close()
    ref_syn.close()
