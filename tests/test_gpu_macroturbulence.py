"""Radial-tangential macroturbulence on the device (k_macroturbulence, k_macroturbulence_adjoint_den, k_macroturbulence_adjoint) against
its restatement (tests/macroturbulence_reference.py): forward and derivative outputs to MACRO_TOL = 1e-12 of max |F| over the window,
the derivative also against difference quotients of the device's own forward, the adjoint per point to MACRO_TOL of the sum of its peak
terms, the device's own dot identity to SUM_TOL of the sum of the absolute terms — every comparison also requires the compared quantity
to exceed ten times its allowance somewhere, so a zero cannot pass.  Then zeta = 0, bits across eager runs, graph replays and the
host-buffer twins, the refusals, the Instrument with both broadenings, and the chain through SpectralSynthesizer down to every line and
to d chi2 / d zeta.  Figures are printed before they are asserted.  tests/test_macroturbulence_cpu.py asserts the window lengths and
mapping estimates of the zeta used here."""
import ctypes as C

import numpy as np
import pytest

import line_adjoint_truth as A
import macroturbulence_reference as mref
import observe_adjoint_reference as aref
import observe_reference as oref
import rotation_reference as rref
from macroturbulence_reference import LD, MACRO_TOL, SUM_TOL
from observe_reference import FLUX_TOL
from stardis_amd import _lib, ops, synth
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from stardis_amd.postprocess import DeviceSpectrum
from test_gpu_response import profiled, small_model, synthesizer, thicken

pytestmark = pytest.mark.gpu

LAM = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))  # S-c2: 7634 points, log-uniform
IRREGULAR = np.sort(np.random.default_rng(7).uniform(6500.0, 6600.0, 3000))
TWO_DENSITY = np.r_[np.linspace(6500.0, 6550.0, 500, endpoint=False), np.linspace(6550.0, 6600.0, 4000)]
GRIDS = {"S-c2": LAM, "irregular": IRREGULAR, "two-density": TWO_DENSITY}
SC2_EDGES = np.linspace(6502.0, 6598.0, 2049)
QUOTIENT_STEPS = (0.008, 0.004)  # of test_dout_against_the_device_s_own_difference_quotients
PAIRS = [("S-c2", 0.3), ("S-c2", 1.5), ("S-c2", 1.6), ("S-c2", 1.62), ("S-c2", 3.2), ("S-c2", 35.0), ("irregular", 4.0), ("irregular", 17.0),
         ("two-density", 4.0), ("two-density", 17.0)]


def vectors(lam, seed=11):
    """-> flux, reference, u (signed), u_reference (signed)"""
    rng = np.random.default_rng(seed)
    return 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0), rng.standard_normal(lam.size), rng.standard_normal(lam.size)


_ROWS = {}


def rows_of(grid, zeta):
    """the restatement's windows and weights of one (grid, zeta), computed once per pair in use (the last one is kept)"""
    if (grid, zeta) not in _ROWS:
        _ROWS.clear()
        _ROWS[grid, zeta] = list(mref.point_rows(GRIDS[grid], zeta))
    return _ROWS[grid, zeta]


def dev_macro(ctx, lam, flux, zeta, reference=None, derivative=False):
    """sdx_macroturbulence_dev on uploaded arrays, zeta through device memory -> (out, out_reference, dout, dout_reference) as host
    arrays, None where not asked for"""
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_f, d_g, d_mac = up(lam), up(flux), up(reference), up(np.array([zeta]))
    new = lambda on: ctx.empty((lam.size,)) if on else None  # noqa: E731
    outs = [new(True), new(reference is not None), new(derivative), new(derivative and reference is not None)]
    ctx.call("sdx_macroturbulence_dev", lam.size, d_lam.ptr, d_f.ptr, _lib.ptr_of(d_g), d_mac.ptr, *(_lib.ptr_of(a) for a in outs))
    ctx.synchronize()
    return tuple(None if a is None else np.array(a.numpy()) for a in outs)


def dev_adjoint(ctx, lam, u, zeta, u_reference=None, nus=None):
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    d_lam, d_u, d_ur, d_nus, d_mac = up(lam), up(u), up(u_reference), up(nus), up(np.array([zeta]))
    w, w_ref = ctx.empty((lam.size,)), None if u_reference is None else ctx.empty((lam.size,))
    ctx.call("sdx_macroturbulence_adjoint_dev", lam.size, d_lam.ptr, d_mac.ptr, d_u.ptr, _lib.ptr_of(d_ur), _lib.ptr_of(d_nus), w.ptr, _lib.ptr_of(w_ref))
    ctx.synchronize()
    return np.array(w.numpy()), None if w_ref is None else np.array(w_ref.numpy())


def held(tag, got, ref, scale, tol=MACRO_TOL, nonzero=True):
    err, allow = np.abs(got.astype(LD) - ref).astype(np.float64), tol * scale.astype(np.float64)
    print(f"{tag}: {ref.size} points, worst |device - restatement| / allowance {float(np.max(err / allow)):.3e}, largest |value| / allowance "
          f"{float(np.max(np.abs(ref).astype(np.float64) / allow)):.3e}")
    assert np.all(np.isfinite(got)) and np.all(allow > 0)
    assert np.all(err <= allow)
    assert not nonzero or np.any(np.abs(ref).astype(np.float64) > 10 * allow)


def check_forward(ctx, tag, lam, zeta, rows=None):
    f, g, _, _ = vectors(lam)
    out, out_ref, dout, dout_ref = dev_macro(ctx, lam, f, zeta, reference=g, derivative=True)
    alone = dev_macro(ctx, lam, f, zeta)
    r = mref.macroturbulence(lam, f, zeta, reference=g, rows=rows)
    single = int(mref.window_lengths(lam, zeta).max()) == 1  # every window the point alone: the derivative is an exact 0
    held(f"{tag}, zeta = {zeta}: out", out, r["out"], r["scale"])
    held(f"{tag}, zeta = {zeta}: out_reference", out_ref, r["out_reference"], r["scale_reference"])
    held(f"{tag}, zeta = {zeta}: dout", dout, r["dout"], r["dscale"], nonzero=not single)
    held(f"{tag}, zeta = {zeta}: dout_reference", dout_ref, r["dout_reference"], r["dscale_reference"], nonzero=not single)
    # the flux depends neither on a reference going along nor on the derivative being asked for
    assert np.array_equal(alone[0], out) and alone[1:] == (None, None, None)
    assert np.array_equal(dev_macro(ctx, lam, f, zeta, derivative=True)[2], dout)
    if single:
        assert not dout.any() and not dout_ref.any()


# ---- 1: forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeta", [0.05, 0.3, 1.5, 1.6, 1.62, 3.2, 35.0])
def test_forward_on_the_sc2_grid(ctx, zeta):
    """interior windows of 1, 7, 31 (eight lanes everywhere), 33 (the estimate straddles the switch within the grid at 1.6 and lies just
    past it at 1.62), 65 (one trip past a wave) and 701 points (11 trips per lane)"""
    n = mref.window_lengths(LAM, zeta)
    expected = mref.mapping_estimate(LAM, zeta)
    print(f"zeta = {zeta}: windows of {n.min()} .. {n.max()} points, the mapping's estimate {expected.min():.2f} .. {expected.max():.2f}")
    assert n.max() == {0.05: 1, 0.3: 7, 1.5: 31, 1.6: 33, 1.62: 33, 3.2: 65, 35.0: 701}[zeta]
    if zeta == 1.5:
        assert expected.max() <= 30.3  # eight lanes per point everywhere
    if zeta == 1.6:
        assert expected.min() <= 32 < expected.max()  # both mappings in one launch
    if zeta == 1.62:
        assert 32 < expected.min() < 33  # a wave per point, just past the switch
    check_forward(ctx, "S-c2", LAM, zeta, rows=rows_of("S-c2", zeta))
    if zeta == 0.05:  # every window is the point alone: (K h F) / (K h), two roundings
        f = vectors(LAM)[0]
        assert np.max(np.abs(dev_macro(ctx, LAM, f, zeta)[0] / f - 1)) <= 3e-16


@pytest.mark.parametrize("grid", ["irregular", "two-density"])
@pytest.mark.parametrize("zeta", [4.0, 17.0])
def test_forward_on_other_grids(ctx, grid, zeta):
    """the mean-spacing estimate is wrong locally; either mapping must serve any point"""
    lam = GRIDS[grid]
    n = mref.window_lengths(lam, zeta)
    expected = mref.mapping_estimate(lam, zeta)
    print(f"{grid}, zeta = {zeta}: windows of {n.min()} .. {n.max()} points against an estimate of {expected.min():.1f} .. {expected.max():.1f}")
    check_forward(ctx, grid, lam, zeta, rows=rows_of(grid, zeta))


def test_forward_on_small_grids(ctx):
    """n = 2, 3, 9 with every window truncated at an end (or both), and n that is no multiple of the group of 8"""
    cases = [(f"n = {n}, every window truncated", 6560.0 + 0.013 * np.arange(n) ** 1.1, 7.0) for n in (2, 3, 9)]
    cases += [(f"n = {n}", 6560.0 * np.exp(np.arange(n) / 4.1e5), zeta) for n, zeta in ((13, 0.5), (77, 1.5), (1001, 5.0))]
    for tag, lam, zeta in cases:
        n = mref.window_lengths(lam, zeta)
        if "truncated" in tag:
            b = 6.0 * zeta / K.C_KMS
            assert np.all((lam * (1 - b) < lam[0]) | (lam * (1 + b) > lam[-1])) and n.max() == lam.size
        check_forward(ctx, tag, lam, zeta)


@pytest.mark.parametrize("zeta", [1.6, 3.2])
def test_dout_against_the_device_s_own_difference_quotients(ctx, zeta):
    """dout against central differences of the device's forward at zeta (1 +- h), h = 0.008 and 0.004, and their Richardson value; the
    allowance is what the two quotients differ by plus MACRO_TOL max |F| / h (the forward's own allowance over the coarse step).  The
    quotients' difference is an O(h^2) quantity that changes sign along the grid, and where it cancels only the second term is left
    for the O(h^4) remainder of the Richardson value: the steps are those at which the RESTATEMENT's remainder stays below that term
    at every point (tests/test_macroturbulence_cpu.py: 1.5e-10 against 1.7e-10; at h = 0.02 and 0.01 the restatement itself misses by
    1.6).  A point that enters or leaves a window between the two zeta carries 3e-18 of the peak: fixed windows cost nothing here."""
    f = vectors(LAM)[0]
    dout = dev_macro(ctx, LAM, f, zeta, derivative=True)[2]
    q = {h: (dev_macro(ctx, LAM, f, zeta * (1 + h))[0].astype(LD) - dev_macro(ctx, LAM, f, zeta * (1 - h))[0]) / (2 * h) for h in QUOTIENT_STEPS}
    coarse, fine = (q[h] for h in QUOTIENT_STEPS)
    rich = (4 * fine - coarse) / 3
    allow = (np.abs(coarse - fine) + MACRO_TOL * np.abs(f).max() / QUOTIENT_STEPS[0]).astype(np.float64)
    err = np.abs(dout - rich).astype(np.float64)
    print(f"zeta = {zeta}: worst |dout - Richardson| / allowance {np.max(err / allow):.3e}, largest |dout| / allowance {np.max(np.abs(dout) / allow):.3e}")
    assert np.all(err <= allow) and np.any(np.abs(dout) > 10 * allow)


# ---- 2: no macroturbulence -----------------------------------------------------------------------------------------------------------
def test_zero_zeta_is_a_copy_and_no_macroturbulence_launches_nothing(ctx):
    f, g, u, _ = vectors(LAM)
    for zeta in (0.0, -5.0, np.nan):
        out, out_ref, dout, dout_ref = dev_macro(ctx, LAM, f, zeta, reference=g, derivative=True)
        assert np.array_equal(out, f) and np.array_equal(out_ref, g) and not dout.any() and not dout_ref.any(), zeta
        assert np.array_equal(dev_adjoint(ctx, LAM, u, zeta)[0], u), zeta
    plain, still = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx), Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_mac=0.0)
    assert not plain.macroturbulent and not plain.broadens and still.macroturbulent and not hasattr(plain, "d_mac") and plain._scratch is None
    d_lam, d_f, d_g, d_c = (ctx.upload(a) for a in (LAM, f, g, np.random.default_rng(1).standard_normal(2048)))
    stages = ("k_macroturbulence", "k_macroturbulence_adjoint", "k_rotate", "k_rotate_adjoint", "k_observe", "k_observe_adjoint")
    with profiled(ctx):
        a = np.array(plain.observe(d_lam, d_f, LAM.size, d_g).numpy())
        wa = np.array(plain.adjoint(d_lam, LAM.size, d_c).numpy())
        ctx.synchronize()
        counts = {k: ctx.profile(k)[0] for k in stages}
        print(f"an instrument without v_mac: {counts}")
        assert counts == dict.fromkeys(stages[:4], 0) | {"k_observe": 1, "k_observe_adjoint": 1}
        b = np.array(still.observe(d_lam, d_f, LAM.size, d_g).numpy())
        wb = np.array(still.adjoint(d_lam, LAM.size, d_c).numpy())
        ctx.synchronize()
        assert ctx.profile("k_macroturbulence")[0] == 1 and ctx.profile("k_macroturbulence_adjoint")[0] == 1 and ctx.profile("k_rotate")[0] == 0
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(wa, wb) and not np.isnan(a).all() and wa.any()
    assert np.array_equal(ops.observe(LAM, f, SC2_EDGES, plain.sigma, ctx=ctx), ops.observe(LAM, f, SC2_EDGES, plain.sigma, ctx=ctx, v_mac=0.0), equal_nan=True)
    assert np.array_equal(still.observe_host(LAM, f, g), a, equal_nan=True)
    with pytest.raises(RuntimeError, match="no macroturbulence"):
        plain.set_macroturbulence(5.0)
    with pytest.raises(RuntimeError, match="no macroturbulence"):
        plain.macroturbulence(d_lam, d_f, LAM.size)


# ---- 3: the adjoint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,zeta", PAIRS)
def test_adjoint(ctx, grid, zeta):
    lam = GRIDS[grid]
    f, g, u, u_ref = vectors(lam)
    nus = K.C_CGS * 1.0e8 / lam
    rows = rows_of(grid, zeta)
    out, out_ref, _, _ = dev_macro(ctx, lam, f, zeta, reference=g)
    terms, terms_ref = mref.dot_terms(lam, u, f, zeta, rows=rows), mref.dot_terms(lam, u_ref, g, zeta, rows=rows)
    r_w, r_wr, scale, scale_ref = mref.adjoint(lam, u, zeta, u_reference=u_ref, rows=rows)
    k = (nus / lam).astype(LD)
    for nus_on in (False, True):
        mode = f"{grid}, zeta = {zeta}{', nus' if nus_on else ''}"
        w, w_ref = dev_adjoint(ctx, lam, u, zeta, u_reference=u_ref, nus=nus if nus_on else None)
        alone, _ = dev_adjoint(ctx, lam, u, zeta, nus=nus if nus_on else None)
        assert np.array_equal(alone, w)
        held(mode + ": w", w, r_w * k if nus_on else r_w, scale * k if nus_on else scale)
        held(mode + ": w_reference", w_ref, r_wr * k if nus_on else r_wr, scale_ref * k if nus_on else scale_ref)
        back = (lam / nus if nus_on else np.ones(lam.size)).astype(LD)
        for tag, o, uu, ww, ff, tt in (("flux", out, u, w, f, terms), ("reference", out_ref, u_ref, w_ref, g, terms_ref)):
            lhs, rhs = float(np.sum(o.astype(LD) * uu)), float(np.sum(ww.astype(LD) * ff * back))
            print(f"{mode}, {tag}: <M f, u> = {lhs:.15e}, <f, M^T u> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (SUM_TOL * tt):.3e}")
            assert abs(lhs - rhs) <= SUM_TOL * tt and abs(lhs) > 10 * SUM_TOL * tt
    # every point lies in a window, its own: weights of one sign give a weight at every point
    positive, _ = dev_adjoint(ctx, lam, np.abs(u) + 0.1, zeta)
    assert np.all(positive > 0)


# ---- 4: determinism, graphs, the host-buffer twins, the refusals -----------------------------------------------------------------------
def capture(ctx, run):
    ctx.call("sdx_graph_begin")
    try:
        run()
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    return graph


def test_bits_repeat_and_graphs_follow_every_setter(ctx):
    inst = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_rot=19.3, v_mac=3.2)
    f, g, _, _ = vectors(LAM)
    c = np.random.default_rng(5).standard_normal(2048)
    nus = K.C_CGS * 1.0e8 / LAM
    d_lam, d_c, d_f, d_g, d_nus = (ctx.upload(a) for a in (LAM, c, f, g, nus))
    pix, w, w_ref = ctx.empty((2048,)), ctx.empty((LAM.size,)), ctx.empty((LAM.size,))

    def run():
        inst.observe(d_lam, d_f, LAM.size, reference=d_g, out=pix)
        inst.adjoint(d_lam, LAM.size, d_c, flux=d_f, reference=d_g, nus=d_nus, out=w, out_reference=w_ref)

    def result():
        return tuple(np.array(a.numpy()) for a in (pix, w, w_ref))

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    def at(zeta, v_rot, eps, v_rad):
        inst.set_macroturbulence(zeta)
        inst.set_rotation(v_rot, eps)
        inst.set_radial_velocity(v_rad)

    run()
    eager0 = result()
    run()
    assert same(eager0, result()) and all(np.nan_to_num(a).any() for a in eager0)
    at(7.5, 55.0, 0.3, 30.0)
    run()
    eager1 = result()
    assert not np.array_equal(eager1[0], eager0[0], equal_nan=True) and not np.array_equal(eager1[1], eager0[1])
    at(7.5, 19.3, 0.6, 0.0)  # only zeta moved against eager0
    run()
    eager2 = result()
    assert not np.array_equal(eager2[0], eager0[0], equal_nan=True) and not np.array_equal(eager2[1], eager0[1])
    at(3.2, 19.3, 0.6, 0.0)
    graph = capture(ctx, run)  # (the scratch was sized by the eager runs: the capture allocates nothing)
    try:
        for a in (pix, w, w_ref):
            a.zero()
        ctx.call("sdx_graph_launch", graph)
        replay0 = result()
        inst.set_macroturbulence(7.5)  # no new capture: the kernels read zeta, the pair and the factor from device memory
        ctx.call("sdx_graph_launch", graph)
        replay2 = result()
        at(7.5, 55.0, 0.3, 30.0)
        ctx.call("sdx_graph_launch", graph)
        replay1 = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    print(f"replay against eager: {[int(np.sum(a != b)) for a, b in zip(replay0, eager0)]} values differ, after set_macroturbulence "
          f"{[int(np.sum(a != b)) for a, b in zip(replay2, eager2)]}, after all three setters {[int(np.sum(a != b)) for a, b in zip(replay1, eager1)]} (NaN pixels count)")
    assert same(replay0, eager0) and same(replay2, eager2) and same(replay1, eager1)
    # the host-buffer twins, stage by stage and through the instrument
    twin = inst.macroturbulence_host(LAM, f, g, derivative=True)
    stage = dev_macro(ctx, LAM, f, 7.5, reference=g, derivative=True)
    assert len(twin) == 4 and all(np.array_equal(a, b) for a, b in zip(twin, stage))
    assert np.array_equal(ops.macroturbulence(LAM, f, 7.5, ctx=ctx), stage[0])
    pair = ops.macroturbulence(LAM, f, 7.5, derivative=True, ctx=ctx)
    assert np.array_equal(pair[0], stage[0]) and np.array_equal(pair[1], stage[2])
    u = np.random.default_rng(6).standard_normal(LAM.size)
    tw = np.empty(LAM.size)
    ctx.call("sdx_macroturbulence_adjoint_f64", LAM.size, LAM.ctypes.data, 7.5, u.ctypes.data, None, nus.ctypes.data, tw.ctypes.data, None)
    assert np.array_equal(tw, dev_adjoint(ctx, LAM, u, 7.5, nus=nus)[0])
    assert np.array_equal(inst.observe_host(LAM, f, g), eager1[0], equal_nan=True)
    host = inst.adjoint_host(LAM, c, flux=f, reference=g, nus=nus)
    assert np.array_equal(host[0], eager1[1]) and np.array_equal(host[1], eager1[2])
    kw = dict(ctx=ctx, v_rot=55.0, limb_darkening=0.3, v_mac=7.5)
    assert np.array_equal(ops.observe(LAM, f, SC2_EDGES, inst.sigma, v_rad=30.0, reference=g, **kw), eager1[0], equal_nan=True)
    assert np.array_equal(ops.observe_adjoint(LAM, c, SC2_EDGES, inst.sigma, v_rad=30.0, flux=f, reference=g, nus=nus, **kw)[0], eager1[1])
    # macroturbulence alone: the device path, the host path and ops agree bit for bit
    only = Instrument(SC2_EDGES, resolving_power=5.0e4, ctx=ctx, v_mac=7.5)
    dev = np.array(only.observe(d_lam, d_f, LAM.size).numpy())
    wd = np.array(only.adjoint(d_lam, LAM.size, d_c, nus=d_nus).numpy())
    assert np.array_equal(only.observe_host(LAM, f), dev, equal_nan=True) and np.array_equal(only.adjoint_host(LAM, c, nus=nus), wd)
    assert np.array_equal(ops.observe(LAM, f, SC2_EDGES, only.sigma, ctx=ctx, v_mac=7.5), dev, equal_nan=True) and not np.array_equal(dev, eager1[0], equal_nan=True)


def test_refusals_leave_the_context_serving(ctx):
    lib = ctx.lib
    lam = LAM[:500]
    f, g, u, _ = vectors(lam)
    n = lam.size
    expect = dev_macro(ctx, lam, f, 1.5)[0]
    expect_w, _ = dev_adjoint(ctx, lam, u, 1.5)
    d = ctx.upload(lam)
    o, o2, o3 = ctx.empty((n,)), ctx.empty((n,)), ctx.empty((n,))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with profiled(ctx):
        # (ctx, n, lambdas, flux, reference, mac_dev, out, out_reference, dout, dout_reference)
        for args in ((1, d.ptr, d.ptr, None, d.ptr, o.ptr, None, None, None), (n, None, d.ptr, None, d.ptr, o.ptr, None, None, None),
                     (n, d.ptr, None, None, d.ptr, o.ptr, None, None, None), (n, d.ptr, d.ptr, None, None, o.ptr, None, None, None),
                     (n, d.ptr, d.ptr, None, d.ptr, None, None, None, None),  # no out
                     (n, d.ptr, d.ptr, None, d.ptr, None, None, o.ptr, None),  # dout without out
                     (n, d.ptr, d.ptr, None, d.ptr, o.ptr, None, o2.ptr, o3.ptr),  # dout_reference without reference
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, o.ptr, None, None, None),  # reference without out_reference
                     (n, d.ptr, d.ptr, None, d.ptr, o.ptr, o2.ptr, None, None),  # out_reference without reference
                     (n, d.ptr, d.ptr, None, d.ptr, d.ptr, None, None, None),  # out is an input
                     (n, d.ptr, d.ptr, None, d.ptr, o.ptr, None, d.ptr, None),  # dout is an input
                     (n, d.ptr, d.ptr, None, d.ptr, o.ptr, None, o.ptr, None),  # dout is out
                     (n, d.ptr, d.ptr, d.ptr, d.ptr, o.ptr, o2.ptr, o3.ptr, o2.ptr)):  # dout_reference is out_reference
            assert lib.sdx_macroturbulence_dev(ctx.handle, *args) == -1 and b"macroturbulence" in lib.sdx_last_error_string(), args
        # (ctx, n, lambdas, mac_dev, u, u_reference, nus, w, w_reference)
        for args in ((1, d.ptr, d.ptr, d.ptr, None, None, o.ptr, None), (n, None, d.ptr, d.ptr, None, None, o.ptr, None), (n, d.ptr, None, d.ptr, None, None, o.ptr, None),
                     (n, d.ptr, d.ptr, None, None, None, o.ptr, None), (n, d.ptr, d.ptr, d.ptr, None, None, None, None), (n, d.ptr, d.ptr, d.ptr, d.ptr, None, o.ptr, None),
                     (n, d.ptr, d.ptr, d.ptr, None, None, o.ptr, o.ptr), (n, d.ptr, d.ptr, o.ptr, None, None, o.ptr, None), (n, d.ptr, d.ptr, o2.ptr, None, o.ptr, o.ptr, None)):
            assert lib.sdx_macroturbulence_adjoint_dev(ctx.handle, *args) == -1 and b"macroturbulence_adjoint" in lib.sdx_last_error_string(), args
        # the twins check what the kernels cannot, before any copy
        out = np.full(n, -7.0)
        for tag, kw in dict(lambdas=dict(lam=np.ascontiguousarray(lam[::-1])), nan_lambda=dict(lam=np.r_[lam[:-1], np.nan]), negative=dict(zeta=-1.0), wide=dict(zeta=500.0),
                            nan_zeta=dict(zeta=np.nan)).items():
            a = dict(dict(lam=lam, zeta=1.5), **kw)
            rc = lib.sdx_macroturbulence_f64(ctx.handle, n, p(a["lam"]), p(f), None, a["zeta"], p(out), None, None, None)
            msg = lib.sdx_last_error_string().decode()
            print(f"{tag}: rc {rc}, '{msg}'")
            assert rc == -1 and np.all(out == -7.0) and ("lambdas" if "lam" in kw else "zeta") in msg
            assert lib.sdx_macroturbulence_adjoint_f64(ctx.handle, n, p(a["lam"]), a["zeta"], p(u), None, None, p(out), None) == -1 and np.all(out == -7.0)
            assert ("lambdas" if "lam" in kw else "zeta") in lib.sdx_last_error_string().decode()
        ctx.synchronize()
        assert ctx.profile("k_macroturbulence")[0] == 0 and ctx.profile("k_macroturbulence_adjoint")[0] == 0
        assert np.array_equal(dev_macro(ctx, lam, f, 1.5)[0], expect) and np.array_equal(dev_adjoint(ctx, lam, u, 1.5)[0], expect_w)
        assert ctx.profile("k_macroturbulence")[0] == 1 and ctx.profile("k_macroturbulence_adjoint")[0] == 1
    assert lib.sdx_macroturbulence_f64(ctx.handle, n, p(lam), p(f), None, 1.5, p(out), None, None, None) == 0 and np.array_equal(out, expect)


# ---- 5: the instrument ---------------------------------------------------------------------------------------------------------------
def broadened(lam, f, V, eps, zeta, reference=None):
    """restatement after restatement, each rounded to fp64 as the device's buffers are -> (flux, reference or None)"""
    rf, rg, _, _ = rref.rotate(lam, f, V, eps, reference=reference) if V is not None else (np.asarray(f), reference, None, None)
    rf, rg = np.asarray(rf, dtype=np.float64), None if rg is None else np.asarray(rg, dtype=np.float64)
    r = mref.macroturbulence(lam, rf, zeta, reference=rg)
    return r["out"].astype(np.float64), None if rg is None else r["out_reference"].astype(np.float64)


def test_instrument_with_both_broadenings(ctx):
    lam = LAM[(LAM > 6530.0) & (LAM < 6570.0)]
    edges = np.linspace(6531.0, 6569.0, 401)
    f, g, _, _ = vectors(lam)
    c = np.random.default_rng(6).standard_normal(400)
    nus = K.C_CGS * 1.0e8 / lam
    V, eps, zeta, v_rad = 40.0, 0.6, 4.0, 25.0
    assert rref.clear_of_profile_edge(lam, V, 1e-8)
    inst = Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=V, limb_darkening=eps, v_mac=zeta)
    rot_only = Instrument(edges, resolving_power=5.0e4, ctx=ctx, v_rot=V, limb_darkening=eps)
    for i in (inst, rot_only):
        i.set_radial_velocity(v_rad)
    assert oref.clear_of_grid_ends(lam, edges, inst.sigma, inst.doppler)
    bf, bg = broadened(lam, f, V, eps, zeta, reference=g)
    b_abs = broadened(lam, np.abs(f), V, eps, zeta)[0]
    edge, edge_rot = inst.edge_affected(lam), rot_only.edge_affected(lam)
    print(f"edge-affected pixels: {int(edge.sum())}, of them {int((edge & ~edge_rot).sum())} because of the macroturbulence's reach alone")
    assert np.all(edge[edge_rot]) and (edge & ~edge_rot).sum() >= 1
    for ref_on in (False, True):
        got = inst.observe_host(lam, f, g if ref_on else None)
        expect = oref.observe(lam, bf, edges, inst.sigma, inst.doppler, reference=bg if ref_on else None)
        ok = ~np.isnan(expect)
        err = np.abs(got[ok] - expect[ok]) / np.abs(expect[ok])
        print(f"observe_host{', reference' if ref_on else ''}: {ok.sum()} pixels, {int((ok & ~edge).sum())} clear of the grid's ends, worst relative difference {err.max():.3e}")
        assert np.array_equal(np.isnan(got), ~ok) and (ok & ~edge).sum() > 300 and edge.sum() > (~ok).sum()
        assert np.all(err[~edge[ok]] <= FLUX_TOL)
        # the transpose through the three stages: <observe(M(rotate(f))), c> = <f, adjoint(c)>
        w = inst.adjoint_host(lam, c, flux=f if ref_on else None, reference=g if ref_on else None, nus=nus)
        w = w[0] if ref_on else w
        terms = aref.dot_terms(lam, c, b_abs, edges, inst.sigma, inst.doppler, reference=bg if ref_on else None)
        lhs, rhs = float(np.sum(c[ok] * got[ok])), float(np.sum(w.astype(LD) * f * lam / nus))
        print(f"adjoint_host{', normalised' if ref_on else ''}: <observe(f), c> = {lhs:.15e}, <f, adjoint(c)> = {rhs:.15e}, difference / allowance "
              f"{abs(lhs - rhs) / (3 * SUM_TOL * terms):.3e}")
        assert abs(lhs - rhs) <= 3 * SUM_TOL * terms and abs(lhs) > 30 * SUM_TOL * terms  # (three stages of reordered sums)


# ---- 6: the engine -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(ctx):
    """the small model of tests/test_gpu_response.py: 12 depths, 300 points, 40 lines"""
    return thicken(ctx, small_model())


V_ROT, V_MAC = 10.0, 3.0


def engine_instrument(ctx, v=12.0, v_rot=V_ROT, v_mac=V_MAC):
    """one pixel that the 6560 - 6570 A grid covers but whose window comes within the rotation's reach of the grid's blue end, one that
    comes within the combined reach only, 24 pixels clear of both ends, one off the red end"""
    inst = Instrument(np.r_[6560.75, 6561.2, np.linspace(6562.0, 6568.0, 25), 6571.0], sigma=0.05, ctx=ctx, v_rot=v_rot, v_mac=v_mac)
    inst.set_radial_velocity(v)
    return inst


STAGES = ("k_macroturbulence", "k_macroturbulence_adjoint", "k_rotate", "k_rotate_adjoint", "k_observe", "k_observe_adjoint", "k_flux_nu_to_lambda",
          "k_line_adjoint", "k_response_weight", "k_raytrace")


def counts(ctx):
    ctx.synchronize()
    return {k: ctx.profile(k)[0] for k in STAGES}


def chain(lam, inst, f_lam, g_lam, zeta):
    """observed and observed_normalized by the restatements at macroturbulence zeta"""
    bf, bg = broadened(lam, f_lam, V_ROT, 0.6, zeta, reference=g_lam)
    return oref.observe(lam, bf, inst.edges, inst.sigma, inst.doppler), oref.observe(lam, bf, inst.edges, inst.sigma, inst.doppler, reference=bg), bf, bg


def test_engine_chain_with_macroturbulence(ctx, model):
    m = model
    n_depth, n_nu, n_lines, n_pix = 12, 300, 40, 27
    lam = K.nu_to_angstrom(m.nus)
    inst, rot_only = engine_instrument(ctx), engine_instrument(ctx, v_mac=None)
    edge = inst.edge_affected(lam)
    assert edge.tolist() == [True, True] + [False] * 24 + [True] and rot_only.edge_affected(lam).tolist() == [True, False] + [False] * 24 + [True]
    syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=inst)
    ref_syn = synthesizer(ctx, m, keep_response=True, keep_continuum_flux=True, instrument=rot_only)
    with profiled(ctx):
        ref_syn.step()
        before = counts(ctx)
    with profiled(ctx):
        syn.step()
        after = counts(ctx)
        print(f"launches of a step without macroturbulence {before}\n                   with macroturbulence {after}")
        assert after == dict(before, k_macroturbulence=1) and before["k_macroturbulence"] == 0 and after["k_observe"] == 2
        assert after["k_macroturbulence_adjoint"] == 0 and after["k_rotate_adjoint"] == 0 and after["k_observe_adjoint"] == 0
        c = np.random.default_rng(5).standard_normal(n_pix)
        c[-1] = np.nan  # the pixel off the grid's end: never read
        sens = syn.observed_line_sensitivities(c)
        on_demand = counts(ctx)
        assert on_demand["k_macroturbulence_adjoint"] == 1 and on_demand["k_rotate_adjoint"] == 1 and on_demand["k_observe_adjoint"] == 1
        assert on_demand["k_line_adjoint"] == 1 and on_demand["k_macroturbulence"] == 1 and on_demand["k_rotate"] == 1
    sens = np.array(sens.numpy())

    # observed and observed_normalized against the restatements
    F, Fc = np.array(syn.F_nu()[-1]), np.array(syn.F_nu_continuum[-1])
    f_lam, g_lam = F * m.nus / lam, Fc * m.nus / lam
    expect_obs, expect_norm, bf, bg = chain(lam, inst, f_lam, g_lam, V_MAC)
    observed, normalized = np.array(syn.observed.numpy()), np.array(syn.observed_normalized.numpy())
    for tag, got, expect in (("observed", observed, expect_obs), ("observed_normalized", normalized, expect_norm)):
        ok = ~np.isnan(expect)
        err = np.abs(got[ok] - expect[ok]) / np.abs(expect[ok])
        print(f"engine, {tag}: worst relative difference {err.max():.3e}")
        assert ok.tolist() == [True] * 26 + [False] and np.array_equal(np.isnan(got), ~ok) and np.all(err <= FLUX_TOL)
    assert not np.array_equal(observed, np.array(ref_syn.observed.numpy()), equal_nan=True)  # the stage really ran
    spec = DeviceSpectrum(syn)
    assert np.array_equal(spec.observed(inst).numpy(), observed, equal_nan=True)
    assert np.array_equal(spec.observed(inst, normalized=True).numpy(), normalized, equal_nan=True)

    # per line against the forward chain c . inst.observe(flux_derivative(single-line plane) nu / lambda), both broadenings inside observe:
    # the bound of test_gpu_rotation.test_engine_chain_with_rotation and one more SUM_TOL for the macroturbulence's reordered sums
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
        allowed = (2 * A.OPACITY_RTOL + n_depth * n_nu * A.EPS + 3 * SUM_TOL) * float(np.abs(w_abs[None, :] * Ra * (plane / total)).sum())
        assert abs(sens[l] - expect) <= allowed, (l, sens[l], expect, allowed)
        worst = max(worst, abs(sens[l] - expect) / allowed) if allowed > 0 else worst
        seen |= abs(sens[l]) > 10 * allowed
    print(f"observed_line_sensitivities against the forward chain per line: worst difference / bound {worst:.3e}")
    assert seen

    # chi-square: the NaN pixel, the pixel without weight AND the wider edge set are left out
    rng = np.random.default_rng(8)
    chi2_inputs = {}
    for norm_on in (False, True):
        obs = normalized if norm_on else observed
        data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(n_pix))
        ivar = rng.uniform(0.5, 2.0, n_pix) / np.nanmax(np.abs(obs)) ** 2
        ivar[5] = 0.0
        use = ~np.isnan(obs) & (ivar != 0) & ~edge
        assert use.sum() == 23 and not np.isnan(obs[1]) and ivar[1] != 0 and not use[1]
        chi2, grad = syn.chi2_line_gradient(data, ivar, normalized=norm_on)
        r, w = np.where(use, data, 0.0) - np.where(use, obs, 0.0), np.where(use, ivar, 0.0)
        expect = float(np.sum(w * r * r))
        print(f"normalized = {norm_on}: chi2 {chi2!r} against numpy {expect!r}")
        assert chi2 == expect and chi2 > 0
        assert np.array_equal(grad.numpy(), syn.observed_line_sensitivities(-2.0 * w * r, normalized=norm_on).numpy()) and np.array(grad.numpy()).any()
        chi2_inputs[norm_on] = (data, ivar, use, chi2)

    # d / d zeta on demand: the launches, then both functions against difference quotients of whole set_macroturbulence + step() runs
    cz = np.where(edge, 0.0, c0)
    assert (cz != 0).sum() >= 20  # pixels clear of every edge
    with profiled(ctx):
        value = {norm_on: syn.observed_macroturbulence_derivative(cz, normalized=norm_on) for norm_on in (False, True)}
        extra = counts(ctx)
        print(f"launches of two observed_macroturbulence_derivative calls {extra}")
        assert extra["k_macroturbulence"] == 2 and extra["k_observe_adjoint"] == 2 and extra["k_macroturbulence_adjoint"] == 0 and extra["k_observe"] == 0
    gradient = {norm_on: syn.chi2_macroturbulence_gradient(*chi2_inputs[norm_on][:2], normalized=norm_on) for norm_on in (False, True)}
    runs = {}
    for h in (0.02, -0.02, 0.01, -0.01):
        inst.set_macroturbulence(V_MAC * (1 + h))
        syn.step()
        runs[h] = (np.array(syn.observed.numpy()), np.array(syn.observed_normalized.numpy()))
    inst.set_macroturbulence(V_MAC)
    syn.step()
    assert np.array_equal(syn.observed.numpy(), observed, equal_nan=True)
    for norm_on in (False, True):
        obs = normalized if norm_on else observed
        data, ivar, use, chi2 = chi2_inputs[norm_on]
        w = np.where(use, ivar, 0.0)
        c_chi = -2.0 * w * (np.where(use, data, 0.0) - np.where(use, obs, 0.0))
        functionals = {"sum c observed": (lambda o: float(np.sum(np.where(cz != 0, cz * o, 0.0))), value[norm_on], cz),  # noqa: E731
                       "chi2": (lambda o: float(np.sum(w * (np.where(use, data, 0.0) - np.where(use, o, 0.0)) ** 2)), gradient[norm_on][1], c_chi)}  # noqa: E731
        assert gradient[norm_on][0] == chi2
        for tag, (fn, got, weights) in functionals.items():
            coarse = (fn(runs[0.02][norm_on]) - fn(runs[-0.02][norm_on])) / (2 * 0.02 * V_MAC)
            fine = (fn(runs[0.01][norm_on]) - fn(runs[-0.01][norm_on])) / (2 * 0.01 * V_MAC)
            rich = (4 * fine - coarse) / 3
            allowance = abs(coarse - fine) + FLUX_TOL * np.nanmax(np.abs(obs)) * float(np.sum(np.abs(weights))) / (0.02 * V_MAC)
            print(f"normalized = {norm_on}, d({tag}) / d zeta: {got:+.9e} against the Richardson value {rich:+.9e} of {coarse:+.9e} and {fine:+.9e}, "
                  f"difference / allowance {abs(got - rich) / allowance:.3e}, |value| / allowance {abs(got) / allowance:.3e}")
            assert abs(got - rich) <= allowance and abs(got) > 10 * allowance
    inst.set_macroturbulence(0.0)
    with pytest.raises(ValueError, match="zeta"):
        syn.chi2_macroturbulence_gradient(*chi2_inputs[False][:2])
    with pytest.raises(RuntimeError, match="no macroturbulence"):
        ref_syn.chi2_macroturbulence_gradient(*chi2_inputs[False][:2])
    inst.set_macroturbulence(V_MAC)

    # the normalised weights through the three stages: their dot identity on the device
    cn = rng.standard_normal(n_pix)
    wn = np.array(syn.pixel_weights_to_grid(cn, normalized=True).numpy())
    terms = aref.dot_terms(lam, cn, broadened(lam, np.abs(f_lam), V_ROT, 0.6, V_MAC)[0], inst.edges, inst.sigma, inst.doppler, reference=bg)
    lhs, rhs = float(np.sum(cn[:-1] * normalized[:-1])), float(wn @ F)
    print(f"normalised: <observed_normalized, c> = {lhs:.15e}, <F_nu, weights> = {rhs:.15e}, difference / allowance {abs(lhs - rhs) / (3 * SUM_TOL * terms):.3e}")
    assert abs(lhs - rhs) <= 3 * SUM_TOL * terms and abs(lhs) > 30 * SUM_TOL * terms
    # a captured step replays the stage and follows set_macroturbulence
    syn.capture()
    try:
        syn.d_observed.zero()
        syn.step()
        assert np.array_equal(syn.observed.numpy(), observed, equal_nan=True)
        inst.set_macroturbulence(6.0)
        syn.step()
        moved = np.array(syn.observed.numpy())
    finally:
        syn._destroy_graphs()
    expect = chain(lam, inst, f_lam, g_lam, 6.0)[0]
    assert not np.array_equal(moved, observed, equal_nan=True) and np.all(np.abs(moved[:-1] - expect[:-1]) <= FLUX_TOL * np.abs(expect[:-1]))
    syn.close()
    ref_syn.close()
