"""k_observe and the k_observe_adjoint_* kernels against the extended-precision evaluation of their definition on hostile inputs
(tests/observe_truth.py): per pixel and per grid point no further from the truth than
    FACTOR d_ref(case) + (U Lambda / A + T + 8) 2^-53
of the sum of the absolute terms, d_ref the fp64 restatement's own distance on the same case and U the error of the device's erf and
erfc recorded in profiles/observe_truth_classes.json — measured again here and asserted not to exceed it, so that a change of the
vendor's math library is reported as that.  The host-buffer twin gives the device path's bits on every case; scaling by a power of two
changes no bit of the mantissa; <observe(f), c> = <f, adjoint(c)> to the roundings of the two sums alone (some 20 x 2^-53 of the terms).  No pixel and no point of any
case is excused.  Every test prints its figures before it asserts; they go to observe_truth.RECORD
(scripts/observe_truth_table.py -> profiles/observe_truth_classes.json).  The truth is mpmath's: no long double is needed."""
import ctypes as C

import numpy as np
import pytest

import observe_adjoint_reference as aref
import observe_reference as oref
import observe_truth as OT
from stardis_amd import ops
from stardis_amd.instrument import Instrument

pytestmark = pytest.mark.gpu
M = OT.M
_FORWARD = {}


def instrument(ctx, name):
    _, _, _, edges, sigma, D = OT.hostile(name)
    inst = Instrument(edges, sigma=sigma, ctx=ctx)
    inst.d_doppler.set(np.array([D]))  # the case's Doppler factor itself, not a velocity's
    inst.doppler = D
    return inst


def forward(ctx, name):
    """the device path on the case, once per process"""
    if name not in _FORWARD:
        lam, f, g, _, _, _ = OT.hostile(name)
        _FORWARD[name] = np.array(instrument(ctx, name).observe_host(lam, f, g))
    return _FORWARD[name]


def host_twin(ctx, lam, f, g, edges, sigma, D):
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(sigma.size, -7.0)
    keep = [np.ascontiguousarray(a) for a in (lam, f, edges, sigma)] + ([np.ascontiguousarray(g)] if g is not None else [])
    rc = ctx.lib.sdx_observe_f64(ctx.handle, lam.size, p(keep[0]), p(keep[1]), None if g is None else p(keep[4]), sigma.size, p(keep[2]), p(keep[3]), D, p(out))
    assert rc == 0, ctx.lib.sdx_last_error_string()
    return out


# ---- U ---------------------------------------------------------------------------------------------------------------------------------
def test_the_device_s_erf_and_erfc_are_within_the_recorded_U(ctx):
    p, a_c, b_c, a_e, b_e = OT.ulp_arguments()
    r_c = ops.observe_response_grad(a_c, b_c, 0.0, 1.0, ctx=ctx)[0]
    r_e = ops.observe_response_grad(a_e, b_e, 0.0, 1.0, ctx=ctx)[0]
    worst, where = OT.ulp_figure(p, 2.0 * r_c, 2.0 * r_e)
    U = OT.device_U()
    print(f"erf / erfc on the device at {p.size} arguments 0 .. 8.5: worst {worst:.3f} x 2^-53 |value| at {where}; recorded U = {U}")
    OT.RECORD.append(dict(case="erf, erfc", quantity="units of 2^-53 |value|", label="device library", kernel=float(worst), restatement=None, allowance=float(U),
                          worst_ratio=float(worst / U)))
    assert 0 < worst <= U, "the device's erf / erfc moved: a change of the math library, not of k_observe (scripts/observe_truth_table.py records a new U)"


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OT.CASES)
def test_forward_against_truth(ctx, name):
    lam, f, g, edges, sigma, D = OT.hostile(name)
    t = OT.case_truth(name)
    got = forward(ctx, name)
    assert np.all(np.isfinite(got))
    twin = host_twin(ctx, lam, f, g, edges, sigma, D)
    print(f"{name}: host twin against the device path: {int(np.sum(twin != got))} pixels differ")
    OT.judge(name, "out", got, t.out, t.A, t.ratio, t.T, oref.observe(lam, f, edges, sigma, D, reference=g), OT.device_U())
    assert np.array_equal(twin, got)


SCALINGS = [("benign", 400), ("benign", -400), ("benign+ref", 400), ("benign+ref", -400), ("range_up", -400), ("range_up+ref", -400), ("range_down", 400),
            ("range_down+ref", 400), ("signed", 400), ("tail_spike+ref", -400)]


@pytest.mark.parametrize("name,k", SCALINGS)
def test_scaling_by_a_power_of_two_changes_no_mantissa(ctx, name, k):
    """every operation on f is a product or a sum: out(2^k f) == 2^k out(f), and with a reference out(2^k f, 2^k g) == out(f, g), bit for
    bit, as long as nothing leaves the normal range (asserted on the fp64 weights: the smallest |w f| 2^k is normal, the largest finite)"""
    lam, f, g, edges, sigma, D = OT.hostile(name)
    base = forward(ctx, name)
    s = 2.0 ** k
    smallest, largest = np.inf, 0.0
    for _, sl, w in aref.pixel_rows(lam, edges, sigma, D)[1]:
        for v in (f, g):
            if v is not None:
                terms = np.abs(w * v[sl])
                smallest, largest = min(smallest, terms[terms > 0].min()), max(largest, terms.sum())
    tiny, huge = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)
    print(f"{name}, 2^{k}: |w f| from {smallest:.3e} to {largest:.3e} before scaling")
    assert smallest * min(s, 1.0) > 1e3 * tiny and largest * max(s, 1.0) < 1e-3 * huge
    inst = instrument(ctx, name)
    if g is None:
        got = np.array(inst.observe_host(lam, f * s, None))
        assert np.all(np.abs(base) * min(s, 1.0) > tiny) and np.all(np.abs(base) * max(s, 1.0) < huge)
        print(f"out(2^k f) against 2^k out(f): {int(np.sum(got != base * s))} pixels differ")
        assert np.array_equal(got, base * s)
    else:
        got = np.array(inst.observe_host(lam, f * s, g * s))
        print(f"out(2^k f, 2^k g) against out(f, g): {int(np.sum(got != base))} pixels differ")
        assert np.array_equal(got, base)


# ---- adjoint ---------------------------------------------------------------------------------------------------------------------------
def device_adjoint(ctx, name, c, with_nus):
    lam, f, g, _, _, _ = OT.hostile(name)
    up = lambda a: None if a is None else ctx.upload(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    res = instrument(ctx, name).adjoint(up(lam), lam.size, up(c), flux=up(f) if g is not None else None, reference=up(g), nus=up(OT.nus_of(lam)) if with_nus else None,
                                        out_reference=g is not None)
    ctx.synchronize()
    return (np.array(res[0].numpy()), np.array(res[1].numpy())) if g is not None else (np.array(res.numpy()), None)


# every case with the pixel vector of its turn; the cases whose wrong versions only one vector exposes (tests/test_observe_truth_cpu.py:
# a 7.9 sigma window shows under `far_tail` alone, the end weights under the other two) with all three
ADJOINT_RUNS = [(name, OT.adjoint_kind(name)) for name in OT.CASES] + [
    (base + ref, kind) for base in ("tail_spike", "deep_core", "spacing_ends") for ref in ("", "+ref") for kind in OT.C_KINDS if kind != OT.adjoint_kind(base)]
DOT_ROUNDINGS = 4  # w f and the quotient on the forward side, c / den and w a on the adjoint's


@pytest.mark.parametrize("with_nus", [False, True], ids=["", "nus"])
@pytest.mark.parametrize("name,kind", ADJOINT_RUNS)
def test_adjoint_against_truth(ctx, name, kind, with_nus):
    lam, f, g, edges, sigma, D = OT.hostile(name)
    c = OT.pixel_vector(name, kind)
    t = OT.case_adjoint_truth(name, kind, with_nus)
    U = OT.device_U()
    w_flux, w_ref = device_adjoint(ctx, name, c, with_nus)
    r_flux, r_ref = OT.restated_adjoint(name, kind, with_nus)
    tag = f"{name}, c {kind}{', nus' if with_nus else ''}"
    assert (t.scale > 0).sum() > 10
    assert np.all(w_flux[t.scale == 0] == 0.0)  # a point in no window of a pixel with weight: exactly 0
    OT.judge(tag, "w_flux", w_flux, t.w_flux, t.scale, t.ratio, t.T, r_flux, U)
    if g is not None:
        assert np.all(w_ref[t.scale_ref == 0] == 0.0)
        OT.judge(tag, "w_reference", w_ref, t.w_ref, t.scale_ref, t.ratio_ref, t.T_ref, r_ref, U)
    # <observe(f), c> = <f, adjoint(c)> of the device's own two outputs, the two dot products formed at the truth's precision.  Both sides
    # are sums of the same products c_j w_ij f_i / den_j, with w_ij and den_j the same bits on either side (the header: "bit for bit the
    # weight of k_observe's loop"), so neither erf / erfc nor an argument's rounding enters: what is left is the rounding of w f, of the sum
    # of depth T_j and of the quotient on one side, of c / den, of w a and of the sum of depth T_i (with nus: two more) on the other,
    #     |lhs - rhs| <= sum_j (T_j + T_i + 4) 2^-53 |c_j| sum_i |w_ij f_i| / |den_j|
    out, fw, R = forward(ctx, name), t.forward, t.forward.rows
    back = [M.mpf(1)] * lam.size if not with_nus else [M.mpf(float(a)) / M.mpf(float(b)) for a, b in zip(lam, OT.nus_of(lam))]  # weights over F_nu apply to F_lambda lambda / nu
    lhs = M.fsum(M.mpf(float(a)) * M.mpf(float(b)) for a, b in zip(c, out))
    rhs = M.fsum(M.mpf(float(a)) * M.mpf(float(b)) * k for a, b, k in zip(w_flux, f, back))
    per_pixel = [abs(float(c[j])) / abs(fw.den[j]) * M.fsum(abs(w * float(v)) for w, v in zip(R.w[j], f[R.i0[j]:R.i1[j]])) for j in range(OT.PER_CLASS)]
    terms = float(M.fsum(per_pixel))
    granted = float(M.fsum((float(fw.T[j]) + float(t.T[0]) + DOT_ROUNDINGS) * OT.EPS * per_pixel[j] for j in range(OT.PER_CLASS)))
    print(f"{tag}: <observe(f), c> = {float(lhs):.15e}, <f, adjoint(c)> = {float(rhs):.15e}, difference {float(abs(lhs - rhs)):.3e} = {float(abs(lhs - rhs)) / terms:.3e} of "
          f"sum |c w f / den| (fp64 restatement of that sum: {aref.dot_terms(lam, c, f, edges, sigma, D, reference=g):.6e}), granted {granted / terms:.3e}")
    OT.RECORD.append(dict(case=tag, quantity="dot identity", label="kernel", kernel=float(abs(lhs - rhs)) / terms, restatement=None, allowance=granted / terms,
                          worst_ratio=float(abs(lhs - rhs)) / granted))
    assert terms > 0 and abs(lhs - rhs) <= granted
