"""The response for a cotangent per (angle, frequency) on the device (sdx_response_angles_dev / _f64, ops.response_angles): k_response
with a compile-time flag, a ray's terms weighted with cot[theta][nu] where the flux weight stands otherwise.

On formal_solution_truth.case(5, 20, per_class=4) — hostile columns — and at n_theta = 1 and 64 with two depth points, the fewest the
kernel takes.  What is checked, every figure printed before it is asserted:
  cot[theta][nu] = w_theta reproduces sdx_response_dev bit for bit, both outputs and with either output NULL;
  a random cot against sum_theta cot[theta][nu] R_theta, R_theta from the n_theta calls of sdx_response_dev with one-hot weights (a
    one-hot call's theta sum adds zeros: R_theta is the ray's own term, the device's operand): the products cot R_theta formed in fp64
    are the device's, so only the fp64 theta sum differs from their sum in longdouble: n_theta 2^-52 sum_theta |cot R_theta|;
  sum_k R_source[k] S[k] against sum_theta cot I_theta (sdx_emergent_intensity_dev) on the finite columns: the distance of the one-hot
    sum above from the same right-hand side, plus the theta sum's rounding carried through the depth sum;
  two calls, a graph replay, the host-buffer twin bit for bit; the refusals."""
import numpy as np
import pytest

import formal_solution_truth as T
import response_truth as R
from stardis_amd import ops
from test_gpu_observe_tangent import capture
from test_gpu_response import profiled

pytestmark = pytest.mark.gpu

L = T.L
SHAPES = [(5, 20), (2, 1), (2, 64)]
_shared = {}


@pytest.fixture(autouse=True)
def extended_precision():
    if not T.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


def setup(ctx, n_depth, n_theta):
    """the case, a source plane, a random cotangent and the one-hot responses R_theta: computed once per shape, left unchanged"""
    key = (n_depth, n_theta)
    if key not in _shared:
        c = T.case(n_depth, n_theta, per_class=4)
        S = R.source_plane(c.nus, c.temps) * np.random.default_rng(n_theta).uniform(0.3, 3.0, (n_depth, c.n_nu))
        cot = np.random.default_rng(7 + n_theta).standard_normal((n_theta, c.n_nu))
        one_hot = []
        for th in range(n_theta):
            e = np.zeros(n_theta)
            e[th] = 1.0
            one_hot.append(ops.response(c.nus, c.temps, c.ray, e, c.alphas, ctx=ctx, source=S))
        Ra = np.stack([a for a, _ in one_hot])  # (n_theta, n_depth, n_nu)
        Rs = np.stack([s for _, s in one_hot])
        for a in (S, cot, Ra, Rs):
            a.setflags(write=False)
        _shared[key] = (c, S, cot, Ra, Rs)
    return _shared[key]


@pytest.mark.parametrize("n_depth,n_theta", SHAPES)
def test_flux_weights_reproduce_the_flux_response_bit_for_bit(ctx, n_depth, n_theta):
    c, S, _, _, _ = setup(ctx, n_depth, n_theta)
    cot = np.repeat(np.asarray(c.weights, dtype=np.float64)[:, None], c.n_nu, axis=1)
    for source in (None, S):
        Ra, Rs = ops.response(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx, source=source)
        Ga, Gs = ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=source)
        assert np.array_equal(Ga, Ra, equal_nan=True) and np.array_equal(Gs, Rs, equal_nan=True)
        assert np.isfinite(Ra).any() and np.any(Ra[np.isfinite(Ra)] != 0) and np.any(Rs[np.isfinite(Rs)] != 0)
        only_a, none = ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=source, want_source=False)
        assert none is None and np.array_equal(only_a, Ra, equal_nan=True)
        none, only_s = ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=source, want_opacity=False)
        assert none is None and np.array_equal(only_s, Rs, equal_nan=True)


@pytest.mark.parametrize("n_depth,n_theta", SHAPES)
def test_random_cotangent_against_the_one_hot_sum(ctx, n_depth, n_theta):
    c, S, cot, Ra1, Rs1 = setup(ctx, n_depth, n_theta)
    got = ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=S)
    for name, a, one in (("R_alpha", got[0], Ra1), ("R_source", got[1], Rs1)):
        with np.errstate(all="ignore"):
            prod = cot[:, None, :] * one  # fp64: the device's products
            want, terms = prod.astype(L).sum(axis=0), np.abs(prod).astype(L).sum(axis=0)
        finite = np.isfinite(terms.astype(np.float64))
        assert np.array_equal(np.isfinite(a), finite)  # a column the formulas leave inf / NaN is that in both
        allow = n_theta * 2.0 ** -52 * terms[finite]
        err = np.abs(a[finite].astype(L) - want[finite])
        exact = allow == 0
        assert np.all(err[exact] == 0)
        worst = float((err[~exact] / allow[~exact]).max()) if (~exact).any() else 0.0
        print(f"{name} {n_depth}/{n_theta}: {int(finite.sum())} finite values of {finite.size}, worst |device - one-hot sum| / allowance = {worst:.3e}")
        assert worst <= 1.0 and finite.any()


@pytest.mark.parametrize("n_depth,n_theta", SHAPES)
def test_source_identity(ctx, n_depth, n_theta):
    """sum_k R_source[k] S[k] = sum_theta cot[theta] I_theta: the emergent intensity is linear in the source function"""
    c, S, cot, _, Rs1 = setup(ctx, n_depth, n_theta)
    _, Rs = ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=S, want_opacity=False)
    I = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx, source=S)
    with np.errstate(all="ignore"):
        rhs = (cot.astype(L) * I.astype(L)).sum(axis=0)
        prod = cot[:, None, :] * Rs1
        restated = (prod.astype(L).sum(axis=0) * S.astype(L)).sum(axis=0)
        carried = n_theta * 2.0 ** -52 * (np.abs(prod).astype(L).sum(axis=0) * np.abs(S).astype(L)).sum(axis=0)
        lhs = (Rs.astype(L) * S.astype(L)).sum(axis=0)
    ok = np.isfinite(rhs.astype(np.float64)) & np.isfinite(restated.astype(np.float64)) & np.isfinite(lhs.astype(np.float64))
    allow = np.abs(restated - rhs)[ok] + carried[ok]
    err = np.abs(lhs - rhs)[ok]
    assert np.all(err[allow == 0] == 0)
    some = allow > 0
    worst = float((err[some] / allow[some]).max())
    rel = float((err[some] / np.maximum(np.abs(rhs[ok][some]), L(1e-300))).max())
    print(f"sum R_source S against sum cot I {n_depth}/{n_theta}: {int(ok.sum())} finite columns of {c.n_nu}; worst / allowance = {worst:.3e} "
          f"(relative to the right-hand side up to {rel:.2e})")
    assert worst <= 1.0 and ok[np.isin(c.cls, R.OPAQUE)].all()


def test_same_bits_twice_replayed_and_from_the_host_twin(ctx):
    c, S, cot, _, _ = setup(ctx, 5, 20)
    n, ld = c.n_nu, c.n_nu + 3
    padded = np.zeros((20, ld))
    padded[:, :n] = cot
    d = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (c.nus, c.temps, c.ray, padded, c.alphas, S)]
    Ra, Rs = ctx.empty((5, n)), ctx.empty((5, n))
    run = lambda: ctx.call("sdx_response_angles_dev", 5, n, 20, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, ld, d[4].ptr, n, d[5].ptr, n,  # noqa: E731
                           Ra.ptr, n, Rs.ptr, n)
    result = lambda: (np.array(Ra.numpy()), np.array(Rs.numpy()))  # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))  # noqa: E731
    run()
    eager = result()
    run()
    assert same(eager, result())
    graph = capture(ctx, run)
    try:
        Ra.zero(), Rs.zero()
        ctx.call("sdx_graph_launch", graph)
        replay = result()
        padded[:, :n] = np.asarray(c.weights, dtype=np.float64)[:, None]
        d[3].set(padded)  # the cotangent is read when the kernel runs: rewritten to the flux weights, the replay is the flux's response
        ctx.call("sdx_graph_launch", graph)
        rewritten = result()
    finally:
        ctx.call("sdx_graph_destroy", graph)
    assert same(replay, eager) and same(rewritten, ops.response(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx, source=S))
    assert not same(rewritten, eager)
    assert same(ops.response_angles(c.nus, c.temps, c.ray, cot, c.alphas, ctx=ctx, source=S), eager)
    out_a, out_s = np.full((5, n), np.nan), np.full((5, n), np.nan)
    h = [np.ascontiguousarray(a, dtype=np.float64) for a in (c.nus, c.temps, c.ray, cot, c.alphas, S)]
    ctx.call("sdx_response_angles_f64", 5, n, 20, *(a.ctypes.data for a in h), out_a.ctypes.data, out_s.ctypes.data)
    assert same((out_a, out_s), eager)
    only = np.full((5, n), np.nan)
    ctx.call("sdx_response_angles_f64", 5, n, 20, *(a.ctypes.data for a in h), None, only.ctypes.data)
    assert np.array_equal(only, eager[1], equal_nan=True)


def test_refusals_enqueue_nothing(ctx):
    c, S, cot, _, _ = setup(ctx, 5, 20)
    n = c.n_nu
    d = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (c.nus, c.temps, c.ray, cot, c.alphas)]
    out, out2 = ctx.empty((5, n)), ctx.empty((5, n))

    def call(n_depth=5, n_theta=20, Ra=out.ptr, Rs=out2.ptr, n_nu=n, cot_ld=n, ald=n, rld=n, cot_ptr=d[3].ptr):
        ctx.call("sdx_response_angles_dev", n_depth, n_nu, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, cot_ptr, cot_ld, d[4].ptr, ald, None, 0, Ra, rld,
                 Rs, n)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for n_nu in (n, 0):  # also at set-up time, with an empty grid
                with pytest.raises(ValueError, match="mixed_precision"):
                    call(n_nu=n_nu)
        finally:
            ctx.set_option("mixed_precision", 0)
        for n_nu in (n, 0):
            with pytest.raises(ValueError, match="64 angles"):
                call(n_theta=65, n_nu=n_nu)
            with pytest.raises(ValueError, match="deep"):
                call(n_depth=1000, n_nu=n_nu)
        with pytest.raises(ValueError, match="no output"):
            call(Ra=None, Rs=None)
        with pytest.raises(ValueError, match="cot_ld"):
            call(cot_ld=n - 1)
        for kw in (dict(cot_ptr=None), dict(ald=n - 1), dict(rld=n - 1), dict(Ra=d[3].ptr)):
            with pytest.raises(ValueError):
                call(**kw)
        ctx.synchronize()
        assert ctx.profile("k_response_angles")[0] == 0 and ctx.profile("k_response")[0] == 0
        call()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile("k_response_angles")[0] == 1 and ctx.profile("k_response")[0] == 0
    with pytest.raises(ValueError):
        ops.response_angles(c.nus, c.temps, c.ray, cot[:, :-1], c.alphas, ctx=ctx)
    with pytest.raises(ValueError):
        ops.response_angles(c.nus, c.temps, c.ray[:, :-1], cot, c.alphas, ctx=ctx)
