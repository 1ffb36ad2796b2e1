"""Emergent intensity of every ray on the device (sdx_emergent_intensity_dev, sdx_emergent_intensity_f64, ops.emergent_intensity): the
surface row of the I_nus volume without the volume.

The kernel runs the device functions of the plain formal-solution kernel (k_raytrace<1>) on the same operands in the same order, so the
check is equality of bits with row N_d - 1 of the I_nus that ops.raytrace_arrays(track=True) returns from that kernel ("segmented_raytrace"
= 0: at these sizes the default would be the segmented kernel, whose intensities differ by the rounding of its composition).  The hostile
columns of tests/formal_solution_truth.py and their 80-bit judgement are carried by the I_nus path (tests/test_gpu_formal_solution_truth.py);
equality of bits transfers them."""
import contextlib

import numpy as np
import pytest

import formal_solution_truth as T
from stardis_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (3, 3), (5, 20), (56, 20), (12, 64)]
LANE = "k_raytrace<1>"


@contextlib.contextmanager
def plain_kernel(ctx):
    """the launches inside take k_raytrace<1> (profiled, for the launch label); restored afterwards"""
    ctx.set_option("segmented_raytrace", 0)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        yield
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)


def last_row(ctx, c, nus, alphas, source=None):
    """row N_d - 1 of I_nus from the plain kernel, as (N_theta, N_nu)"""
    with plain_kernel(ctx):
        _, I = ops.raytrace_arrays(nus, c.temps, c.ray, c.weights, alphas, track=True, ctx=ctx, inward_rays=c.spherical,
                                   photospheric_correction=c.correction if c.spherical else 1.0, source=source)
        assert ctx.profile_variant("k_raytrace") == LANE
    return np.ascontiguousarray(I[-1].T)


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("n_depth,n_theta", SHAPES)
def test_bits_of_the_last_row_plane_parallel(ctx, n_depth, n_theta):
    c = T.case(n_depth, n_theta, per_class=4)
    want = last_row(ctx, c, c.nus, c.alphas)
    with plain_kernel(ctx):
        got = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx)
        assert ctx.profile("k_emergent_intensity")[0] == 1 and ctx.profile("k_raytrace")[0] == 0
    assert got.shape == (n_theta, c.n_nu)
    print(f"{n_depth}/{n_theta}: {c.n_nu} columns, {int(np.isfinite(want).sum())} finite values of {want.size}")
    assert same_bits(got, want) and np.isfinite(want).any() and np.any(want[np.isfinite(want)] != 0)
    # the host-buffer twin: the same kernel, the same bits
    twin = np.full((n_theta, c.n_nu), np.nan)
    p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data  # noqa: E731
    nus, t, ray, alphas = (np.ascontiguousarray(a, dtype=np.float64) for a in (c.nus, c.temps, c.ray, c.alphas))
    ctx.call("sdx_emergent_intensity_f64", n_depth, c.n_nu, n_theta, p(nus), p(t), p(ray), p(alphas), None, 0, twin.ctypes.data)
    assert same_bits(twin, want)
    # a device plane in, a device array out
    d_I = ops.emergent_intensity(c.nus, c.temps, c.ray, ctx.upload(alphas), ctx=ctx, device=True)
    assert same_bits(d_I.numpy(), want)


def test_bits_of_the_last_row_spherical(ctx):
    c = T.case(9, 20, per_class=4, spherical=True)
    want = last_row(ctx, c, c.nus, c.alphas)
    got = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx, inward_rays=True)
    assert same_bits(got, want) and np.isfinite(want).any()
    outward_only = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx)
    assert not same_bits(outward_only, want)  # (the inward sweep is part of the answer)


def test_bits_with_a_source_plane(ctx):
    c = T.case(5, 20, per_class=4)
    rng = np.random.default_rng(11)
    source = ops.blackbody_flux_at_nu(c.nus, c.temps, ctx=ctx) * rng.uniform(0.5, 1.5, (c.n_depth, c.n_nu))
    want = last_row(ctx, c, c.nus, c.alphas, source=source)
    got = ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx, source=source)
    assert same_bits(got, want)
    assert not same_bits(got, ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx))


@pytest.mark.parametrize("n_nu", [1, 63, 65])
def test_partial_waves_and_groups(ctx, n_nu):
    """20 angles: three frequencies per wave, twelve per workgroup — 1 is a partial wave, 63 and 65 end in a partial group"""
    c = T.case(5, 20, per_class=4)
    reps = -(-n_nu // c.n_nu)
    alphas = np.ascontiguousarray(np.tile(c.alphas, (1, reps))[:, :n_nu])
    nus = np.linspace(7.5e14, 3.0e14, n_nu) if n_nu > 1 else np.array([5.0e14])
    want = last_row(ctx, c, nus, alphas)
    # a guard row behind every angle's spectrum: the leading dimension is honoured and nothing is written past n_nu
    ld = n_nu + 3
    d_I = ctx.upload(np.full((20, ld), -7.0))
    d = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (nus, c.temps, c.ray, alphas)]
    ctx.call("sdx_emergent_intensity_dev", c.n_depth, n_nu, 20, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n_nu, None, 0, 0, d_I.ptr, ld)
    out = d_I.numpy()
    assert same_bits(np.ascontiguousarray(out[:, :n_nu]), want) and np.all(out[:, n_nu:] == -7.0)
    assert same_bits(ops.emergent_intensity(nus, c.temps, c.ray, alphas, ctx=ctx), want)


def test_refusals(ctx):
    c = T.case(3, 3, per_class=4)
    empty = lambda n_depth, n_theta: ctx.call("sdx_emergent_intensity_dev", n_depth, 0, n_theta, None, None, None, None, 0, None, 0, 0, None, 0)  # noqa: E731
    empty(56, 20)  # (an empty grid asks at set-up time: served)
    ctx.set_option("mixed_precision", 1)
    try:
        with pytest.raises(ValueError, match="mixed_precision"):
            empty(56, 20)
        with pytest.raises(ValueError, match="mixed_precision"):
            ops.emergent_intensity(c.nus, c.temps, c.ray, c.alphas, ctx=ctx)
    finally:
        ctx.set_option("mixed_precision", 0)
    with pytest.raises(ValueError, match="64 angles"):
        empty(5, 65)
    with pytest.raises(ValueError, match="LDS"):
        empty(5000, 20)
    d = [ctx.upload(np.ascontiguousarray(a, dtype=np.float64)) for a in (c.nus, c.temps, c.ray, c.alphas)]
    with pytest.raises(ValueError, match="not in place"):
        ctx.call("sdx_emergent_intensity_dev", c.n_depth, c.n_nu, 3, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, c.n_nu, None, 0, 0, d[3].ptr, c.n_nu)
