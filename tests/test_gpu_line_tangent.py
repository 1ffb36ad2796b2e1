"""The tangent of the line-opacity sum on the device (sdx_line_tangent_dev, sdx_line_tangent_f64, ops.line_tangent,
SpectralSynthesizer.line_tangent / flux_tangent / microturbulence_tangent / observed_line_jacobian / chi2_joint_gradient).

The kernel is judged by the restatement of tests/line_tangent_reference.py (tests/test_line_tangent_cpu.py checks what that rests on):
per element of the plane |got - ref| <= (OPACITY_RTOL + n_cover 2^-53) scale with the project's per-term parity OPACITY_RTOL = 1e-12,
n_cover the number of items whose window covers the element and the scale built from absolute pieces; an element without a scale is
exactly 0.0.  Models: line_adjoint_truth.SHAPES.  Every test prints its figures before it asserts."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import line_tangent_reference as R
from conftest import ROOT
from observe_reference import SUM_TOL  # identities between reordered sums: 1e-12 of the sum of the absolute terms
from stardis_amd import _lib, linelist as LL, ops, synth
from test_gpu_line_param_adjoint import C_LIGHT, H_NU, assert_windows_hold, flux_of, held_against_quotients, perturbed, richardson
from test_gpu_observe_adjoint import engine_instrument
from test_gpu_response import FLUX_PARITY, H, fixed_window_lines, model, profiled, synthesizer  # noqa: F401  (`model`: the module-scoped fixture)

pytestmark = pytest.mark.gpu

A, T = R.A, R.T
STAGE = "k_line_tangent"
TABLES = ("line_nus", "doppler_widths", "gammas", "alphas")
COMBOS = [("strength",), ("damping",), ("doppler",), ("centre",), R.NAMES]
# every stage name the library's launch sites carry
STEP_STAGES = sorted(set(re.findall(r'"(k_[a-z_0-9]+)"', open(os.path.join(ROOT, "stardis_amd", "csrc", "stardis_hip.hip")).read())))
assert STAGE in STEP_STAGES and "k_line_all" in STEP_STAGES and "k_raytrace" in STEP_STAGES


@functools.lru_cache(maxsize=None)
def reference(name, which, per_depth):
    return R.plane(name, **R.directions(name, per_depth, which))


def tangent(ctx, m, dirs, shard=None):
    """sdx_line_tangent_dev on the model's sorted tables, the output pre-filled with NaN -> the plane of the shard's columns"""
    order, ln, dw, g, al = R.sorted_tables(m)
    b, n = (0, m.n_nu) if shard is None else shard
    host, cols = ops.line_directions(m.n_lines, m.n_depth, **dirs)
    d = [ctx.upload(a) for a in (m.nus, ln, dw, g, al)]
    d_dirs = [None if v is None else ctx.upload(np.ascontiguousarray(v[order])) for v in host]
    out = ctx.empty((m.n_depth, n))
    out.set(np.full((m.n_depth, n), np.nan))
    ctx.call("sdx_line_tangent_dev", m.n_depth, m.n_nu, d[0].ptr, b, n, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, g.shape[1], d[4].ptr,
             *[_lib.ptr_of(v) for v in d_dirs], cols, out.ptr, n)
    ctx.synchronize()
    return np.array(out.numpy())


def judge(label, got, ref, factor=1.0):
    assert np.isfinite(got).all(), label  # (every element was written)
    ratio = R.worst_ratio(got, ref, factor)
    print(f"{label}: worst |got - ref| / bound {ratio:.3e} over {int((ref.scale > 0).sum())} elements, {int((ref.scale == 0).sum())} exact zeros, "
          f"up to {int(ref.n_cover.max())} items per element")
    assert ratio <= 1.0, (label, ratio)


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ALL_MODELS)
def test_against_the_reference(ctx, name):
    m = A.model(name)
    L = m.lines
    assert m.n_lines > 1 and (np.diff(L["line_nus"]) >= 0).all()  # (the models' lists ascend: ops reads them as they are)
    for j, which in enumerate(COMBOS):
        per_depth = bool((j + R.ALL_MODELS.index(name)) % 2)
        dirs = R.directions(name, per_depth, which)
        with profiled(ctx):
            got = tangent(ctx, m, dirs)
            assert ctx.profile(STAGE)[0] == 1
        judge(f"{name}, {'+'.join(which)}, per_depth={per_depth}", got, reference(name, tuple(which), per_depth))
        if len(which) > 1 or which == ("strength",):  # the other ways in: the same bits
            via_host = ops.line_tangent(*A.line_args(m), ctx=ctx, **dirs)
            cols = m.n_depth if per_depth else 1
            on_device = {k: ctx.upload(np.ascontiguousarray(np.broadcast_to(R.per_item(m, v)[:, :cols], (m.n_lines, cols)))) for k, v in dirs.items()}
            via_device = ops.line_tangent(*A.line_args(m), ctx=ctx, device=True, **on_device)
            twin = np.full((m.n_depth, m.n_nu), np.nan)
            host, cols = ops.line_directions(m.n_lines, m.n_depth, **dirs)
            _lib.check(ctx.lib.sdx_line_tangent_f64(ctx.handle, m.n_depth, m.n_nu, m.nus.ctypes.data, m.n_lines, L["line_nus"].ctypes.data,
                                                    L["doppler_widths"].ctypes.data, L["gammas"].ctypes.data, L["gammas"].shape[1], L["alphas"].ctypes.data,
                                                    *[None if v is None else v.ctypes.data for v in host], cols, twin.ctypes.data))
            assert np.array_equal(via_host, got) and np.array_equal(via_device.numpy(), got) and np.array_equal(twin, got)


# ---- 2. strength = 1 against the line opacity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "inner"])
def test_strength_one_is_the_line_opacity(ctx, name):
    m = A.model(name)
    mask = R.species_mask(name)
    ctx.set_option("far_field", 0)
    try:
        whole = ops.calc_alan_entries(*A.line_args(m), ctx=ctx)
        part = ops.calc_alan_entries(*A.line_args(m, mask == 1), ctx=ctx)
    finally:
        ctx.set_option("far_field", -1)
    ref_whole, ref_part = R.plane(name, strength=1.0), R.plane(name, strength=mask)
    diff = np.abs(tangent(ctx, m, dict(strength=1.0)) - whole)
    ratio = float((diff[ref_whole.scale > 0] / A.bound(ref_whole.scale, ref_whole.n_cover)[ref_whole.scale > 0]).max())
    print(f"{name}: tangent along strength = 1 against the line opacity, worst |difference| / bound {ratio:.3e}")
    assert ratio <= 1.0 and not diff[ref_whole.scale == 0].any()
    masked = tangent(ctx, m, dict(strength=mask))
    judge(f"{name}, a mask of {int(mask.sum())} lines", masked, ref_part)
    diff = np.abs(masked - part)
    ratio = float((diff[ref_part.scale > 0] / A.bound(ref_part.scale, ref_part.n_cover)[ref_part.scale > 0]).max())
    only_others = (ref_part.scale == 0) & (ref_whole.scale > 0)
    print(f"{name}: the masked tangent against the line opacity of the sub-list: {ratio:.3e}; {int(only_others.sum())} elements only the other lines cover")
    assert ratio <= 1.0 and not masked[ref_part.scale == 0].any() and not part[ref_part.scale == 0].any()
    if name != "inner":
        assert only_others.any()


# ---- 3. the dot identity on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged", "inner"])
def test_dot_identity(ctx, name):
    """sum W d alpha against the two adjoints contracted with the directions; each side judged against the extended-precision value of
    the restatement, so the two differ by at most the sum of the bounds"""
    m = A.model(name)
    per_depth = name != "ragged"
    dirs = R.directions(name, per_depth)
    ref = reference(name, tuple(R.NAMES), per_depth)
    got = tangent(ctx, m, dirs)
    s0 = ops.line_adjoint(*A.line_args(m), m.W, per_depth=True, ctx=ctx)
    par = ops.line_param_adjoint(*A.line_args(m), m.W, per_depth=True, ctx=ctx)
    restated = dict(strength=A.restated(name), damping=T.restated(name).damping, doppler=T.restated(name).doppler, centre=T.restated(name).centre)
    item = {k: R.per_item(m, v) for k, v in dirs.items()}
    left = float((m.W.astype(R.LD) * got.astype(R.LD)).sum())
    left_bound = float((np.abs(m.W) * A.bound(ref.scale, ref.n_cover)).sum())
    right, right_bound = R.LD(0), 0.0
    for k, s in (("strength", s0), ("damping", par["damping"]), ("doppler", par["doppler"]), ("centre", par["centre"])):
        right += (item[k].astype(R.LD) * s.astype(R.LD)).sum()
        right_bound += float((np.abs(item[k]) * A.bound(restated[k].scale_ld, restated[k].terms_ld)).sum())
    diff = abs(left - float(right))
    print(f"{name}: sum W d alpha {left:+.9e}, adjoints {float(right):+.9e}, |difference| {diff:.3e}, bounds {left_bound:.3e} + {right_bound:.3e}: "
          f"ratio {diff / (left_bound + right_bound):.3e}")
    assert left != 0.0 and diff <= left_bound + right_bound


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shards", [("small", ((0, 100), (100, 120), (220, 80))), ("inner", ((3000, 6000),))])
def test_shards_are_the_whole_grids_columns(ctx, name, shards):
    m = A.model(name)
    dirs = R.directions(name, name == "small")
    whole = tangent(ctx, m, dirs)
    assert whole.any()
    for b, n in shards:
        part = tangent(ctx, m, dirs, shard=(b, n))
        assert part.shape == (m.n_depth, n) and np.array_equal(part, whole[:, b:b + n]), (name, b, n)
        via_ops = ops.line_tangent(*A.line_args(m), ctx=ctx, shard=(b, n), **dirs)
        assert np.array_equal(via_ops, part)


# ---- 5. order and duplicates -------------------------------------------------------------------------------------------------------
def test_any_order_and_duplicates(ctx):
    m = A.model("small")
    dirs = R.directions("small", True)
    L = {k: np.concatenate([m.lines[k], m.lines[k][7:8]]) for k in TABLES}  # line 7 twice: equal frequencies, a stable sort keeps their order
    dirs = {k: np.concatenate([v, 0.5 * v[7:8]]) for k, v in dirs.items()}
    order = np.argsort(L["line_nus"], kind="stable")
    sorted_call = ops.line_tangent(m.n_depth, m.nus, *[np.ascontiguousarray(L[k][order]) for k in TABLES], ctx=ctx,
                                   **{k: np.ascontiguousarray(v[order]) for k, v in dirs.items()})
    shuffle = np.random.default_rng(3).permutation(m.n_lines + 1)
    shuffle = np.concatenate([shuffle[shuffle != m.n_lines], [m.n_lines]])  # (the copy stays behind the original, as the stable sort leaves it)
    mixed = ops.line_tangent(m.n_depth, m.nus, *[np.ascontiguousarray(L[k][shuffle]) for k in TABLES], ctx=ctx,
                             **{k: np.ascontiguousarray(v[shuffle]) for k, v in dirs.items()})
    assert np.array_equal(mixed, sorted_call) and sorted_call.any()
    # the duplicate adds half of line 7's own plane
    alone = ops.line_tangent(*A.line_args(m), ctx=ctx, **{k: np.where(np.arange(m.n_lines)[:, None] == 7, v[:m.n_lines], 0.0) for k, v in dirs.items()})
    base = ops.line_tangent(*A.line_args(m), ctx=ctx, **{k: v[:m.n_lines] for k, v in dirs.items()})
    ref = reference("small", tuple(R.NAMES), True)
    assert np.all(np.abs(sorted_call - (base + 0.5 * alone)) <= 2 * A.bound(ref.scale, ref.n_cover + 1))
    with pytest.raises(ValueError, match="ascending"):
        ops.line_tangent(m.n_depth, m.nus, *[np.ascontiguousarray(L[k][shuffle]) for k in TABLES], ctx=ctx, strength=ctx.upload(np.ones(m.n_lines + 1)))


# ---- 6. determinism and capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "inner"])
def test_determinism_and_capture(ctx, name):
    m = A.model(name)
    dirs = R.directions(name, name == "ragged")
    first, again = tangent(ctx, m, dirs), tangent(ctx, m, dirs)  # (the first call is the warm-up: the scratch has its size)
    assert np.array_equal(first, again) and first.any()
    order, ln, dw, g, al = R.sorted_tables(m)
    host, cols = ops.line_directions(m.n_lines, m.n_depth, **dirs)
    d = [ctx.upload(a) for a in (m.nus, ln, dw, g, al)]
    d_dirs = [ctx.upload(np.ascontiguousarray(v[order])) for v in host]
    out = ctx.zeros((m.n_depth, m.n_nu))
    ctx.call("sdx_graph_begin")
    try:
        ctx.call("sdx_line_tangent_dev", m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, g.shape[1], d[4].ptr,
                 *[v.ptr for v in d_dirs], cols, out.ptr, m.n_nu)
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    ctx.synchronize()
    assert not out.numpy().any()  # recorded, not run
    for _ in range(2):
        out.zero()
        ctx.call("sdx_graph_launch", graph)
        ctx.synchronize()
        assert np.array_equal(out.numpy(), first)
    ctx.call("sdx_graph_destroy", graph)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    m = A.model("odd")
    order, ln, dw, g, al = R.sorted_tables(m)
    d = [ctx.upload(a) for a in (m.nus, ln, dw, g, al)]
    ones = ctx.upload(np.ones((m.n_lines, m.n_depth)))
    sentinel = np.full((m.n_depth, m.n_nu), -7.25)
    out = ctx.upload(sentinel)
    four = [ones.ptr, None, ones.ptr, None]

    def call(n_nu=m.n_nu, begin=0, count=None, gamma_cols=m.n_depth, dirs=four, dir_cols=m.n_depth, n_lines=m.n_lines, n_depth=m.n_depth):
        count = n_nu if count is None else count
        ctx.call("sdx_line_tangent_dev", n_depth, n_nu, d[0].ptr, begin, count, n_lines, d[1].ptr, d[2].ptr, d[3].ptr, gamma_cols, d[4].ptr, *dirs, dir_cols,
                 out.ptr, m.n_nu)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for n_nu in (m.n_nu, 0):  # also at set-up time, with an empty grid
                with pytest.raises(ValueError, match="mixed_precision"):
                    call(n_nu=n_nu)
        finally:
            ctx.set_option("mixed_precision", 0)
        for n_nu in (m.n_nu, 0):
            with pytest.raises(ValueError, match="no direction"):
                call(n_nu=n_nu, dirs=[None] * 4)
            with pytest.raises(ValueError, match="directions must have"):
                call(n_nu=n_nu, dir_cols=2)
            with pytest.raises(ValueError, match="gammas"):
                call(n_nu=n_nu, gamma_cols=2)
            with pytest.raises(ValueError, match="shard"):
                call(n_nu=n_nu, begin=1, count=n_nu)
        with pytest.raises(ValueError, match="shard"):
            call(begin=-1, count=5)
        with pytest.raises(ValueError, match="int32"):  # the int32 limits
            call(n_nu=1 << 31, count=m.n_nu)
        with pytest.raises(ValueError, match="fit int32"):
            call(n_lines=1 << 31)
        with pytest.raises(ValueError, match="n_depth"):
            call(n_depth=0, gamma_cols=0, dir_cols=0)
        assert ctx.lib.sdx_line_tangent_dev(None, m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, m.n_depth, d[4].ptr,
                                            *four, m.n_depth, out.ptr, m.n_nu) == -1
        call(begin=5, count=0)  # an empty shard: nothing is launched
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 0 and np.array_equal(out.numpy(), sentinel)
        call(n_lines=0)  # no lines: the zeros are still written
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 1 and not out.numpy().any()
        call()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 2
    judge("after the refusals", np.array(out.numpy()), R.plane("odd", strength=1.0, doppler=1.0))


# ---- 8. the engine -----------------------------------------------------------------------------------------------------------------
def test_engine_dense_list_line_list_and_order(ctx, model):
    """a LineList synthesizer and the dense synthesizer built from LL.line_params of the same list: bit for bit; an unsorted dense
    list takes its directions in the caller's order; a shard returns its own columns"""
    m = model
    ll = synth.synth_linelist(m.nus, m.atm, 30, seed=7, mix=(0.5, 0.4, 0.1))
    a, g, dw = LL.line_params(ll, ctx=ctx)
    rng = np.random.default_rng(4)
    dirs = dict(strength=rng.standard_normal(30), damping=rng.standard_normal((30, 12)), doppler=0.3, centre=rng.standard_normal(30) * 1e8)
    dense = dict(line_nus=ll.nu, doppler_widths=dw, gammas=g, alphas=a)
    out = []
    for lines in (ll, dense):
        syn = synthesizer(ctx, m, lines, keep_response=True)
        syn.step()
        ctx.synchronize()
        out.append((np.array(syn.line_tangent(**dirs).numpy()), np.array(syn.flux_tangent(**dirs).numpy()), np.array(syn.microturbulence_tangent(1.2e5).numpy())))
        assert not syn.microturbulence_tangent(0.0).numpy().any()
        syn.close()
    for got_ll, got_dense in zip(*out):
        assert np.array_equal(got_ll, got_dense) and np.isfinite(got_dense).all() and got_dense.any()
    assert out[1][0].shape == (12, 300) and out[1][1].shape == (300,) and out[1][2].shape == (300,)
    assert np.array_equal(out[1][0], ops.line_tangent(12, m.nus, ll.nu, dw, g, a, ctx=ctx, **dirs))
    shuffle = rng.permutation(30)
    mixed = synthesizer(ctx, m, {k: np.ascontiguousarray(v[shuffle]) for k, v in dense.items()}, keep_response=True)
    mixed.step()
    ctx.synchronize()
    moved = {k: (v if np.ndim(v) == 0 else np.ascontiguousarray(v[shuffle])) for k, v in dirs.items()}
    assert np.array_equal(mixed.line_tangent(**moved).numpy(), out[1][0]) and np.array_equal(mixed.microturbulence_tangent(1.2e5).numpy(), out[1][2])
    mixed.close()
    part = synthesizer(ctx, m, dense, keep_response=True, shard=(100, 120))
    part.step()
    ctx.synchronize()
    assert np.array_equal(part.line_tangent(**dirs).numpy(), out[1][0][:, 100:220]) and np.array_equal(part.flux_tangent(**dirs).numpy(), out[1][1][100:220])
    part.close()
    plain = synthesizer(ctx, m, dense)
    assert plain.line_tangent(strength=1.0).shape == (12, 300)  # the plane needs no response functions; its projection does
    with pytest.raises(RuntimeError, match="keep_response=True"):
        plain.flux_tangent(strength=1.0)
    plain.close()


def test_engine_species_mask_and_microturbulence(ctx, model):
    m = model
    syn = synthesizer(ctx, m, keep_response=True)
    syn.step()
    ctx.synchronize()
    F_last = np.array(syn.F_nu()[-1])
    mask = np.zeros(40)
    mask[m.x_lines] = 1.0
    got, expect = np.array(syn.flux_tangent(strength=mask).numpy()), np.array(syn.flux_derivative(m.alpha_x).numpy())
    worst = float(np.abs(got - expect).max())
    print(f"flux_tangent(strength=mask of X) against flux_derivative(alpha_X): max |difference| {worst:.3e}, max |derivative| {np.abs(expect).max():.3e}, "
          f"allowed {FLUX_PARITY * np.abs(F_last).max():.3e}")
    assert worst <= FLUX_PARITY * np.abs(F_last).max() and np.abs(expect).max() > 1e3 * FLUX_PARITY * np.abs(F_last).max()
    # forward against reverse: sum_i w_i microturbulence_tangent(xi)_i = microturbulence_sensitivity(xi, w)
    xi = 1.5e5
    w = np.random.default_rng(2).standard_normal(300)
    forward = np.array(syn.microturbulence_tangent(xi).numpy())
    reverse = syn.microturbulence_sensitivity(xi, w)
    factor = xi * (m.lines["line_nus"] / C_LIGHT)[:, None] ** 2 / m.lines["doppler_widths"] ** 2
    # the bounds of both sides: the plane's and the items' per-term bounds carried through the projection weights |w R / total|
    Wp = np.abs(w[None, :] * np.array(syn.response_opacity.numpy()) / np.array(syn.total_alphas()))
    ref = R.plane("small", doppler=factor)
    q = T.restated("small", W=Wp).doppler
    assert np.array_equal(A.model("small").lines["line_nus"], m.lines["line_nus"])  # (the small model of the restatements is this one)
    bounds = float((Wp * A.bound(ref.scale, ref.n_cover)).sum()) + float((np.abs(factor) * A.bound(q.scale_ld, q.terms_ld)).sum())
    bounds += SUM_TOL * float((Wp * ref.scale).sum())  # (the weight plane, the projection and the host sums: the same terms in another order)
    left = float(np.sum(w.astype(R.LD) * forward))
    print(f"microturbulence: sum w tangent {left:+.9e}, sensitivity {reverse:+.9e}, |difference| {abs(left - reverse):.3e}, bounds {bounds:.3e}")
    assert left != 0.0 and abs(left - reverse) <= bounds
    syn.close()


@pytest.mark.parametrize("key", ["doppler", "centre"])
def test_engine_against_difference_quotients(ctx, model, key):
    """flux_tangent along ln doppler_width and the rest frequency of the fixed-window lines of species X against Richardson quotients
    of whole steps: the helpers and the acceptance rule of tests/test_gpu_line_param_adjoint.py"""
    m = model
    rows = np.intersect1d(m.x_lines, fixed_window_lines(m.nus, m.lines, np.exp(2 * H)))
    assert rows.size >= 6
    h = H_NU if key == "centre" else H
    flux = {}
    for step in (h, -h, h / 2, -h / 2):
        moved = perturbed(m.lines, rows, key, step)
        assert_windows_hold(m.nus, m.lines, moved, rows)
        flux[step] = flux_of(ctx, m, moved)
    coarse, fine = richardson(flux, h)
    syn = synthesizer(ctx, m, keep_response=True)
    syn.step()
    ctx.synchronize()
    F_last = np.array(syn.F_nu()[-1])
    direction = np.zeros(40)
    direction[rows] = 1.0
    tangent_columns = np.array(syn.flux_tangent(**{key: direction}).numpy())
    ok, seen = held_against_quotients(f"flux_tangent({key}), the lines of X", lambda w: float(np.sum(w * tangent_columns)), coarse, fine, F_last, h)
    syn.close()
    assert ok and seen


# ---- 9. forward against reverse through the instrument -----------------------------------------------------------------------------
def test_forward_against_reverse_through_the_instrument(ctx, model):
    m = model
    inst = engine_instrument(ctx, v=-8.0)
    syn = synthesizer(ctx, m, keep_response=True, instrument=inst)
    syn.step()
    ctx.synchronize()
    rng = np.random.default_rng(8)
    c = rng.standard_normal(25)
    obs = np.array(syn.observed.numpy())
    c[np.isnan(obs)] = 0.0
    xi = 1.5e5
    mask = np.zeros(40)
    mask[m.x_lines] = 1.0
    factor = xi * (m.lines["line_nus"] / C_LIGHT)[:, None] ** 2 / m.lines["doppler_widths"] ** 2
    directions = {"X": dict(strength=mask), "xi": dict(microturbulence=xi)}
    J = {k: np.array(v.numpy()) for k, v in syn.observed_line_jacobian(directions).items()}
    assert list(J) == ["X", "xi"] and all(v.shape == (25,) for v in J.values())
    assert np.array_equal(J["xi"], syn.observed_line_jacobian({"p": dict(doppler=factor)})["p"].numpy(), equal_nan=True)
    assert all(np.array_equal(np.isnan(v), np.isnan(obs)) for v in J.values())
    # the reverse route, and the bound of both: per-term bounds of the plane and of the items through the grid weights |w R / total|,
    # plus the projection's and the instrument's forward-against-transpose reordering, SUM_TOL of the sums of the absolute terms
    # (the instrument's: |c| against the tangent of |dF|, its weights being positive)
    dF = {"X": syn.flux_tangent(strength=mask).numpy(), "xi": syn.microturbulence_tangent(xi).numpy()}
    J_abs = {k: np.array(syn.observed_tangent(np.abs(v)).numpy()) for k, v in dF.items()}
    assert all((v[~np.isnan(v)] >= 0).all() for v in J_abs.values())
    w_grid = np.array(syn.pixel_weights_to_grid(c).numpy())
    Wp = np.abs(w_grid[None, :] * np.array(syn.response_opacity.numpy()) / np.array(syn.total_alphas()))
    for name, wrt, per_line in (("X", "strength", np.broadcast_to(mask[:, None], (40, 12))), ("xi", "doppler", factor)):
        reverse = float(np.sum(np.array(syn.observed_line_sensitivities(c, per_depth=True, wrt=wrt).numpy()).astype(R.LD) * per_line))
        forward = float(np.sum(np.where(np.isnan(obs), 0.0, c * J[name]).astype(R.LD)))
        ref = R.plane("small", **{wrt: per_line})
        q = A.restated("small", W=Wp) if wrt == "strength" else T.restated("small", W=Wp).doppler
        bounds = float((Wp * A.bound(ref.scale, ref.n_cover)).sum()) + float((np.abs(per_line) * A.bound(q.scale_ld, q.terms_ld)).sum())
        bounds += SUM_TOL * (float((Wp * ref.scale).sum()) + float(np.nansum(np.abs(c) * J_abs[name])))
        print(f"{name}: sum c J {forward:+.9e}, observed_line_sensitivities . direction {reverse:+.9e}, |difference| {abs(forward - reverse):.3e}, bounds {bounds:.3e}")
        assert forward != 0.0 and abs(forward - reverse) <= bounds
    # the joint gradient
    data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(obs.size))
    ivar = rng.uniform(0.5, 2.0, obs.size) / np.nanmax(np.abs(obs)) ** 2
    chi2_i, grad_i, H_i = syn.chi2_instrument_gradient(data, ivar, ("v_rad", "lsf"), curvature=True)
    same = syn.chi2_joint_gradient(data, ivar, ("v_rad", "lsf"), curvature=True)
    assert same[0] == chi2_i and same[1] == grad_i and np.array_equal(same[2], H_i)
    chi2, grad, Hm = syn.chi2_joint_gradient(data, ivar, ("v_rad", "lsf"), directions, curvature=True)
    assert chi2 == chi2_i and list(grad) == ["v_rad", "lsf", "X", "xi"] and Hm.shape == (4, 4)
    assert np.array_equal(Hm, Hm.T) and np.array_equal(Hm[:2, :2], H_i) and all(grad[k] == grad_i[k] for k in grad_i) and (np.diag(Hm) > 0).all()
    assert syn.chi2_joint_gradient(data, ivar, (), directions)[1] == {k: grad[k] for k in ("X", "xi")}
    use = ~np.isnan(obs) & (ivar != 0)
    cc = -2.0 * np.where(use, ivar, 0.0) * (np.where(use, data, 0.0) - np.where(use, obs, 0.0))
    w_grid = np.array(syn.pixel_weights_to_grid(cc).numpy())
    Wp = np.abs(w_grid[None, :] * np.array(syn.response_opacity.numpy()) / np.array(syn.total_alphas()))
    for name, wrt, per_line in (("X", "strength", np.broadcast_to(mask[:, None], (40, 12))), ("xi", "doppler", factor)):
        reverse = float(np.sum(np.array(syn.chi2_line_gradient(data, ivar, per_depth=True, wrt=wrt)[1].numpy()).astype(R.LD) * per_line))
        ref = R.plane("small", **{wrt: per_line})
        q = A.restated("small", W=Wp) if wrt == "strength" else T.restated("small", W=Wp).doppler
        bounds = float((Wp * A.bound(ref.scale, ref.n_cover)).sum()) + float((np.abs(per_line) * A.bound(q.scale_ld, q.terms_ld)).sum())
        bounds += SUM_TOL * (float((Wp * ref.scale).sum()) + float(np.nansum(np.abs(cc) * J_abs[name])))
        print(f"chi2, {name}: joint gradient {grad[name]:+.9e}, chi2_line_gradient . direction {reverse:+.9e}, |difference| {abs(grad[name] - reverse):.3e}, bounds {bounds:.3e}")
        assert grad[name] != 0.0 and abs(grad[name] - reverse) <= bounds
    with pytest.raises(ValueError, match="unknown parameter"):
        syn.observed_jacobian("X")
    with pytest.raises(ValueError, match="reuses"):
        syn.chi2_joint_gradient(data, ivar, ("v_rad",), {"v_rad": dict(strength=mask)})
    syn.close()


# ---- 10. a step is unchanged -------------------------------------------------------------------------------------------------------
def test_a_step_is_unchanged(ctx, model):
    m = model
    outputs, counts = [], []
    for ask in (False, True):
        syn = synthesizer(ctx, m, keep_response=True)
        with profiled(ctx):
            syn.step()
            ctx.synchronize()
            first = {k: ctx.profile(k)[0] for k in STEP_STAGES}
        assert first[STAGE] == 0
        if ask:
            with profiled(ctx):
                assert syn.line_tangent(strength=1.0, doppler=0.1).numpy().any()
                ctx.synchronize()
                assert ctx.profile(STAGE)[0] == 1 and all(ctx.profile(k)[0] == 0 for k in STEP_STAGES if k != STAGE)
        with profiled(ctx):
            syn.step()
            ctx.synchronize()
            counts.append((first, {k: ctx.profile(k)[0] for k in STEP_STAGES}))
        outputs.append((np.array(syn.F_nu()), np.array(syn.total_alphas()), np.array(syn.response_opacity.numpy())))
        syn.close()
    print("launches per stage of a step:", counts[0][0])
    assert counts[0][0] == counts[0][1] == counts[1][0] == counts[1][1] and sum(counts[0][0].values()) > 0
    assert all(np.array_equal(a, b) for a, b in zip(*outputs))
