"""Per-line flux sensitivities on the device (sdx_line_adjoint_dev, sdx_response_weight_dev, ops.line_adjoint,
SpectralSynthesizer.line_sensitivities).

The kernels are judged by the reference's own terms (tests/line_adjoint_truth.py; tests/test_line_adjoint_cpu.py checks what that rests
on): per (line, depth) item |got - ref| <= (OPACITY_RTOL + n_terms 2^-53) sum |W| term, with the project's per-term line-opacity parity
OPACITY_RTOL = 1e-12 and n_terms the item's window length; per line the same with the line's total of terms and the scale summed over
depth.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import line_adjoint_truth as A
from stardis_amd import _lib, linelist as LL, ops, synth
from test_gpu_response import FLUX_PARITY, H, model, profiled, small_model, synthesizer, thicken  # noqa: F401  (`model`: the module-scoped fixture)

pytestmark = pytest.mark.gpu

NAMES = ["small", "ragged", "tiny", "odd", "long", "inner"]


def adjoint(ctx, m, W=None, shard=None, lines=None, want="both"):
    """sdx_line_adjoint_dev on the model's grid -> (out_line, out_line_depth) as host arrays (None for the one not asked for)"""
    L = m.lines if lines is None else lines
    b, n = (0, m.n_nu) if shard is None else shard
    W = m.W if W is None else W
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], W[:, b:b + n])]
    nl = L["line_nus"].size
    o_l = ctx.zeros((nl,)) if want in ("both", "line") else None
    o_ld = ctx.zeros((nl, m.n_depth)) if want in ("both", "depth") else None
    ctx.call("sdx_line_adjoint_dev", m.n_depth, m.n_nu, d[0].ptr, b, n, nl, d[1].ptr, d[2].ptr, d[3].ptr, L["gammas"].shape[1], d[4].ptr, d[5].ptr, n,
             _lib.ptr_of(o_l), _lib.ptr_of(o_ld))
    ctx.synchronize()
    return (None if o_l is None else np.array(o_l.numpy())), (None if o_ld is None else np.array(o_ld.numpy()))


def judge(label, got_l, got_ld, r, factor=1.0):
    ratio_ld = np.abs(got_ld - r.s_ld) / np.where(r.scale_ld > 0, A.bound(r.scale_ld, r.terms_ld, factor), 1.0)
    ratio_l = np.abs(got_l - r.s_l) / np.where(r.scale_l > 0, A.bound(r.scale_l, r.terms_l, factor), 1.0)
    print(f"{label}: worst |got - ref| / bound per item {ratio_ld.max():.3e}, per line {ratio_l.max():.3e}")
    assert np.isfinite(got_l).all() and np.isfinite(got_ld).all()
    assert np.array_equal(got_ld[r.scale_ld == 0], np.zeros(int((r.scale_ld == 0).sum())))  # no term in the shard: exactly 0
    assert (ratio_ld <= 1.0).all() and (ratio_l <= 1.0).all()


# ---- 1. against the reference's terms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_the_references_terms(ctx, name):
    m = A.model(name)
    got_l, got_ld = adjoint(ctx, m)
    judge(name, got_l, got_ld, A.restated(name))
    # the array-level function and the host-buffer twin: the same bits
    assert np.array_equal(ops.line_adjoint(*A.line_args(m), m.W, ctx=ctx), got_l)
    assert np.array_equal(ops.line_adjoint(*A.line_args(m), ctx.upload(m.W), per_depth=True, ctx=ctx, device=True).numpy(), got_ld)
    L = m.lines
    o_l, o_ld = np.zeros(m.n_lines), np.zeros((m.n_lines, m.n_depth))
    _lib.check(ctx.lib.sdx_line_adjoint_f64(ctx.handle, m.n_depth, m.n_nu, m.nus.ctypes.data, m.n_lines, L["line_nus"].ctypes.data,
                                            L["doppler_widths"].ctypes.data, L["gammas"].ctypes.data, L["gammas"].shape[1], L["alphas"].ctypes.data,
                                            m.W.ctypes.data, o_l.ctypes.data, o_ld.ctypes.data))
    assert np.array_equal(o_l, got_l) and np.array_equal(o_ld, got_ld)


@pytest.mark.parametrize("name", ["long", "inner"])
def test_supertiles(ctx, name):
    """the tiled role with fewer partial sums than (item, tile) pairs: several tiles per supertile, added by the wave that owns them
    (context option "adjoint_partials"; at its default every tile of these grids is a supertile of its own).  `inner`: windows that
    start in the middle of a tile and of a supertile and end before the grid does."""
    m = A.model(name)
    r = A.restated(name)
    results = []
    try:
        for partials in (1, 25, 40, 1 << 22):  # `long`: one supertile of nine tiles; two of five and four; three of three; nine of one
            ctx.set_option("adjoint_partials", partials)
            got = adjoint(ctx, m)
            judge(f"{name}, adjoint_partials = {partials}", *got, r)
            assert np.array_equal(adjoint(ctx, m)[1], got[1])
            results.append(got[1])
    finally:
        ctx.set_option("adjoint_partials", 1 << 22)
    assert any(not np.array_equal(results[0], other) for other in results[1:])  # (the order of the sums did change)


@pytest.mark.parametrize("name,shard", [("long", (1500, 6000)), ("inner", (3000, 6000)), ("inner", (5000, 7001))])
def test_tiled_items_in_a_shard(ctx, name, shard):
    """windows of more than 4096 points inside a shard that does not begin at column 0: tiles counted from the shard's first column,
    windows that begin behind the first tile and supertile"""
    m = A.model(name)
    r = A.restated(name, shard=shard)
    assert (r.terms_ld > 4096).any()
    try:
        for partials in (1 << 22, 25):
            ctx.set_option("adjoint_partials", partials)
            judge(f"{name}, shard {shard}, adjoint_partials = {partials}", *adjoint(ctx, m, shard=shard), r)
    finally:
        ctx.set_option("adjoint_partials", 1 << 22)


# ---- 2. the windows are exact ------------------------------------------------------------------------------------------------------
def test_windows_are_exact(ctx):
    m = A.model("small")
    lo, hi = ops.line_windows(*A.line_args(m), ctx=ctx)
    assert np.array_equal(lo, A.windows("small")[0]) and np.array_equal(hi, A.windows("small")[1])
    inner = np.flatnonzero(((hi - lo) == 20).all(axis=1) & (lo >= 1).all(axis=1) & (hi <= m.n_nu - 1).all(axis=1))
    assert inner.size
    l = int(inner[0])
    one = {k: np.ascontiguousarray(v[l:l + 1]) for k, v in m.lines.items()}
    clean = adjoint(ctx, m, lines=one)[1][0]
    for d in range(m.n_depth):
        W = m.W.copy()
        W[d, lo[l, d] - 1] = W[d, hi[l, d]] = np.nan
        assert np.array_equal(adjoint(ctx, m, W=W, lines=one)[1][0], clean)  # just outside: not read
        for col in (lo[l, d], hi[l, d] - 1):
            W = m.W.copy()
            W[d, col] = np.nan
            got = adjoint(ctx, m, W=W, lines=one)[1][0]
            assert np.isnan(got[d]) and np.array_equal(np.delete(got, d), np.delete(clean, d))


# ---- 3. order, duplicates, outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_order_duplicates_and_outputs(ctx, name):
    m = A.model(name)
    got_l, got_ld = adjoint(ctx, m)
    back = {k: np.ascontiguousarray(v[::-1]) for k, v in m.lines.items()}
    r_l, r_ld = adjoint(ctx, m, lines=back)
    assert np.array_equal(r_l[::-1], got_l) and np.array_equal(r_ld[::-1], got_ld)
    k = m.n_lines // 2
    twice = {key: np.ascontiguousarray(np.concatenate([v, v[k:k + 1]])) for key, v in m.lines.items()}
    t_l, t_ld = adjoint(ctx, m, lines=twice)
    assert np.array_equal(t_l[:-1], got_l) and np.array_equal(t_ld[:-1], got_ld) and t_l[-1] == t_l[k] and np.array_equal(t_ld[-1], t_ld[k])
    assert np.array_equal(adjoint(ctx, m, want="line")[0], got_l)
    assert np.array_equal(adjoint(ctx, m, want="depth")[1], got_ld)


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------
def test_shards(ctx):
    m = A.model("small")
    whole_l, whole_ld = adjoint(ctx, m)
    parts = {}
    for shard in ((0, 100), (100, 120), (220, 80)):
        parts[shard] = adjoint(ctx, m, shard=shard)
        r = A.restated("small", shard=shard)
        judge(f"shard {shard}", *parts[shard], r)
        assert np.array_equal(ops.line_adjoint(*A.line_args(m), np.ascontiguousarray(m.W[:, shard[0]:shard[0] + shard[1]]), ctx=ctx, shard=shard),
                              parts[shard][0])
    # a floor-window line whose window misses the shard: exactly 0
    lo, hi = A.windows("small")
    floor = A.regimes("small")[0]
    outside = [l for l in floor if (hi[l] <= 100).all() or (lo[l] >= 220).all()]
    assert outside
    assert all(parts[(100, 120)][0][l] == 0.0 and not parts[(100, 120)][1][l].any() for l in outside)
    # the partials add to the whole within the bound of the whole
    r = A.restated("small")
    sum_l, sum_ld = sum(p[0] for p in parts.values()), sum(p[1] for p in parts.values())
    ratio = max(float((np.abs(sum_ld - whole_ld) / A.bound(r.scale_ld, r.terms_ld)).max()), float((np.abs(sum_l - whole_l) / A.bound(r.scale_l, r.terms_l)).max()))
    print(f"three shards against the whole grid: worst difference / bound {ratio:.3e}")
    assert ratio <= 1.0


# ---- 5. determinism and capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "long"])
def test_determinism_and_capture(ctx, name):
    m = A.model(name)
    first, again = adjoint(ctx, m), adjoint(ctx, m)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    L = m.lines
    d = [ctx.upload(a) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], m.W)]
    o_l, o_ld = ctx.zeros((m.n_lines,)), ctx.zeros((m.n_lines, m.n_depth))
    ctx.call("sdx_graph_begin")
    try:
        ctx.call("sdx_line_adjoint_dev", m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, L["gammas"].shape[1], d[4].ptr,
                 d[5].ptr, m.n_nu, o_l.ptr, o_ld.ptr)
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    ctx.synchronize()
    assert not o_l.numpy().any() and not o_ld.numpy().any()  # recorded, not run
    for _ in range(2):
        o_l.zero()
        o_ld.zero()
        ctx.call("sdx_graph_launch", graph)
        ctx.synchronize()
        assert np.array_equal(o_l.numpy(), first[0]) and np.array_equal(o_ld.numpy(), first[1])
    ctx.call("sdx_graph_destroy", graph)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    m = A.model("odd")
    L = m.lines
    d = [ctx.upload(a) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], m.W)]
    o_l, o_ld = ctx.zeros((m.n_lines,)), ctx.zeros((m.n_lines, m.n_depth))

    def call(n_nu=m.n_nu, begin=0, count=None, gamma_cols=m.n_depth, line=o_l.ptr, depth=o_ld.ptr, n_lines=m.n_lines):
        count = n_nu if count is None else count
        ctx.call("sdx_line_adjoint_dev", m.n_depth, n_nu, d[0].ptr, begin, count, n_lines, d[1].ptr, d[2].ptr, d[3].ptr, gamma_cols, d[4].ptr, d[5].ptr,
                 m.n_nu, line, depth)

    with profiled(ctx):
        ctx.set_option("mixed_precision", 1)
        try:
            for n_nu in (m.n_nu, 0):  # also at set-up time, with an empty grid
                with pytest.raises(ValueError, match="mixed_precision"):
                    call(n_nu=n_nu)
        finally:
            ctx.set_option("mixed_precision", 0)
        for n_nu in (m.n_nu, 0):
            with pytest.raises(ValueError, match="no output"):
                call(n_nu=n_nu, line=None, depth=None)
            with pytest.raises(ValueError, match="gammas"):
                call(n_nu=n_nu, gamma_cols=2)
            with pytest.raises(ValueError, match="shard"):
                call(n_nu=n_nu, begin=1, count=n_nu)
        with pytest.raises(ValueError, match="shard"):
            call(begin=-1, count=5)
        assert ctx.lib.sdx_line_adjoint_dev(None, m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, m.n_depth, d[4].ptr,
                                            d[5].ptr, m.n_nu, o_l.ptr, o_ld.ptr) == -1
        call(n_lines=0)  # trivial calls: nothing is launched
        call(begin=5, count=0)
        ctx.synchronize()
        assert ctx.profile("k_line_adjoint")[0] == 0 and not o_l.numpy().any()
        call()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile("k_line_adjoint")[0] == 1
    r = A.restated("odd")
    judge("after the refusals", np.array(o_l.numpy()), np.array(o_ld.numpy()), r)


# ---- 7. the engine: identity with what exists --------------------------------------------------------------------------------------
def test_engine_identity(ctx, model):
    m = model
    n_depth, n_nu, n_lines = 12, 300, 40
    w = np.random.default_rng(1).standard_normal(n_nu)
    syn = synthesizer(ctx, m, keep_response=True)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile("k_line_adjoint")[0] == 0 and ctx.profile("k_response_weight")[0] == 0  # on demand: the step is the step it was
        sens = syn.line_sensitivities(w)
        ctx.synchronize()
        assert ctx.profile("k_line_adjoint")[0] == 1 and ctx.profile("k_response_weight")[0] == 1
    assert sens.shape == (n_lines,)
    sens = np.array(sens.numpy())
    Ra, total = np.array(syn.response_opacity.numpy()), np.array(syn.total_alphas())
    args = (n_depth, m.nus)
    worst = 0.0
    for l in range(n_lines):
        one = [np.ascontiguousarray(m.lines[k][l:l + 1]) for k in ("line_nus", "doppler_widths", "gammas", "alphas")]
        plane = ops.calc_alan_entries(*args, *one, ctx=ctx)
        expect = float((w * syn.flux_derivative(plane).numpy()).sum())
        allowed = (2 * A.OPACITY_RTOL + n_depth * n_nu * A.EPS) * float(np.abs(w[None, :] * Ra * (plane / total)).sum())
        worst = max(worst, abs(sens[l] - expect) / allowed)
        assert abs(sens[l] - expect) <= allowed, (l, sens[l], expect, allowed)
    print(f"line_sensitivities against flux_derivative of the single-line planes: worst difference / bound {worst:.3e}")
    # per depth: the rows sum to the per-line values
    per_depth = np.array(syn.line_sensitivities(w, per_depth=True).numpy())
    assert per_depth.shape == (n_lines, n_depth)
    scale = np.array([float(np.abs(w[None, :] * Ra * (ops.calc_alan_entries(*args, *[np.ascontiguousarray(m.lines[k][l:l + 1]) for k in
                      ("line_nus", "doppler_widths", "gammas", "alphas")], ctx=ctx) / total)).sum()) for l in range(n_lines)])
    assert (np.abs(per_depth.sum(axis=1) - sens) <= (2 * A.OPACITY_RTOL + n_depth * n_nu * A.EPS) * scale).all()
    # a DeviceArray for the weights: the same bits; no weights: unit weights
    assert np.array_equal(syn.line_sensitivities(ctx.upload(w)).numpy(), sens)
    assert np.array_equal(syn.line_sensitivities().numpy(), syn.line_sensitivities(np.ones(n_nu)).numpy())
    with pytest.raises(ValueError, match="weights"):
        syn.line_sensitivities(np.ones(n_nu - 1))
    # an unsorted list: the answers come in the caller's order
    shuffle = np.random.default_rng(3).permutation(n_lines)
    mixed = synthesizer(ctx, m, {k: np.ascontiguousarray(v[shuffle]) for k, v in m.lines.items()}, keep_response=True)
    mixed.step()
    ctx.synchronize()
    assert np.array_equal(mixed.line_sensitivities(w).numpy(), sens[shuffle])
    mixed.close()
    # the weight plane and the direct entry point: what the method launches
    W = w[None, :] * (Ra / total)
    assert np.array_equal(ops.line_adjoint(n_depth, m.nus, *[m.lines[k] for k in ("line_nus", "doppler_widths", "gammas", "alphas")], W, ctx=ctx), sens)
    syn.close()
    # a frequency shard: the partial sum over its own columns
    part = synthesizer(ctx, m, keep_response=True, shard=(100, 120))
    part.step()
    ctx.synchronize()
    got = np.array(part.line_sensitivities(w[100:220]).numpy())
    expect = ops.line_adjoint(n_depth, m.nus, *[m.lines[k] for k in ("line_nus", "doppler_widths", "gammas", "alphas")], np.ascontiguousarray(W[:, 100:220]),
                              ctx=ctx, shard=(100, 120))
    assert np.array_equal(got, expect) and got.any() and not np.array_equal(got, sens)
    part.close()
    # without keep_response
    plain = synthesizer(ctx, m)
    with pytest.raises(RuntimeError, match="keep_response=True"):
        plain.line_sensitivities()
    plain.close()


def test_engine_line_list_of_scalars(ctx, model):
    """a LineList synthesizer and the dense synthesizer built from LL.line_params of the same list: bit for bit"""
    m = model
    ll = synth.synth_linelist(m.nus, m.atm, 30, seed=7, mix=(0.5, 0.4, 0.1))
    a, g, dw = LL.line_params(ll, ctx=ctx)
    w = np.random.default_rng(1).standard_normal(m.nus.size)
    out = []
    for lines in (ll, dict(line_nus=ll.nu, doppler_widths=dw, gammas=g, alphas=a)):
        syn = synthesizer(ctx, m, lines, keep_response=True)
        syn.step()
        ctx.synchronize()
        out.append((np.array(syn.line_sensitivities(w).numpy()), np.array(syn.line_sensitivities(w, per_depth=True).numpy())))
        syn.close()
    assert out[0][0].shape == (30,) and np.isfinite(out[0][0]).all() and out[0][0].any()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 8. the engine: against difference quotients -----------------------------------------------------------------------------------
def test_engine_against_difference_quotients(ctx, model):
    m = model
    syn = synthesizer(ctx, m, keep_response=True)
    syn.step()
    ctx.synchronize()
    F_last = np.array(syn.F_nu()[-1])
    extrapolated = (4 * m.fine - m.coarse) / 3
    columns = np.argsort(np.abs(extrapolated))[-20:]
    w = np.zeros(m.nus.size)
    w[columns] = 1.0
    value = float(np.array(syn.line_sensitivities(w).numpy())[m.x_lines].sum())
    syn.close()
    target = float(extrapolated[columns].sum())
    allowance = float((np.abs(m.coarse - m.fine)[columns] + FLUX_PARITY * np.abs(F_last).max() / H).sum())
    print(f"sum over the lines of X: {value:.6e}, difference quotients {target:.6e}, |difference| {abs(value - target):.3e}, allowance {allowance:.3e}, "
          f"|value| / allowance {abs(value) / allowance:.1f}")
    assert abs(value - target) <= allowance
    assert abs(value) > 10 * allowance  # a zero cannot pass
