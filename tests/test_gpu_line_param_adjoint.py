"""Line-profile sensitivities on the device (sdx_line_param_adjoint_dev, sdx_line_param_adjoint_f64, ops.line_param_adjoint,
SpectralSynthesizer.line_sensitivities(wrt=...), microturbulence_sensitivity).  It mirrors tests/test_gpu_line_adjoint.py.

The kernels are judged by the restatement of tests/line_param_truth.py (tests/test_line_param_truth_cpu.py checks what that rests on): per
(line, depth) item and per line, for each of the three outputs, |got - ref| <= (OPACITY_RTOL + n_terms 2^-53) scale with the project's
per-term parity OPACITY_RTOL = 1e-12, n_terms the window's overlap with the shard and the scales built from absolute pieces (damping:
sum |W| amp y |w'|; doppler: sum |W| amp (|K| + |x| |w'| + y |w'|); centre: sum |W| amp |w'| / doppler).  Every test prints its figures
before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import line_param_truth as T
import oracle
from stardis_amd import _lib, linelist as LL, ops, synth
from test_gpu_observe_adjoint import engine_instrument
from test_gpu_response import FLUX_PARITY, H, fixed_window_lines, model, profiled, synthesizer  # noqa: F401  (`model`: the module-scoped fixture)

pytestmark = pytest.mark.gpu

A = T.A
NAMES = ["small", "ragged", "tiny", "odd", "long", "inner"]
KEYS = ("damping", "doppler", "centre")
STAGE = "k_line_param_adjoint"
TABLES = ("line_nus", "doppler_widths", "gammas", "alphas")


@functools.lru_cache(maxsize=None)
def restated(name, shard=None):
    return T.restated(name, shard=shard)


def param_adjoint(ctx, m, W=None, shard=None, lines=None, want=KEYS, depth=True, line=True):
    """sdx_line_param_adjoint_dev on the model's grid -> dict key -> (per line, per depth) host arrays (None where not asked for)"""
    L = m.lines if lines is None else lines
    b, n = (0, m.n_nu) if shard is None else shard
    W = m.W if W is None else W
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], W[:, b:b + n])]
    nl = L["line_nus"].size
    o_l = {k: ctx.zeros((nl,)) if (line and k in want) else None for k in KEYS}
    o_ld = {k: ctx.zeros((nl, m.n_depth)) if (depth and k in want) else None for k in KEYS}
    ctx.call("sdx_line_param_adjoint_dev", m.n_depth, m.n_nu, d[0].ptr, b, n, nl, d[1].ptr, d[2].ptr, d[3].ptr, L["gammas"].shape[1], d[4].ptr, d[5].ptr, n,
             *[_lib.ptr_of(o_l[k]) for k in KEYS], *[_lib.ptr_of(o_ld[k]) for k in KEYS])
    ctx.synchronize()
    return {k: (None if o_l[k] is None else np.array(o_l[k].numpy()), None if o_ld[k] is None else np.array(o_ld[k].numpy())) for k in KEYS}


def judge(label, got, r):
    worst = {}
    for k in KEYS:
        q = getattr(r, k)
        got_l, got_ld = got[k]
        ratio_ld = np.abs(got_ld - q.s_ld) / np.where(q.scale_ld > 0, T.bound(q.scale_ld, q.terms_ld), 1.0)
        ratio_l = np.abs(got_l - q.s_l) / np.where(q.scale_l > 0, T.bound(q.scale_l, q.terms_l), 1.0)
        worst[k] = (float(ratio_ld.max()), float(ratio_l.max()))
        print(f"{label}, {k}: worst |got - ref| / bound per item {ratio_ld.max():.3e}, per line {ratio_l.max():.3e}")
    for k in KEYS:
        q = getattr(r, k)
        got_l, got_ld = got[k]
        assert np.isfinite(got_l).all() and np.isfinite(got_ld).all()
        assert np.array_equal(got_ld[q.scale_ld == 0], np.zeros(int((q.scale_ld == 0).sum())))  # no term in the shard: exactly 0
        assert worst[k][0] <= 1.0 and worst[k][1] <= 1.0, (label, k, worst)


def same(a, b):
    return all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) for k in KEYS)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(ctx, name):
    m = T.model(name)
    got = param_adjoint(ctx, m)
    judge(name, got, restated(name))
    # the array-level function and the host-buffer twin: the same bits
    per_line = ops.line_param_adjoint(*A.line_args(m), m.W, ctx=ctx)
    per_depth = ops.line_param_adjoint(*A.line_args(m), ctx.upload(m.W), per_depth=True, ctx=ctx, device=True)
    assert set(per_line) == set(per_depth) == set(KEYS)
    L = m.lines
    host_l, host_ld = {k: np.zeros(m.n_lines) for k in KEYS}, {k: np.zeros((m.n_lines, m.n_depth)) for k in KEYS}
    _lib.check(ctx.lib.sdx_line_param_adjoint_f64(ctx.handle, m.n_depth, m.n_nu, m.nus.ctypes.data, m.n_lines, L["line_nus"].ctypes.data,
                                                  L["doppler_widths"].ctypes.data, L["gammas"].ctypes.data, L["gammas"].shape[1], L["alphas"].ctypes.data,
                                                  m.W.ctypes.data, *[host_l[k].ctypes.data for k in KEYS], *[host_ld[k].ctypes.data for k in KEYS]))
    for k in KEYS:
        assert np.array_equal(per_line[k], got[k][0]) and np.array_equal(per_depth[k].numpy(), got[k][1])
        assert np.array_equal(host_l[k], got[k][0]) and np.array_equal(host_ld[k], got[k][1])
    only = ops.line_param_adjoint(*A.line_args(m), m.W, ctx=ctx, wrt=("centre",))
    assert list(only) == ["centre"] and np.array_equal(only["centre"], got["centre"][0])


@pytest.mark.parametrize("name", ["long", "inner"])
def test_supertiles(ctx, name):
    """the tiled role with fewer groups of partial sums than (item, tile) pairs ("adjoint_partials" counts doubles, a group is four): one
    supertile of all tiles, two, three, and every tile a supertile of its own"""
    m = T.model(name)
    r = restated(name)
    results = []
    try:
        for partials in (1, 100, 160, 1 << 22):
            ctx.set_option("adjoint_partials", partials)
            got = param_adjoint(ctx, m)
            judge(f"{name}, adjoint_partials = {partials}", got, r)
            assert same(param_adjoint(ctx, m), got)
            results.append(got)
    finally:
        ctx.set_option("adjoint_partials", 1 << 22)
    assert any(not same(results[0], other) for other in results[1:])  # (the order of the sums did change)


@pytest.mark.parametrize("name,shard", [("long", (1500, 6000)), ("inner", (3000, 6000)), ("inner", (5000, 7001))])
def test_tiled_items_in_a_shard(ctx, name, shard):
    m = T.model(name)
    r = restated(name, shard)
    assert (r.damping.terms_ld > 4096).any()
    try:
        for partials in (1 << 22, 100):
            ctx.set_option("adjoint_partials", partials)
            judge(f"{name}, shard {shard}, adjoint_partials = {partials}", param_adjoint(ctx, m, shard=shard), r)
    finally:
        ctx.set_option("adjoint_partials", 1 << 22)


# ---- 2. shards ---------------------------------------------------------------------------------------------------------------------
def test_shards(ctx):
    m = T.model("small")
    whole = param_adjoint(ctx, m)
    parts = {}
    for shard in ((0, 100), (100, 120), (220, 80)):
        parts[shard] = param_adjoint(ctx, m, shard=shard)
        judge(f"shard {shard}", parts[shard], restated("small", shard))
        via_ops = ops.line_param_adjoint(*A.line_args(m), np.ascontiguousarray(m.W[:, shard[0]:shard[0] + shard[1]]), ctx=ctx, shard=shard)
        assert all(np.array_equal(via_ops[k], parts[shard][k][0]) for k in KEYS)
    # (0, n) is the whole grid
    assert same(param_adjoint(ctx, m, shard=(0, m.n_nu)), whole)
    lo, hi = A.windows("small")
    floor = A.regimes("small")[0]
    outside = [l for l in floor if (hi[l] <= 100).all() or (lo[l] >= 220).all()]
    assert outside
    for k in KEYS:
        assert all(parts[(100, 120)][k][0][l] == 0.0 and not parts[(100, 120)][k][1][l].any() for l in outside)
    r = restated("small")
    for k in KEYS:
        q = getattr(r, k)
        sum_l, sum_ld = sum(p[k][0] for p in parts.values()), sum(p[k][1] for p in parts.values())
        ratio = max(float((np.abs(sum_ld - whole[k][1]) / T.bound(q.scale_ld, q.terms_ld)).max()), float((np.abs(sum_l - whole[k][0]) / T.bound(q.scale_l, q.terms_l)).max()))
        print(f"{k}: a head, a middle and a tail shard against the whole grid: worst difference / bound {ratio:.3e}")
        assert ratio <= 1.0


# ---- 3. order, duplicates, outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_order_duplicates_and_outputs(ctx, name):
    m = T.model(name)
    got = param_adjoint(ctx, m)
    order = np.random.default_rng(4).permutation(m.n_lines)
    order = np.concatenate([order, order[:3]])  # a shuffled list with duplicates
    mixed = {k: np.ascontiguousarray(v[order]) for k, v in m.lines.items()}
    r = param_adjoint(ctx, m, lines=mixed)
    for k in KEYS:
        assert np.array_equal(r[k][0], got[k][0][order]) and np.array_equal(r[k][1], got[k][1][order])
    # outputs requested singly and all together: equal bits
    for k in KEYS:
        one_line = param_adjoint(ctx, m, want=(k,), depth=False)
        one_depth = param_adjoint(ctx, m, want=(k,), line=False)
        assert np.array_equal(one_line[k][0], got[k][0]) and one_line[k][1] is None
        assert np.array_equal(one_depth[k][1], got[k][1]) and one_depth[k][0] is None
        assert all(one_line[other] == (None, None) for other in KEYS if other != k)


# ---- 4. determinism and capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "long"])
def test_determinism_and_capture(ctx, name):
    m = T.model(name)
    first, again = param_adjoint(ctx, m), param_adjoint(ctx, m)
    assert same(first, again)
    L = m.lines
    d = [ctx.upload(a) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], m.W)]
    o_l, o_ld = [ctx.zeros((m.n_lines,)) for _ in KEYS], [ctx.zeros((m.n_lines, m.n_depth)) for _ in KEYS]
    ctx.call("sdx_graph_begin")
    try:
        ctx.call("sdx_line_param_adjoint_dev", m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, L["gammas"].shape[1], d[4].ptr,
                 d[5].ptr, m.n_nu, *[o.ptr for o in o_l], *[o.ptr for o in o_ld])
    finally:
        graph = C.c_void_p()
        _lib.check(ctx.lib.sdx_graph_end(ctx.handle, C.byref(graph)))
    ctx.synchronize()
    assert not any(o.numpy().any() for o in o_l + o_ld)  # recorded, not run
    for _ in range(2):
        for o in o_l + o_ld:
            o.zero()
        ctx.call("sdx_graph_launch", graph)
        ctx.synchronize()
        for j, k in enumerate(KEYS):
            assert np.array_equal(o_l[j].numpy(), first[k][0]) and np.array_equal(o_ld[j].numpy(), first[k][1])
    ctx.call("sdx_graph_destroy", graph)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    m = T.model("odd")
    L = m.lines
    d = [ctx.upload(a) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], m.W)]
    o_l, o_ld = [ctx.zeros((m.n_lines,)) for _ in KEYS], [ctx.zeros((m.n_lines, m.n_depth)) for _ in KEYS]
    outs = [o.ptr for o in o_l + o_ld]

    def call(n_nu=m.n_nu, begin=0, count=None, gamma_cols=m.n_depth, out=outs, n_lines=m.n_lines, n_depth=m.n_depth):
        count = n_nu if count is None else count
        ctx.call("sdx_line_param_adjoint_dev", n_depth, n_nu, d[0].ptr, begin, count, n_lines, d[1].ptr, d[2].ptr, d[3].ptr, gamma_cols, d[4].ptr, d[5].ptr,
                 m.n_nu, *out)

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
                call(n_nu=n_nu, out=[None] * 6)
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
            call(n_depth=0, gamma_cols=0)
        assert ctx.lib.sdx_line_param_adjoint_dev(None, m.n_depth, m.n_nu, d[0].ptr, 0, m.n_nu, m.n_lines, d[1].ptr, d[2].ptr, d[3].ptr, m.n_depth, d[4].ptr,
                                                  d[5].ptr, m.n_nu, *outs) == -1
        call(n_lines=0)  # trivial calls: nothing is launched
        call(begin=5, count=0)
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 0 and ctx.profile("k_line_adjoint")[0] == 0 and not any(o.numpy().any() for o in o_l + o_ld)
        call()  # and the context still serves
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 1 and ctx.profile("k_line_adjoint")[0] == 0
    got = {k: (np.array(o_l[j].numpy()), np.array(o_ld[j].numpy())) for j, k in enumerate(KEYS)}
    judge("after the refusals", got, restated("odd"))


# ---- 6. the engine: identity with what exists --------------------------------------------------------------------------------------
def test_engine_identity(ctx, model):
    m = model
    n_depth, n_nu, n_lines = 12, 300, 40
    w = np.random.default_rng(1).standard_normal(n_nu)
    syn = synthesizer(ctx, m, keep_response=True)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert ctx.profile("k_line_adjoint")[0] == 0 and ctx.profile(STAGE)[0] == 0  # on demand: the step launches what it launched
        damping = syn.line_sensitivities(w, wrt="damping")
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 1 and ctx.profile("k_line_adjoint")[0] == 0 and ctx.profile("k_response_weight")[0] == 1
        everything = syn.line_sensitivities(w, wrt=("strength", "damping", "doppler", "centre"))
        ctx.synchronize()
        assert ctx.profile(STAGE)[0] == 2 and ctx.profile("k_line_adjoint")[0] == 1  # a tuple: one pass for the three shape parameters
    assert damping.shape == (n_lines,) and isinstance(everything, dict) and list(everything) == ["strength", "damping", "doppler", "centre"]
    # wrt="strength" is the existing call, bit for bit; a tuple's entries are the single calls
    plain = np.array(syn.line_sensitivities(w).numpy())
    assert np.array_equal(syn.line_sensitivities(w, wrt="strength").numpy(), plain) and np.array_equal(everything["strength"].numpy(), plain)
    single = {k: np.array(syn.line_sensitivities(w, wrt=k).numpy()) for k in KEYS}
    assert np.array_equal(single["damping"], damping.numpy())
    for k in KEYS:
        assert np.array_equal(everything[k].numpy(), single[k]) and np.isfinite(single[k]).all() and single[k].any()
    pair = syn.line_sensitivities(w, per_depth=True, wrt=("centre", "doppler"))
    assert list(pair) == ["centre", "doppler"] and pair["centre"].shape == (n_lines, n_depth)
    for k in ("centre", "doppler"):
        assert np.array_equal(pair[k].numpy(), syn.line_sensitivities(w, per_depth=True, wrt=k).numpy())
    # the weight plane and the direct entry point: what the method launches
    Ra, total = np.array(syn.response_opacity.numpy()), np.array(syn.total_alphas())
    W = w[None, :] * (Ra / total)
    direct = ops.line_param_adjoint(n_depth, m.nus, *[m.lines[k] for k in TABLES], W, ctx=ctx)
    assert all(np.array_equal(direct[k], single[k]) for k in KEYS)
    # an unsorted list: the answers come in the caller's order
    shuffle = np.random.default_rng(3).permutation(n_lines)
    mixed = synthesizer(ctx, m, {k: np.ascontiguousarray(v[shuffle]) for k, v in m.lines.items()}, keep_response=True)
    mixed.step()
    ctx.synchronize()
    for k in KEYS:
        assert np.array_equal(mixed.line_sensitivities(w, wrt=k).numpy(), single[k][shuffle])
    mixed.close()
    syn.close()
    # a frequency shard: the partial sum over its own columns, what ops.line_param_adjoint gives on the shard
    part = synthesizer(ctx, m, keep_response=True, shard=(100, 120))
    part.step()
    ctx.synchronize()
    got = part.line_sensitivities(w[100:220], wrt=KEYS)
    expect = ops.line_param_adjoint(n_depth, m.nus, *[m.lines[k] for k in TABLES], np.ascontiguousarray(W[:, 100:220]), ctx=ctx, shard=(100, 120))
    for k in KEYS:
        g = np.array(got[k].numpy())
        assert np.array_equal(g, expect[k]) and g.any() and not np.array_equal(g, single[k])
    part.close()
    plain_syn = synthesizer(ctx, m)
    with pytest.raises(RuntimeError, match="keep_response=True"):
        plain_syn.line_sensitivities(wrt="doppler")
    plain_syn.close()


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
        per_line, per_depth = syn.line_sensitivities(w, wrt=KEYS), syn.line_sensitivities(w, per_depth=True, wrt=KEYS)
        out.append(({k: np.array(v.numpy()) for k, v in per_line.items()}, {k: np.array(v.numpy()) for k, v in per_depth.items()}, syn.microturbulence_sensitivity(1.2e5, w)))
        syn.close()
    for k in KEYS:
        assert out[0][0][k].shape == (30,) and np.isfinite(out[0][0][k]).all() and out[0][0][k].any()
        assert np.array_equal(out[0][0][k], out[1][0][k]) and np.array_equal(out[0][1][k], out[1][1][k])
    assert out[0][2] == out[1][2] and out[0][2] != 0.0


def test_engine_chi2_gradient(ctx, model):
    """chi2_line_gradient(..., wrt="damping") is observed_line_sensitivities(c, wrt="damping") with c = -2 ivar r"""
    m = model
    inst = engine_instrument(ctx, v=-8.0)
    syn = synthesizer(ctx, m, keep_response=True, instrument=inst)
    syn.step()
    ctx.synchronize()
    rng = np.random.default_rng(8)
    obs = np.array(syn.observed.numpy())
    data = np.where(np.isnan(obs), 1.0, obs) * (1.0 + 0.01 * rng.standard_normal(obs.size))
    ivar = rng.uniform(0.5, 2.0, obs.size) / np.nanmax(np.abs(obs)) ** 2
    use = ~np.isnan(obs) & (ivar != 0)
    r = np.where(use, data, 0.0) - np.where(use, obs, 0.0)
    c = -2.0 * np.where(use, ivar, 0.0) * r
    chi2, grad = syn.chi2_line_gradient(data, ivar, wrt="damping")
    assert chi2 == syn.chi2_line_gradient(data, ivar)[0]
    expect = np.array(syn.observed_line_sensitivities(c, wrt="damping").numpy())
    assert np.array_equal(grad.numpy(), expect) and expect.any()
    assert np.array_equal(expect, syn.line_sensitivities(syn.pixel_weights_to_grid(c), wrt="damping").numpy())
    both = syn.chi2_line_gradient(data, ivar, per_depth=True, wrt=("strength", "centre"))[1]
    assert list(both) == ["strength", "centre"] and both["centre"].shape == (40, 12)
    assert np.array_equal(both["strength"].numpy(), syn.chi2_line_gradient(data, ivar, per_depth=True)[1].numpy())
    syn.close()


# ---- 7. the engine: against difference quotients, end to end -----------------------------------------------------------------------
AMU, K_B, C_LIGHT = 1.6605390666e-24, 1.380649e-16, 29979245800.0  # sdx_math.h
H_NU = 2.0e6  # Hz: the step of the rest frequencies, a thousandth of the grid's spacing


def perturbed(lines, rows, key, h):
    """the line tables with ln gamma, ln doppler_width (+ h) or the rest frequency (+ h Hz) of `rows` moved"""
    out = {k: v.copy() for k, v in lines.items()}
    if key == "damping":
        out["gammas"][rows] *= np.exp(h)
    elif key == "doppler":
        out["doppler_widths"][rows] *= np.exp(h)
    else:
        out["line_nus"][rows] += h
    return out


def assert_windows_hold(nus, base, moved, rows):
    """every line of `rows` keeps its window at every depth (oracle.window on both tables)"""
    for l in rows:
        for d in range(base["alphas"].shape[1]):
            args = [(t["line_nus"][l], t["gammas"][l, d if t["gammas"].shape[1] > 1 else 0], t["doppler_widths"][l, d], t["alphas"][l, d]) for t in (base, moved)]
            assert oracle.window(nus, *args[0]) == oracle.window(nus, *args[1]), (l, d)


def flux_of(ctx, m, lines):
    syn = synthesizer(ctx, m, lines)
    syn.step()
    ctx.synchronize()
    F = np.array(syn.F_nu()[-1])
    syn.close()
    return F


def richardson(flux, h):
    """-> (coarse, fine) central difference quotients from the fluxes at +-h and +-h/2"""
    return (flux[h] - flux[-h]) / (2 * h), (flux[h / 2] - flux[-h / 2]) / h


def held_against_quotients(label, value_of, coarse, fine, F_last, h):
    """the pattern of test_gpu_line_adjoint.test_engine_against_difference_quotients: the 20 columns with the largest quotients, unit
    weights on them; allowance = |coarse - fine| + FLUX_PARITY max|F| / h per column"""
    extrapolated = (4 * fine - coarse) / 3
    columns = np.argsort(np.abs(extrapolated))[-20:]
    w = np.zeros(F_last.size)
    w[columns] = 1.0
    value = value_of(w)
    target = float(extrapolated[columns].sum())
    allowance = float((np.abs(coarse - fine)[columns] + FLUX_PARITY * np.abs(F_last).max() / h).sum())
    print(f"{label}: value {value:+.6e}, difference quotients {target:+.6e}, |difference| {abs(value - target):.3e}, allowance {allowance:.3e}, "
          f"|value| / allowance {abs(value) / allowance:.1f}")
    return abs(value - target) <= allowance, abs(value) > 10 * allowance  # a zero cannot pass


@pytest.mark.parametrize("key", KEYS)
def test_engine_against_difference_quotients(ctx, model, key):
    """ln gamma, ln doppler_width and the rest frequency of the six lines of species X (floor or whole-grid windows: the strongest of the
    lines whose windows do not move) moved together; every one of them keeps its window at every depth under all four perturbations"""
    m = model
    h = H_NU if key == "centre" else H
    flux = {}
    for step in (h, -h, h / 2, -h / 2):
        moved = perturbed(m.lines, m.x_lines, key, step)
        assert_windows_hold(m.nus, m.lines, moved, m.x_lines)
        flux[step] = flux_of(ctx, m, moved)
    coarse, fine = richardson(flux, h)
    syn = synthesizer(ctx, m, keep_response=True)
    syn.step()
    ctx.synchronize()
    F_last = np.array(syn.F_nu()[-1])
    ok, seen = held_against_quotients(f"{key}, the lines of X", lambda w: float(np.array(syn.line_sensitivities(w, wrt=key).numpy())[m.x_lines].sum()), coarse, fine, F_last, h)
    syn.close()
    assert ok and seen


def test_microturbulence_against_difference_quotients(ctx, model):
    """The fixed-window lines of the model with a Doppler table rebuilt from doppler_width = nu / c sqrt(2 k T / m + xi^2) (sdx_broadening.h;
    masses of H, He, C, Mg and Fe dealt to the lines) at xi, xi +- h, xi +- h / 2: every line keeps its window at every depth under all
    four, and microturbulence_sensitivity(xi) is the Richardson value of the quotients.  xi = 0 returns exactly 0."""
    m = model
    mass = np.random.default_rng(12).choice([1.008, 4.0026, 12.011, 24.305, 55.845], m.lines["line_nus"].size) * AMU
    temps = np.asarray(m.atm["temperatures"], dtype=np.float64).reshape(-1)
    xi, h = 1.5e5, 150.0  # cm/s

    def table(v, rows=slice(None)):
        out = {k: np.ascontiguousarray(a[rows]) for k, a in m.lines.items()}
        out["doppler_widths"] = (out["line_nus"] / C_LIGHT)[:, None] * np.sqrt(2.0 * K_B * temps[None, :] / mass[rows][:, None] + v * v)
        return out

    # the lines of the rebuilt list with floor or whole-grid windows (test_gpu_response.fixed_window_lines: fixed under a factor exp(2 H) on
    # the window's reach, which xi +- h moves by less than exp(h / xi) = exp(H))
    rows = fixed_window_lines(m.nus, table(xi), np.exp(2 * H))
    assert rows.size >= 6
    at_xi = table(xi, rows)
    all_rows = np.arange(rows.size)
    flux = {}
    for step in (h, -h, h / 2, -h / 2):
        moved = table(xi + step, rows)
        assert_windows_hold(m.nus, at_xi, moved, all_rows)
        flux[step] = flux_of(ctx, m, moved)
    coarse, fine = richardson(flux, h)
    syn = synthesizer(ctx, m, at_xi, keep_response=True)
    syn.step()
    ctx.synchronize()
    F_last = np.array(syn.F_nu()[-1])
    assert syn.microturbulence_sensitivity(0.0) == 0.0 and syn.microturbulence_sensitivity(0.0, np.ones(m.nus.size)) == 0.0
    ok, seen = held_against_quotients("microturbulence", lambda w: syn.microturbulence_sensitivity(xi, w), coarse, fine, F_last, h)
    # the projection is the host sum over the per-depth Doppler output
    w = np.random.default_rng(2).standard_normal(m.nus.size)
    per = np.array(syn.line_sensitivities(w, per_depth=True, wrt="doppler").numpy())
    expect = float(np.sum(per * (xi * (at_xi["line_nus"] / C_LIGHT)[:, None] ** 2 / at_xi["doppler_widths"] ** 2)))
    got = syn.microturbulence_sensitivity(xi, w)
    assert isinstance(got, float) and abs(got - expect) <= 1e-14 * float(np.sum(np.abs(per) * xi * (at_xi["line_nus"] / C_LIGHT)[:, None] ** 2 / at_xi["doppler_widths"] ** 2))
    syn.close()
    assert ok and seen
