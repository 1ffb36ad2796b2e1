"""The host side of SpectralSynthesizer without a device: the one step call and its options, the intake of a caller's vector, the
chi-square sums and the replay of a stale graph.  The class is built with object.__new__ on a context that records call(name, *args)
and refuses everything it is not expected to be asked."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from stardis_amd import _lib
from stardis_amd.engine import SpectralSynthesizer

NS = types.SimpleNamespace


def dev(ptr, shape=(1,), dtype=np.float64):
    """a stand-in _lib.DeviceArray made without __init__: an address, a shape and a dtype"""
    a = object.__new__(_lib.DeviceArray)
    a.ctx, a.ptr, a.shape, a.dtype = None, ptr, tuple(shape), np.dtype(dtype)
    return a


class NoDevice:
    """a context that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


class Recorder:
    """a context that records call(), upload() and empty() and raises on anything else; sdx_graph_launch raises StaleGraphError
    `stale` times"""

    def __init__(self, stale=0):
        self.calls, self.uploads, self.stale = [], [], stale

    def call(self, name, *args):
        self.calls.append((name, args))
        if name == "sdx_graph_launch" and self.stale:
            self.stale -= 1
            raise _lib.StaleGraphError("stale")

    def upload(self, array, dtype=np.float64):
        self.uploads.append(np.array(array))
        return dev(0xA000 + len(self.uploads), np.shape(array))

    def empty(self, shape, dtype=np.float64):
        return dev(0xE000, shape)

    def __getattr__(self, name):
        raise AssertionError(f"the context was asked for {name}")


def bare(ctx, **kw):
    syn = object.__new__(SpectralSynthesizer)
    syn.ctx = ctx
    syn.graph = syn.graph_classify = syn.graph_batch = syn.plan = None
    for k, v in kw.items():
        setattr(syn, k, v)
    return syn


# ---- the step call -------------------------------------------------------------------------------------------------------------------
PLAN = 0x7000


def stepper(linelist=False, plan=True, continuum=False, two_collective=False, keep_line=True, keep_total=True):
    """a synthesizer of 4 depths, 9 frequencies (the shard 2 .. 8) and 3 lines.  The plan and the evaluation counter are there in every
    configuration: where the step may not pass them it has to leave them out itself"""
    ctx = Recorder()
    struct = _lib.LineListStruct()
    syn = bare(ctx, n_depth=4, n_nu=9, begin=2, count=6, n_lines=3, gamma_cols=4, n_theta=2, cont=_lib.Continuum(), d_nus=dev(0x100), d_t=dev(0x200),
               d_ray=dev(0x300), d_w=dev(0x400), d_ln=dev(0x500), d_dw=dev(0x600), d_g=dev(0x700), d_a=dev(0x800), d_line=dev(0x900),
               d_total=dev(0xA00), d_F=dev(0xB00), _flux_tensor=None, d_evals=dev(0xC00, dtype=np.int64), count_evaluations=True,
               _keep_line=keep_line, _keep_total=keep_total, keep_continuum_flux=continuum, d_Fc=dev(0xD00) if continuum else None,
               m_max=dev(0xE00, (3,)) if two_collective else None, linelist=NS(byref=lambda: C.byref(struct)) if linelist else None,
               keep_contribution=False, keep_response=False, instrument=None)
    syn.plan = C.c_void_p(PLAN) if plan else None
    return syn, ctx, struct


STEP_CASES = [
    ("dense + plan", dict(), dict(grid_plan=PLAN, evals=0xC00)),
    ("dense without plan", dict(plan=False), dict(evals=0xC00)),
    ("dense, planes not kept", dict(keep_line=False, keep_total=False), dict(grid_plan=PLAN, evals=0xC00, line=None, total=None)),
    ("line list", dict(linelist=True), dict(linelist=True, evals=0xC00)),
    ("continuum flux, dense", dict(continuum=True), dict(grid_plan=PLAN, F_nu_continuum=0xD00, continuum_ld=6, evals=0xC00)),
    ("continuum flux, line list", dict(continuum=True, linelist=True), dict(linelist=True, F_nu_continuum=0xD00, continuum_ld=6, evals=0xC00)),
    ("two-collective", dict(two_collective=True), dict(line_m_max=0xE00)),
    ("two-collective, continuum flux", dict(two_collective=True, continuum=True), dict(line_m_max=0xE00, F_nu_continuum=0xD00, continuum_ld=6)),
]


@pytest.mark.parametrize("name,kw,want", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_one_step_call(name, kw, want):
    """Every configuration is exactly one sdx_synthesize_opt_dev call; the options and the arguments that differ are pinned by value: no
    plan with a line list or in the two-collective mode, no evaluation counter in the two-collective mode, no dense pointers with a line
    list."""
    syn, ctx, struct = stepper(**kw)
    syn.enqueue()
    assert [c[0] for c in ctx.calls] == ["sdx_synthesize_opt_dev"]
    args = ctx.calls[0][1]
    assert len(args) == 22
    opt = args[20]._obj
    assert isinstance(opt, _lib.SynthesisOptions)
    want = dict(dict(grid_plan=None, linelist=False, line_m_max=None, F_nu_continuum=None, continuum_ld=0, evals=None, line=0x900, total=0xA00), **want)
    assert opt.grid_plan == want["grid_plan"] and opt.line_m_max == want["line_m_max"]
    assert opt.F_nu_continuum == want["F_nu_continuum"] and opt.continuum_ld == want["continuum_ld"]
    assert bool(opt.linelist) == want["linelist"] and (not want["linelist"] or C.addressof(opt.linelist.contents) == C.addressof(struct))
    # (the options this class never sets)
    assert opt.source is None and opt.I_nus is None and opt.inward_rays == 0 and opt.n_line_planes == 0 and opt.source_ld == 0
    assert args[:6] == (4, 9, 0x100, 2, 6, 3)
    assert args[6:11] == ((None, None, None, 4, None) if want["linelist"] else (0x500, 0x600, 0x700, 4, 0x800))
    assert args[11]._obj is syn.cont and args[12:16] == (2, 0x200, 0x300, 0x400)
    assert args[16:20] == (want["line"], want["total"], 0xB00, 6)
    assert args[21] == want["evals"]


def test_step_call_without_counting():
    syn, ctx, _ = stepper()
    syn.count_evaluations = False
    syn.enqueue()
    assert ctx.calls[0][1][21] is None


def test_fused_and_unfused_share_their_tail():
    """contribution, response and the instrument follow the synthesis on both routes, in that order"""
    syn, ctx, _ = stepper()
    syn.keep_contribution = syn.keep_response = True
    syn.d_C, syn.d_Ra, syn.d_Rs = dev(0x1100), dev(0x1200), dev(0x1300)
    syn.instrument = NS(broadens=False, observe=lambda *a, **k: ctx.calls.append(("observe", a)))
    syn.d_lambdas, syn.d_Flam, syn.d_observed = dev(0x1400), dev(0x1500), dev(0x1600)
    syn.enqueue()
    tail = ["sdx_contribution_dev", "sdx_response_dev", "sdx_flux_nu_to_lambda_dev", "observe"]
    assert [c[0] for c in ctx.calls] == ["sdx_synthesize_opt_dev"] + tail
    del ctx.calls[:]
    syn.enqueue_unfused()
    assert [c[0] for c in ctx.calls] == ["sdx_line_opacity_dev", "sdx_total_alphas_dev", "sdx_raytrace_dev"] + tail


# ---- the intake of a caller's vector ---------------------------------------------------------------------------------------------------
def intake_sites(ctx):
    """name -> (call, number of values or shape, the message's own words, whether a longer device buffer passes)"""
    syn = bare(ctx, n_depth=4, n_nu=5, count=6, n_lines=2, begin=0, keep_response=True, keep_contribution=True, d_Ra=dev(1), d_Rs=dev(2), d_total=dev(3),
               d_C=dev(4), d_nus=dev(5), d_lambdas=dev(6), instrument=NS(n_pix=7), linelist=None, _line_order=None, d_ln=dev(7), d_dw=dev(8), d_g=dev(9),
               d_a=dev(10), gamma_cols=4)
    return {
        "alpha_part": (syn.flux_derivative, (4, 6), None, False),
        "weights": (syn.line_sensitivities, 6, "weights must hold one value per column of the synthesizer (6), got {}", False),
        "c": (lambda v: syn._pixel_vector("c", v), 7, "c must hold one value per pixel of the instrument (7), got {}", False),
        "dF_nu": (lambda v: syn._column_tangent("dF_nu", v), 5, "dF_nu must hold one value per column of the spectrum (5), got {}", True),
        "x": (syn.formation_mean, 4, "x must hold one value per depth point (4), got {}", True),
    }


@pytest.mark.parametrize("name", ["alpha_part", "weights", "c", "dF_nu", "x"])
def test_intake_host_array(name):
    call, want, message, _ = intake_sites(NoDevice())[name]
    if isinstance(want, tuple):  # the exact shape, no reshape
        for bad in (np.zeros((4, 5)), np.zeros((3, 6)), np.zeros(24), np.zeros((6, 4))):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == f"alpha_part must have shape (4, 6), got {bad.shape}"
    else:  # flattened, exactly one value each
        for bad in (np.zeros(want - 1), np.zeros(want + 1), np.zeros((2, want))):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == message.format(bad.size)
    # a right-sized array goes up, as float64 and (a vector) flat, and the call goes on to the context
    ctx = Recorder()
    call = intake_sites(ctx)[name][0]
    good = np.arange(24, dtype=np.float32).reshape(4, 6) if isinstance(want, tuple) else np.arange(want, dtype=np.int64).reshape(1, want)
    call(good)
    assert len(ctx.uploads) == 1 and ctx.uploads[0].dtype == np.float64
    assert np.array_equal(ctx.uploads[0], good if isinstance(want, tuple) else good.reshape(-1))


@pytest.mark.parametrize("name", ["alpha_part", "weights", "c", "dF_nu", "x"])
def test_intake_device_buffer(name):
    call, want, message, longer_passes = intake_sites(NoDevice())[name]
    shape = want if isinstance(want, tuple) else (want,)
    n = int(np.prod(shape))
    with pytest.raises(TypeError) as e:
        call(dev(0x10, shape, np.float32))
    assert str(e.value) == f"{name} must hold float64 values"
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):  # (a tensor that is not on the device)
        call(NS(data_ptr=lambda: 0x10, is_cuda=False, is_contiguous=lambda: True, shape=shape, dtype="torch.float64", numel=lambda: n))
    if isinstance(want, tuple):  # enough values AND the exact shape
        with pytest.raises(ValueError) as e:
            call(dev(0x10, (4, 5)))
        assert str(e.value) == "alpha_part holds 20 values, 24 are needed"
        for bad in ((6, 4), (24,), (4, 7)):
            with pytest.raises(ValueError) as e:
                call(dev(0x10, bad))
            assert str(e.value) == f"alpha_part must have shape (4, 6), got {bad}"
    elif longer_passes:
        with pytest.raises(ValueError) as e:
            call(dev(0x10, (n - 1,)))
        assert str(e.value) == f"{name} holds {n - 1} values, {n} are needed"
    else:
        for size in (n - 1, n + 1):
            with pytest.raises(ValueError) as e:
                call(dev(0x10, (size,)))
            assert str(e.value) == message.format(size)
    # the buffers that pass are used where they are: nothing is uploaded
    for ok in [shape] + ([(n + 3,)] if longer_passes else []):
        ctx = Recorder()
        call = intake_sites(ctx)[name][0]
        buf = dev(0x4440, ok)
        got = call(buf)
        assert not ctx.uploads and (got is buf if name == "c" else any(0x4440 in args for _, args in ctx.calls))


def test_intake_comes_after_the_kept_planes():
    """nothing was kept: that is said first, whatever the vector looks like"""
    sites = intake_sites(NoDevice())
    syn = sites["x"][0].__self__
    syn.keep_response = syn.keep_contribution = False
    with pytest.raises(RuntimeError, match="keep_response=True"):
        syn.flux_derivative(np.zeros(3))
    with pytest.raises(RuntimeError, match="keep_response=True"):
        syn.line_sensitivities(np.zeros(3))
    with pytest.raises(RuntimeError, match="keep_contribution=True"):
        syn.formation_mean(np.zeros(3))


# ---- chi-square ------------------------------------------------------------------------------------------------------------------------
N_PIX = 9
PARAMS = ("v_rad", "lsf", "v_mac")


class Downloads:
    """a device vector that counts its downloads"""

    def __init__(self, host):
        self.host, self.n = host, 0

    def numpy(self):
        self.n += 1
        return self.host.copy()


def chi2_case(seed=2):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(0.5, 1.0, N_PIX)
    obs[8] = np.nan  # a pixel the grid does not cover
    edge = np.zeros(N_PIX, dtype=bool)
    edge[0] = True  # an edge-affected pixel
    ivar = rng.uniform(0.5, 2.0, N_PIX)
    ivar[4] = 0.0
    data = rng.uniform(0.5, 1.0, N_PIX)
    columns = {k: rng.standard_normal(N_PIX) for k in PARAMS}
    for v in columns.values():
        v[8] = np.nan  # (NaN where the observed spectrum is NaN)
    inst = NS(n_pix=N_PIX, broadens=True, edge_affected=lambda lam: edge.copy(), _wrt=lambda wrt: PARAMS if wrt is None else tuple(wrt),
              parameter_tangents=lambda d_lam, n, d_f, reference=None, wrt=None: {k: Downloads(columns[k]) for k in wrt})
    syn = bare(NoDevice(), instrument=inst, keep_response=False, keep_continuum_flux=False, d_observed=Downloads(obs), lambdas=None, d_lambdas=None,
               d_Flam=None, d_Fclam=None, n_nu=20)
    return syn, data, ivar, obs, edge, columns


def restated(names, data, ivar, obs, edge, columns):
    use = ~np.isnan(obs) & (ivar != 0) & ~edge
    r = np.where(use, data, 0.0) - np.where(use, obs, 0.0)
    w = np.where(use, ivar, 0.0)
    c = -2.0 * w * r
    J = {k: np.where(use, columns[k], 0.0) for k in names}
    H = np.empty((len(names), len(names)))
    for ia, a in enumerate(names):
        for ib in range(ia, len(names)):
            H[ia, ib] = H[ib, ia] = 2.0 * math.fsum(w * J[a] * J[names[ib]])
    return float(np.sum(w * r * r)), {k: math.fsum(c * J[k]) for k in names}, H, use


def test_chi2_instrument_gradient_is_the_restatement():
    syn, data, ivar, obs, edge, columns = chi2_case()
    chi2_ref, grad_ref, H_ref, use = restated(PARAMS, data, ivar, obs, edge, columns)
    assert use.tolist() == [False, True, True, True, False, True, True, True, False]
    chi2, grad, H = syn.chi2_instrument_gradient(data, ivar, None, curvature=True)
    assert syn.d_observed.n == 1  # one download of the observed spectrum per call
    assert chi2 == chi2_ref and grad == grad_ref and list(grad) == list(PARAMS)
    assert np.array_equal(H, H_ref) and np.array_equal(H, H.T) and np.all(np.isfinite(H))
    assert syn.chi2_instrument_gradient(data, ivar, ("lsf",)) == (chi2_ref, {"lsf": grad_ref["lsf"]})
    assert syn.d_observed.n == 2


def test_chi2_joint_gradient_without_lines_is_the_instrument_gradient():
    syn, data, ivar, *_ = chi2_case()
    assert syn.keep_response is False  # (and it is not asked for)
    for directions in (None, {}):
        a = syn.chi2_joint_gradient(data, ivar, PARAMS, directions, curvature=True)
        b = syn.chi2_instrument_gradient(data, ivar, PARAMS, curvature=True)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert syn.chi2_joint_gradient(data, ivar, ("v_rad",)) == syn.chi2_instrument_gradient(data, ivar, ("v_rad",))
    with pytest.raises(RuntimeError, match="keep_response=True"):
        syn.chi2_joint_gradient(data, ivar, PARAMS, {"gf": dict(strength=1.0)})


def test_chi2_joint_gradient_with_lines_is_the_restatement():
    syn, data, ivar, obs, edge, columns = chi2_case()
    syn.keep_response = True
    line_columns = {"gf": np.random.default_rng(9).standard_normal(N_PIX), "xi": np.random.default_rng(10).standard_normal(N_PIX)}
    syn.observed_line_jacobian = lambda directions, normalized=False: {k: Downloads(line_columns[k]) for k in directions}
    names = ("lsf", "v_rad", "gf", "xi")
    chi2_ref, grad_ref, H_ref, _ = restated(names, data, ivar, obs, edge, dict(columns, **line_columns))
    chi2, grad, H = syn.chi2_joint_gradient(data, ivar, ("lsf", "v_rad"), {"gf": {}, "xi": {}}, curvature=True)
    assert syn.d_observed.n == 1
    assert chi2 == chi2_ref and grad == grad_ref and list(grad) == list(names) and np.array_equal(H, H_ref)
    chi2, grad = syn.chi2_joint_gradient(data, ivar, (), {"xi": {}})
    assert list(grad) == ["xi"] and grad["xi"] == grad_ref["xi"]
    with pytest.raises(ValueError, match="reuses the instrument's parameter names"):
        syn.chi2_joint_gradient(data, ivar, ("lsf",), {"lsf": {}})


def test_chi2_no_pixel_left():
    syn, data, ivar, *_ = chi2_case()
    message = "no pixel left: every pixel is NaN (not covered by the grid), edge-affected or has inverse_variance 0"
    for call in (lambda: syn.chi2_instrument_gradient(data, np.zeros(N_PIX), None), lambda: syn.chi2_joint_gradient(data, np.zeros(N_PIX), PARAMS),
                 lambda: syn._chi2_pixel_weights(data, np.zeros(N_PIX), False)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message
    with pytest.raises(ValueError) as e:
        syn.chi2_instrument_gradient(data[:-1], ivar, None)
    assert str(e.value) == f"data must hold one value per pixel of the instrument ({N_PIX}), got {N_PIX - 1}"


# ---- replay of a stale graph -----------------------------------------------------------------------------------------------------------
def recorded(stale):
    ctx = Recorder(stale)
    syn = bare(ctx, graph="step", graph_classify="classify", graph_batch="batch", batch=3)
    captures = []

    def capture(**kw):
        captures.append(kw)
        assert (syn.graph, syn.graph_classify, syn.graph_batch, syn.batch) == (None, None, None, 1)  # (destroyed first)
        syn.graph, syn.graph_classify = "step'", "classify'"
        if "batch" in kw:
            syn.graph_batch, syn.batch = "batch'", kw["batch"]
        return syn

    syn.capture = capture
    return syn, ctx, captures


DESTROYED = [("sdx_graph_destroy", (g,)) for g in ("step", "classify", "batch")]


@pytest.mark.parametrize("method,graph,capture_args,result", [("step", "step", {}, None), ("step_classify", "classify", dict(eager_phase2=False), None),
                                                              ("step_batch", "batch", dict(batch=3), 3)])
def test_stale_graph_is_recorded_again(method, graph, capture_args, result):
    syn, ctx, captures = recorded(stale=1)
    assert getattr(syn, method)() == result
    assert captures == [capture_args]
    assert ctx.calls == [("sdx_graph_launch", (graph,))] + DESTROYED + [("sdx_graph_launch", (graph + "'",))]
    # a graph that is not stale is launched and nothing else
    syn, ctx, captures = recorded(stale=0)
    assert getattr(syn, method)() == result
    assert captures == [] and ctx.calls == [("sdx_graph_launch", (graph,))]


def test_stale_twice_is_an_error():
    syn, ctx, captures = recorded(stale=2)
    with pytest.raises(_lib.StaleGraphError):
        syn.step()
    assert len(captures) == 1


def test_steps_without_a_graph():
    ctx = Recorder()
    syn = bare(ctx, batch=1)
    done = []
    syn.enqueue, syn.enqueue_classify = lambda: done.append("enqueue"), lambda: done.append("classify")
    syn.step_classify()
    syn.step()
    assert syn.step_batch() == 1
    assert done == ["classify", "enqueue", "enqueue"] and ctx.calls == []
    syn._destroy_graphs()
    assert ctx.calls == [] and syn.batch == 1
