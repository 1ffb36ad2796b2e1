"""The eight products of the formal solution over the grid's columns, without a device: the exact ctx.call each ops wrapper makes
(name and argument tuple) over its optional planes, outputs and forms of alpha_scatter; the type and text of every refusal the wrappers
make themselves; and what the 17 C entry points answer to a null context.  3 depths, 2 frequencies, 2 angles."""
import ctypes as C

import numpy as np
import pytest

from test_engine_host_cpu import NoDevice, Recorder, dev

from stardis_amd import _lib, ops

ND, NN, NT = 3, 2, 2
NUS = np.array([3.0e14, 2.0e14])
T = np.array([9000.0, 7000.0, 5000.0])
RD = np.array([[1.0, 1.5], [2.0, 2.5]])
W = np.array([0.25, 0.75])
PLANE = np.arange(1.0, 7.0).reshape(ND, NN)
E = 0xE000  # what Recorder.empty() hands out
A, S, B, Z, COT, DIRECT, SC1, SC2, ANGLES = (dev(p, s) for p, s in [(0x51, (ND, NN)), (0x52, (ND, NN)), (0x53, (ND, NN)), (0x54, (ND, NN)),
                                                                   (0x55, (ND, NN)), (0x56, (ND, NN)), (0x57, (ND,)), (0x58, (ND, NN)),
                                                                   (0x59, (NT, NN))])


def up(ctx, array):
    """the address Recorder.upload() gave the one upload that holds `array`"""
    hits = [0xA001 + i for i, u in enumerate(ctx.uploads) if u.shape == np.shape(array) and np.array_equal(u, array)]
    assert len(hits) == 1, (array, ctx.uploads)
    return hits[0]


def one_call(ctx, name):
    assert [c[0] for c in ctx.calls] == [name]
    return ctx.calls[0][1]


def head(ctx, weights=True):
    return (ND, NN, NT, up(ctx, NUS), up(ctx, T), up(ctx, RD)) + ((up(ctx, W),) if weights else ())


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [None, "host"])
@pytest.mark.parametrize("alphas", ["device", "host"])
def test_contribution_call(source, alphas):
    ctx = Recorder()
    out = ops.contribution_arrays(NUS, T, RD, W, A if alphas == "device" else PLANE, ctx=ctx, source=None if source is None else 2.0 * PLANE,
                                  device=True)
    args = one_call(ctx, "sdx_contribution_dev")
    assert args == head(ctx) + (0x51 if alphas == "device" else up(ctx, PLANE), NN, None if source is None else up(ctx, 2.0 * PLANE), NN, E, NN)
    assert out.ptr == E and out.shape == (ND, NN)
    assert len(ctx.uploads) == 4 + (alphas == "host") + (source is not None)


@pytest.mark.parametrize("source", [None, "host"])
@pytest.mark.parametrize("inward", [False, True])
def test_emergent_intensity_call(source, inward):
    ctx = Recorder()
    out = ops.emergent_intensity(NUS, T, RD, A, ctx=ctx, source=None if source is None else 2.0 * PLANE, inward_rays=inward, device=True)
    args = one_call(ctx, "sdx_emergent_intensity_dev")
    assert args == head(ctx, weights=False) + (0x51, NN, None if source is None else up(ctx, 2.0 * PLANE), NN, 1 if inward else 0, E, NN)
    assert out.ptr == E and out.shape == (NT, NN)
    assert len(ctx.uploads) == 3 + (source is not None)


OUTPUT_PAIRS = [(True, True), (False, True), (True, False)]


@pytest.mark.parametrize("source", [None, "host"])
@pytest.mark.parametrize("want_a,want_s", OUTPUT_PAIRS)
def test_response_call(source, want_a, want_s):
    ctx = Recorder()
    out = ops.response(NUS, T, RD, W, A, ctx=ctx, source=None if source is None else 2.0 * PLANE, device=True, want_opacity=want_a,
                       want_source=want_s)
    args = one_call(ctx, "sdx_response_dev")
    assert args == head(ctx) + (0x51, NN, None if source is None else up(ctx, 2.0 * PLANE), NN, E if want_a else None, NN, E if want_s else None, NN)
    assert [o is not None for o in out] == [want_a, want_s]


def test_response_leaves_an_empty_weight_vector_to_the_library():
    """no angle-count check of its own: zero weights with a (N_d - 1, 0) table go to the entry point, which refuses them"""
    ctx = Recorder()
    ops.response(NUS, T, np.zeros((ND - 1, 0)), np.zeros(0), A, ctx=ctx, device=True)
    assert one_call(ctx, "sdx_response_dev")[:3] == (ND, NN, 0)


@pytest.mark.parametrize("cotangent", ["device", "host"])
@pytest.mark.parametrize("source", [None, "host"])
@pytest.mark.parametrize("want_a,want_s", OUTPUT_PAIRS)
def test_response_angles_call(cotangent, source, want_a, want_s):
    ctx = Recorder()
    cot = np.array([[0.5, 0.25], [0.125, 2.0]])
    out = ops.response_angles(NUS, T, RD, ANGLES if cotangent == "device" else cot, A, ctx=ctx, source=None if source is None else 2.0 * PLANE,
                              device=True, want_opacity=want_a, want_source=want_s)
    args = one_call(ctx, "sdx_response_angles_dev")
    assert args == head(ctx, weights=False) + (0x59 if cotangent == "device" else up(ctx, cot), NN, 0x51, NN,
                                               None if source is None else up(ctx, 2.0 * PLANE), NN, E if want_a else None, NN,
                                               E if want_s else None, NN)
    assert [o is not None for o in out] == [want_a, want_s]


@pytest.mark.parametrize("source", [None, "host", "device"])
@pytest.mark.parametrize("want_j,want_l", OUTPUT_PAIRS)
def test_mean_intensity_call(source, want_j, want_l):
    ctx = Recorder()
    out = ops.mean_intensity(NUS, T, RD, W, A, ctx=ctx, source={None: None, "host": 2.0 * PLANE, "device": S}[source], device=True, want_J=want_j,
                             want_L=want_l)
    args = one_call(ctx, "sdx_mean_intensity_dev")
    src = up(ctx, 2.0 * PLANE) if source == "host" else 0x52 if source == "device" else None
    assert args == head(ctx) + (0x51, NN, src, NN, E if want_j else None, NN, E if want_l else None, NN)
    assert [o is not None for o in out] == [want_j, want_l]


@pytest.mark.parametrize("scatter,ld", [(SC1, 0), (SC2, NN), ("host1", 0), ("host2", NN)])
@pytest.mark.parametrize("thermal", [None, "device"])
@pytest.mark.parametrize("want_j", [True, False])
def test_scatter_source_call(scatter, ld, thermal, want_j):
    ctx = Recorder()
    host = {"host1": np.array([0.5, 0.25, 0.125]), "host2": 0.5 * PLANE}.get(scatter) if isinstance(scatter, str) else None
    out = ops.scatter_source(NUS, T, RD, W, A, scatter if host is None else host, ctx=ctx, thermal=None if thermal is None else B, tol=1e-9,
                             max_iter=17, device=True, want_J=want_j)
    args = one_call(ctx, "sdx_scatter_source_dev")
    assert args == head(ctx) + (0x51, NN, scatter.ptr if host is None else up(ctx, host), ld, None if thermal is None else 0x53, NN, 1e-9, 17, E, NN,
                                E if want_j else None, NN, E, E, E)
    assert type(args[-9]) is float and type(args[-8]) is int
    assert (out.J is not None) == want_j and out.S.ptr == E and out.iterations.shape == (NN,) and out.change.shape == (NN,)


@pytest.mark.parametrize("source", [None, "device"])
@pytest.mark.parametrize("want_lt,want_g", OUTPUT_PAIRS)
def test_mean_intensity_adjoint_call(source, want_lt, want_g):
    ctx = Recorder()
    out = ops.mean_intensity_adjoint(NUS, T, RD, W, A, Z, ctx=ctx, source=None if source is None else S, device=True, want_Lt=want_lt, want_G=want_g)
    args = one_call(ctx, "sdx_mean_intensity_adjoint_dev")
    assert args == head(ctx) + (0x51, NN, 0x54, NN, None if source is None else 0x52, NN, E if want_lt else None, NN, E if want_g else None, NN)
    assert [o is not None for o in out] == [want_lt, want_g]


@pytest.mark.parametrize("scatter,ld", [(SC1, 0), (SC2, NN)])
@pytest.mark.parametrize("direct", [None, "device"])
@pytest.mark.parametrize("thermal", [None, "host"])
@pytest.mark.parametrize("want_y", [True, False])
def test_scatter_response_call(scatter, ld, direct, thermal, want_y):
    ctx = Recorder()
    out = ops.scatter_response(NUS, T, RD, W, A, scatter, S, COT, ctx=ctx, direct=None if direct is None else DIRECT,
                               thermal=None if thermal is None else 3.0 * PLANE, tol=0.0, max_iter=1, device=True, want_y=want_y)
    args = one_call(ctx, "sdx_scatter_response_dev")
    assert args == head(ctx) + (0x51, NN, scatter.ptr, ld, None if thermal is None else up(ctx, 3.0 * PLANE), NN, 0x52, NN, 0x55, NN,
                                None if direct is None else 0x56, NN, 0.0, 1, E if want_y else None, NN, E, NN, E, NN, E, NN, E, E, E)
    assert (out.y is not None) == want_y and out.R_thermal.ptr == E and out.R_absorption.ptr == E and out.R_scatter.ptr == E
    assert out.status.shape == (NN,)


def test_raytrace_arrays_checks_the_source_plane_only():
    ctx = Recorder()
    odd = dev(0x61, (5, 7))  # (no shape check of total_alphas, nor of the ray table beyond numpy's reshape)
    assert ops.raytrace_arrays(NUS, T, RD, W, odd, ctx=ctx, want_flux=False) == (None, None)
    assert one_call(ctx, "sdx_raytrace_dev") == head(ctx) + (0x61, NN, None, NN, None, 0)
    with pytest.raises(ValueError) as e:
        ops.raytrace_arrays(NUS, T, RD, W, odd, ctx=Recorder(), want_flux=False, source=np.ones((2, 2)))
    assert str(e.value) == "source function must return shape (3, 2), got (2, 2)"


# ---- the refusals the wrappers make themselves, before any device is asked for ------------------------------------------------------------
BAD = np.ones((2, 2))
SHORT = dev(0x71, (2, 2))
RD65, W65 = np.ones((ND - 1, 65)), np.ones(65)
SOURCE_TEXT = "source function must return shape (3, 2), got (2, 2)"
ALPHAS_TEXT = "total_alphas must have shape (3, 2), got (2, 2)"
RD_TEXT = "ray_distances must have shape (2, 2), got (3, 2)"
SC_TEXT = "alpha_scatter must have shape (3,) or (3, 2), got (2,)"
nd = NoDevice


def lam(what, **planes):
    """the refusals of the four scattering wrappers' shared intake, for the wrapper `what` called as f(ray_distances, weights, alphas, **kw)"""
    f = {"mean_intensity": lambda rd, w, a, **kw: ops.mean_intensity(NUS, T, rd, w, a, ctx=nd(), **kw),
         "scatter_source": lambda rd, w, a, **kw: ops.scatter_source(NUS, T, rd, w, a, SC1, ctx=nd(), **kw),
         "mean_intensity_adjoint": lambda rd, w, a, **kw: ops.mean_intensity_adjoint(NUS, T, rd, w, a, kw.pop("z", Z), ctx=nd(), **kw),
         "scatter_response": lambda rd, w, a, **kw: ops.scatter_response(NUS, T, rd, w, a, SC1, kw.pop("S", S), kw.pop("cotangent", COT), ctx=nd(),
                                                                         **kw)}[what]
    cases = [(lambda: f(RD65, W65, A), f"{what}: more than 64 angles are not supported, got 65"),
             (lambda: f(np.ones((3, 2)), W, A), RD_TEXT),
             (lambda: f(np.ones((2, 0)), np.ones(0), A), "ray_distances must have shape (2, 0), got (2, 0)"),
             (lambda: f(RD, W, SHORT), ALPHAS_TEXT),
             (lambda: f(RD, W, BAD), ALPHAS_TEXT)]
    for name in planes:
        cases.append((lambda name=name: f(RD, W, A, **{name: BAD}), f"{name} must have shape (3, 2), got (2, 2)"))
        cases.append((lambda name=name: f(RD, W, A, **{name: SHORT}), f"{name} must have shape (3, 2), got (2, 2)"))
    return cases


REFUSALS = [
    (lambda: ops.contribution_arrays(NUS, T, RD, W, A, ctx=nd(), source=BAD), SOURCE_TEXT),
    (lambda: ops.emergent_intensity(NUS, T, np.ones((3, 2)), A, ctx=nd()), "ray_distances must have shape (2, N_theta), got (3, 2)"),
    (lambda: ops.emergent_intensity(NUS, T, np.ones(4), A, ctx=nd()), "ray_distances must have shape (2, N_theta), got (4,)"),
    (lambda: ops.emergent_intensity(NUS, T, np.ones((2, 0)), A, ctx=nd()), "ray_distances must have shape (2, N_theta), got (2, 0)"),
    (lambda: ops.emergent_intensity(NUS, T[:1], np.ones((0, 2)), A, ctx=nd()), "ray_distances must have shape (0, N_theta), got (0, 2)"),
    (lambda: ops.emergent_intensity(NUS, T, RD65, A, ctx=nd()), "at most 64 angles are traced in one launch, got 65"),
    (lambda: ops.emergent_intensity(NUS, T, RD, SHORT, ctx=nd()), ALPHAS_TEXT),
    (lambda: ops.emergent_intensity(NUS, T, RD, BAD, ctx=nd()), ALPHAS_TEXT),
    (lambda: ops.emergent_intensity(NUS, T, RD, A, ctx=nd(), source=BAD), SOURCE_TEXT),
    (lambda: ops.response(NUS, T, np.ones((3, 2)), W, A, ctx=nd()), RD_TEXT),
    (lambda: ops.response(NUS, T[:1], np.ones((0, 2)), W, A, ctx=nd()), "ray_distances must have shape (0, 2), got (0, 2)"),
    (lambda: ops.response(NUS, T, RD, W, SHORT, ctx=nd()), ALPHAS_TEXT),
    (lambda: ops.response(NUS, T, RD, W, A, ctx=nd(), source=BAD), SOURCE_TEXT),
    (lambda: ops.response(NUS, T, RD, W, A, ctx=nd(), want_opacity=False, want_source=False), "response: no output requested"),
    (lambda: ops.response_angles(NUS, T, RD, np.ones((2, 3)), A, ctx=nd()), "cotangent must have shape (n_theta, 2), got (2, 3)"),
    (lambda: ops.response_angles(NUS, T, RD, np.ones(2), A, ctx=nd()), "cotangent must have shape (n_theta, 2), got (2,)"),
    (lambda: ops.response_angles(NUS, T, RD, dev(0x72, (0, 2)), A, ctx=nd()), "cotangent must have shape (n_theta, 2), got (0, 2)"),
    (lambda: ops.response_angles(NUS, T, np.ones((3, 2)), ANGLES, A, ctx=nd()), RD_TEXT),
    (lambda: ops.response_angles(NUS, T, RD, ANGLES, SHORT, ctx=nd()), ALPHAS_TEXT),
    (lambda: ops.response_angles(NUS, T, RD, ANGLES, A, ctx=nd(), source=BAD), SOURCE_TEXT),
    (lambda: ops.response_angles(NUS, T, RD, ANGLES, A, ctx=nd(), want_opacity=False, want_source=False), "response_angles: no output requested"),
    *lam("mean_intensity", source=None),
    (lambda: ops.mean_intensity(NUS, T, RD, W, A, ctx=nd(), want_J=False, want_L=False), "mean_intensity: no output requested"),
    *lam("scatter_source", thermal=None),
    (lambda: ops.scatter_source(NUS, T, RD, W, A, np.ones(2), ctx=nd()), SC_TEXT),
    (lambda: ops.scatter_source(NUS, T, RD, W, A, dev(0x73, (2,)), ctx=nd()), SC_TEXT),
    (lambda: ops.scatter_source(NUS, T, RD, W, A, SC1, ctx=nd(), tol=-1.0), "scatter_source: tol must be >= 0, got -1.0"),
    (lambda: ops.scatter_source(NUS, T, RD, W, A, SC1, ctx=nd(), tol=float("nan")), "scatter_source: tol must be >= 0, got nan"),
    (lambda: ops.scatter_source(NUS, T, RD, W, A, SC1, ctx=nd(), max_iter=0), "scatter_source: max_iter must be >= 1, got 0"),
    *lam("mean_intensity_adjoint", z=None, source=None),
    (lambda: ops.mean_intensity_adjoint(NUS, T, RD, W, A, None, ctx=nd()), "mean_intensity_adjoint: z is required"),
    (lambda: ops.mean_intensity_adjoint(NUS, T, RD, W, A, Z, ctx=nd(), want_Lt=False, want_G=False), "mean_intensity_adjoint: no output requested"),
    *lam("scatter_response", S=None, cotangent=None, direct=None, thermal=None),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, SC1, None, COT, ctx=nd()), "scatter_response: S and cotangent are required"),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, SC1, S, None, ctx=nd()), "scatter_response: S and cotangent are required"),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, np.ones(2), S, COT, ctx=nd()), SC_TEXT),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, SC1, S, COT, ctx=nd(), tol=-1.0), "scatter_response: tol must be >= 0, got -1.0"),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, SC1, S, COT, ctx=nd(), tol=float("nan")), "scatter_response: tol must be >= 0, got nan"),
    (lambda: ops.scatter_response(NUS, T, RD, W, A, SC1, S, COT, ctx=nd(), max_iter=0), "scatter_response: max_iter must be >= 1, got 0"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusal(k):
    call, text = REFUSALS[k]
    with pytest.raises(ValueError) as e:
        call()
    assert type(e.value) is ValueError and str(e.value) == text


def test_refusals_come_in_todays_order():
    """a call wrong in several ways: the angle count before the ray table before total_alphas before the planes before alpha_scatter, tol,
    max_iter and the outputs"""
    with pytest.raises(ValueError, match="more than 64 angles"):
        ops.scatter_source(NUS, T, np.ones((3, 2)), W65, BAD, np.ones(2), ctx=nd(), thermal=BAD, tol=-1.0)
    with pytest.raises(ValueError, match="ray_distances"):
        ops.scatter_source(NUS, T, np.ones((3, 2)), W, BAD, np.ones(2), ctx=nd(), thermal=BAD, tol=-1.0)
    with pytest.raises(ValueError, match="total_alphas"):
        ops.scatter_source(NUS, T, RD, W, BAD, np.ones(2), ctx=nd(), thermal=BAD, tol=-1.0)
    with pytest.raises(ValueError, match="thermal must"):
        ops.scatter_source(NUS, T, RD, W, A, np.ones(2), ctx=nd(), thermal=BAD, tol=-1.0)
    with pytest.raises(ValueError, match="alpha_scatter"):
        ops.scatter_source(NUS, T, RD, W, A, np.ones(2), ctx=nd(), tol=-1.0, max_iter=0)
    with pytest.raises(ValueError, match="tol must"):
        ops.scatter_source(NUS, T, RD, W, A, SC1, ctx=nd(), tol=-1.0, max_iter=0)
    with pytest.raises(ValueError, match="ray_distances"):
        ops.emergent_intensity(NUS, T, np.ones((3, 65)), BAD, ctx=nd(), source=BAD)
    with pytest.raises(ValueError, match="at most 64"):
        ops.emergent_intensity(NUS, T, RD65, BAD, ctx=nd(), source=BAD)
    with pytest.raises(ValueError, match="cotangent"):
        ops.response_angles(NUS, T, np.ones((3, 2)), np.ones(2), BAD, ctx=nd())
    with pytest.raises(ValueError, match="source function"):
        ops.response(NUS, T, RD, W, A, ctx=nd(), source=BAD, want_opacity=False, want_source=False)
    with pytest.raises(ValueError, match="z is required"):
        ops.mean_intensity_adjoint(NUS, T, RD, W, A, None, ctx=nd(), want_Lt=False, want_G=False)


# ---- the C entry points and a null context -------------------------------------------------------------------------------------------------
NULL_CONTEXT = {
    "sdx_raytrace_f64": "raytrace",
    "sdx_contribution_dev": "contribution", "sdx_contribution_f64": "contribution",
    "sdx_emergent_intensity_dev": "emergent_intensity", "sdx_emergent_intensity_f64": "emergent_intensity",
    "sdx_response_dev": "response", "sdx_response_f64": "response",
    "sdx_response_angles_dev": "response_angles", "sdx_response_angles_f64": "response",  # (both twins speak as "response" here)
    "sdx_mean_intensity_dev": "mean_intensity", "sdx_mean_intensity_f64": "mean_intensity",
    "sdx_scatter_source_dev": "scatter_source", "sdx_scatter_source_f64": "scatter_source",
    "sdx_mean_intensity_adjoint_dev": "mean_intensity_adjoint", "sdx_mean_intensity_adjoint_f64": "mean_intensity_adjoint",
    "sdx_scatter_response_dev": "scatter_response", "sdx_scatter_response_f64": "scatter_response",
}


@pytest.mark.parametrize("entry", sorted(NULL_CONTEXT))
@pytest.mark.parametrize("n_nu", [0, 2])
def test_null_context(entry, n_nu):
    """-1 and "<name>: need n_depth >= 2, n_theta > 0", before any pointer is looked at, for an empty grid too"""
    assert len(NULL_CONTEXT) == 17
    lib = _lib.load()
    _, argtypes = _lib.PROTOTYPES[entry]
    args = [3, n_nu, 2] + [None if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") else t(0).value for t in argtypes[4:]]
    assert getattr(lib, entry)(None, *args) == -1
    assert lib.sdx_last_error_code() == -1
    assert lib.sdx_last_error_string().decode() == NULL_CONTEXT[entry] + ": need n_depth >= 2, n_theta > 0"
