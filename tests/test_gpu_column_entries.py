"""The products of the formal solution over the grid's columns, entry by entry: every host-buffer twin (sdx_*_f64) gives its device
entry's bytes, and every entry refuses what it refuses with the code and the words it has always had.

Shapes: 2, 3 and 9 depths; 1, 3, 20 and 64 angles (one group, a group that does not divide a wave, the usual one, a full wave); 1 and 7
frequencies, the 7 columns of the device planes 8 apart.  Forms: with a source (thermal) plane and without, alpha_scatter per depth and
per (depth, frequency), inward rays for the intensities, every optional output absent in turn, an empty grid.  The refusals are tables
of (call, message): every one returns before anything is launched.  scripts/lib_ab.py (`columns`) drives the same calls on two builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTHS, ANGLES, FREQUENCIES = (2, 3, 9), (1, 3, 20, 64), (1, 7)
FILL = -7.0  # what an output holds before the call
TOL, MAX_ITER = 1e-10, 40

# entry -> the device entry's arguments behind (n_depth, n_nu, n_theta); x:ld is a pointer and its leading dimension.  The twin takes the
# same without the leading dimensions, sc:ld as (sc, per_frequency)
DEVICE = {
    "raytrace": "nus temps ray w alphas:ld F:ld I_nus accumulate",
    "contribution": "nus temps ray w alphas:ld source:ld C:ld",
    "emergent_intensity": "nus temps ray alphas:ld source:ld inward I:ld",
    "response": "nus temps ray w alphas:ld source:ld Ra:ld Rs:ld",
    "response_angles": "nus temps ray cot:ld alphas:ld source:ld Ra:ld Rs:ld",
    "mean_intensity": "nus temps ray m alphas:ld source:ld J:ld L:ld",
    "scatter_source": "nus temps ray m alphas:ld sc:ld thermal:ld tol max_iter S_out:ld J:ld it st ch",
    "mean_intensity_adjoint": "nus temps ray m alphas:ld z:ld source:ld Lt:ld G:ld",
    "scatter_response": "nus temps ray m alphas:ld sc:ld thermal:ld S:ld c:ld direct:ld tol max_iter y:ld Rt:ld Rab:ld Rsc:ld it st ch",
}
PRODUCTS = [e for e in DEVICE if e != "raytrace"]
OUTPUTS = {"raytrace": "F I_nus", "contribution": "C", "emergent_intensity": "I", "response": "Ra Rs", "response_angles": "Ra Rs", "mean_intensity": "J L",
           "scatter_source": "S_out J it st ch", "mean_intensity_adjoint": "Lt G", "scatter_response": "y Rt Rab Rsc it st ch"}
REQUIRED = {"F", "C", "I", "S_out"}  # (the other outputs may be absent, though not all of an entry's planes at once)
PLANE_OF = {"raytrace": None, "scatter_source": "thermal", "scatter_response": "thermal"}  # the optional source plane's name; default "source"


def tokens(entry, twin):
    sig = DEVICE[entry].split()
    if not twin:
        return sig
    return [t for s in sig if s != "accumulate" for t in (["sc", "per_frequency"] if s == "sc:ld" else [s.replace(":ld", "")])]


class Problem:
    """seeded inputs of one shape on the host (n_nu columns) and on the device (ld columns)"""

    def __init__(self, ctx, n_depth, n_theta, n_nu, seed=1):
        rng = np.random.default_rng([seed, n_depth, n_theta, n_nu])
        self.ctx, self.n_depth, self.n_theta, self.n_nu, self.ld = ctx, n_depth, n_theta, n_nu, 8 if n_nu == 7 else n_nu
        nd, nt, nn = n_depth, n_theta, n_nu
        thetas = (np.arange(nt) + 0.5) * (0.5 * np.pi / nt) * 0.98
        w = rng.uniform(0.5, 1.5, nt) / nt
        x = w * np.sin(thetas)
        alphas = 10.0 ** rng.uniform(-8.0, -6.0, (nd, nn))
        h = dict(nus=np.sort(rng.uniform(3.0e14, 8.0e14, nn))[::-1].copy(), temps=np.sort(rng.uniform(4000.0, 9000.0, nd)),
                 ray=rng.uniform(2.0e5, 2.0e7, (nd - 1, 1)) / np.cos(thetas), w=w, m=x / (2.0 * x.sum()), cot=rng.uniform(-1.0, 1.0, (nt, nn)), alphas=alphas,
                 source=rng.uniform(0.5, 2.0, (nd, nn)) * 1e-5, thermal=rng.uniform(0.5, 2.0, (nd, nn)) * 1e-5, sc=alphas * rng.uniform(0.0, 0.6, (nd, nn)),
                 sc1=alphas.min(axis=1) * rng.uniform(0.0, 0.6, nd), z=rng.uniform(-1.0, 1.0, (nd, nn)), S=rng.uniform(0.5, 2.0, (nd, nn)) * 1e-5,
                 c=rng.uniform(-1.0, 1.0, (nd, nn)), direct=rng.uniform(-1.0, 1.0, (nd, nn)), F=rng.uniform(0.0, 1.0, (nd, nn)))
        self.host = {k: np.ascontiguousarray(a) for k, a in h.items()}
        self.device = {k: ctx.upload(self.padded(a)) for k, a in self.host.items()}

    def padded(self, a):
        if a.ndim != 2 or a.shape[1] != self.n_nu or a is self.host.get("ray"):
            return a
        out = np.full((a.shape[0], self.ld), np.nan)
        out[:, :self.n_nu] = a
        return out

    def shape(self, name):
        nd, nt, nn = self.n_depth, self.n_theta, self.n_nu
        return {"I": (nt, nn), "I_nus": (nd, nn, nt), "it": (nn,), "st": (nn,), "ch": (nn,)}.get(name, (nd, nn))

    def arguments(self, entry, twin, form, outs, **over):
        """the argument tuple of a call.  form: plane (the source or thermal plane is given), sc2d, inward, drop (outputs left out); outs:
        {name: array}; over: arguments by name (x, x_ld) that replace what the problem would pass"""
        v = dict(n_depth=self.n_depth, n_nu=self.n_nu, n_theta=self.n_theta, tol=TOL, max_iter=MAX_ITER, inward=form.get("inward", 0), accumulate=1,
                 per_frequency=1 if form.get("sc2d", True) else 0)
        address = (lambda a: a.ctypes.data) if twin else (lambda a: a.ptr)
        arrays = self.host if twin else self.device
        for name, a in arrays.items():
            v[name], v[name + "_ld"] = address(a), self.ld
        if not form.get("sc2d", True):
            v["sc"], v["sc_ld"] = address(arrays["sc1"]), 0
        if not form.get("plane", True):
            v[PLANE_OF.get(entry, "source")] = None
        for name in OUTPUTS[entry].split():
            v[name], v[name + "_ld"] = (None if outs.get(name) is None else address(outs[name])), self.ld
        v.update(over)
        args = [v["n_depth"], v["n_nu"], v["n_theta"]]
        for t in tokens(entry, twin):
            args += [v[t[:-3]], v[t[:-3] + "_ld"]] if t.endswith(":ld") else [v[t]]
        return tuple(args)

    def outputs(self, entry, twin, form):
        """fresh outputs, FILL everywhere (F: the flux the call adds to); a dropped one is None"""
        outs = {}
        for name in OUTPUTS[entry].split():
            if name in form.get("drop", ()):
                outs[name] = None
                continue
            shape, dtype = self.shape(name), np.int32 if name in ("it", "st") else np.float64
            a = self.host["F"].astype(dtype) if name == "F" else np.full(shape, FILL, dtype=dtype)
            if not twin:
                a = self.ctx.upload(self.padded(a) if name != "I_nus" else a, dtype)
            outs[name] = a
        return outs

    def run(self, entry, twin, form):
        """one call -> {output: host array of n_nu columns, or None}"""
        outs = self.outputs(entry, twin, form)
        self.ctx.call(f"sdx_{entry}_{'f64' if twin else 'dev'}", *self.arguments(entry, twin, form, outs))
        if twin:
            return outs
        self.ctx.synchronize()
        planes = {name: a for name, a in outs.items() if a is not None and len(self.shape(name)) == 2}
        return {name: None if a is None else np.ascontiguousarray(a.numpy()[:, :self.n_nu]) if name in planes else a.numpy() for name, a in outs.items()}


def forms(entry):
    """the forms of an entry that differ in what it reads and writes"""
    out = [dict(plane=True, sc2d=True, inward=0), dict(plane=False, sc2d=False, inward=1)]
    for name in OUTPUTS[entry].split():
        if name not in REQUIRED:
            out.append(dict(plane=True, sc2d=True, inward=0, drop=(name,)))
    if entry == "scatter_response":
        out.append(dict(plane=True, sc2d=False, inward=0, drop=("y", "Rab", "Rsc", "it", "st", "ch")))
    return out


@functools.lru_cache(maxsize=None)
def problem(ctx, n_depth, n_theta, n_nu):
    return Problem(ctx, n_depth, n_theta, n_nu)


# ---- 1. the twins give the device entries' bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth", DEPTHS)
@pytest.mark.parametrize("entry", list(DEVICE))
def test_twin_gives_the_device_entry_bytes(ctx, entry, n_depth):
    for n_theta in ANGLES:
        for n_nu in FREQUENCIES:
            p = problem(ctx, n_depth, n_theta, n_nu)
            for form in forms(entry):
                dev, twin = p.run(entry, False, form), p.run(entry, True, form)
                for name in OUTPUTS[entry].split():
                    where = (entry, n_depth, n_theta, n_nu, form, name)
                    if name in form.get("drop", ()):
                        assert dev[name] is None and twin[name] is None, where
                        continue
                    assert dev[name].shape == twin[name].shape == p.shape(name) and dev[name].dtype == twin[name].dtype, where
                    assert dev[name].tobytes() == twin[name].tobytes(), where
                    assert not (twin[name] == (p.host["F"] if name == "F" else FILL)).all(), where  # (it was written)


@pytest.mark.parametrize("entry", list(DEVICE))
def test_empty_grid(ctx, entry):
    """n_nu = 0: nothing is read, nothing is launched, both forms return SDX_OK — with null pointers too"""
    p = problem(ctx, 9, 3, 7)
    for twin in (False, True):
        if entry == "raytrace" and not twin:
            continue
        outs = p.outputs(entry, twin, {})
        p.ctx.call(f"sdx_{entry}_{'f64' if twin else 'dev'}", *p.arguments(entry, twin, {}, outs, n_nu=0))
        nothing = {t[:-3] if t.endswith(":ld") else t: None for t in tokens(entry, twin) if t.split(":")[0] in p.host or t.split(":")[0] in OUTPUTS[entry].split()}
        p.ctx.call(f"sdx_{entry}_{'f64' if twin else 'dev'}", *p.arguments(entry, twin, {}, {}, n_nu=0, **nothing))
        if twin:
            for name, a in outs.items():
                assert (a == (p.host["F"] if name == "F" else FILL)).all(), (entry, name)


# ---- 2. the refusals --------------------------------------------------------------------------------------------------------------------
NEED = "need n_depth >= 2, n_theta > 0"
ANGLES64 = "more than 64 angles are not supported (all angles are traced in one launch)"
RESPONSE_MIXED = "no response functions with mixed_precision = 1 (they differentiate the fp64 formal solution)"
RESPONSE_DEEP = "no response functions for models this deep (the columns and the stashed intensities do not fit LDS)"
LAMBDA_MIXED = "not with mixed_precision = 1 (the mean intensity is that of the fp64 formal solution)"
LAMBDA_DEEP = "models this deep are not served (the columns of one frequency do not fit LDS)"
ADJOINT_DEEP = "models this deep are not served (the columns and stashed values of one frequency do not fit LDS)"
# entry -> (the mixed_precision sentence, the sentence for a model too deep, that model's (n_depth, n_theta): the ones the entries' own tests use)
GATE = {
    "contribution": ("no contribution function with mixed_precision = 1 (it decomposes the fp64 formal solution)",
                     "no contribution function for models this deep (the columns do not fit LDS)", (1100, 1)),
    "emergent_intensity": ("no emergent intensities with mixed_precision = 1 (they are the fp64 formal solution's last row)",
                           "no emergent intensities for models this deep (the columns do not fit LDS)", (1100, 1)),
    "response": (RESPONSE_MIXED, RESPONSE_DEEP, (1000, 7)), "response_angles": (RESPONSE_MIXED, RESPONSE_DEEP, (1000, 7)),
    "mean_intensity": (LAMBDA_MIXED, LAMBDA_DEEP, (1400, 7)), "scatter_source": (LAMBDA_MIXED, LAMBDA_DEEP, (1400, 7)),
    "mean_intensity_adjoint": (LAMBDA_MIXED, ADJOINT_DEEP, (500, 7)), "scatter_response": (LAMBDA_MIXED, ADJOINT_DEEP, (500, 7)),
}
SOURCE = "bad source plane (source_ld < n_nu), or neither a source plane nor temperatures"
THERMAL = "bad thermal plane (thermal_ld < n_nu), or neither a thermal plane nor temperatures"
ITERATION = "need tol >= 0 (not NaN) and max_iter >= 1"
NAN = float("nan")
ALL_PLANES = dict(y=None, Rt=None, Rab=None, Rsc=None)
# entry -> [(arguments replaced, the message behind "<entry>: ")] of the DEVICE entry, at 9 depths, 7 angles, 7 frequencies 8 apart (short: 6)
DEVICE_REFUSALS = {
    "contribution": [(dict(nus=None), "null pointer or leading dimension below n_nu"), (dict(w=None), "null pointer or leading dimension below n_nu"),
                     (dict(alphas_ld=6), "null pointer or leading dimension below n_nu"), (dict(C=None), "null pointer or leading dimension below n_nu"),
                     (dict(C_ld=6), "null pointer or leading dimension below n_nu"), (dict(source_ld=6), SOURCE), (dict(source=None, temps=None), SOURCE)],
    "emergent_intensity": [(dict(ray=None), "null pointer or leading dimension below n_nu"), (dict(alphas_ld=6), "null pointer or leading dimension below n_nu"),
                           (dict(I=None), "null pointer or leading dimension below n_nu"), (dict(I_ld=6), "null pointer or leading dimension below n_nu"),
                           (dict(source_ld=6), SOURCE), (dict(source=None, temps=None), SOURCE),
                           (dict(I="alphas"), "not in place (I_out must not be one of the inputs)"),
                           (dict(I="nus", n_nu=0), "not in place (I_out must not be one of the inputs)")],
    "response": [(dict(Ra=None, Rs=None), "no output requested"), (dict(nus=None), "null pointer or alpha_ld below n_nu"),
                 (dict(alphas_ld=6), "null pointer or alpha_ld below n_nu"), (dict(Rs_ld=6), "leading dimension of an output below n_nu"),
                 (dict(source_ld=6), SOURCE), (dict(source=None, temps=None), SOURCE)],
    "response_angles": [(dict(Ra=None, Rs=None), "no output requested"), (dict(cot=None), "null pointer or alpha_ld below n_nu"),
                        (dict(cot_ld=6), "cot_ld below n_nu"), (dict(Ra_ld=6), "leading dimension of an output below n_nu"), (dict(source_ld=6), SOURCE),
                        (dict(Rs="cot"), "not in place (an output must not be the cotangent)")],
    "mean_intensity": [(dict(J=None, L=None), "no output requested"), (dict(m=None), "null pointer or alpha_ld below n_nu"),
                       (dict(alphas_ld=6), "null pointer or alpha_ld below n_nu"), (dict(L_ld=6), "leading dimension of an output below n_nu"),
                       (dict(source_ld=6), SOURCE), (dict(source=None, temps=None), SOURCE)],
    "scatter_source": [(dict(tol=-1.0), ITERATION), (dict(tol=NAN), ITERATION), (dict(max_iter=0), ITERATION), (dict(tol=-1.0, n_nu=0), ITERATION),
                       (dict(max_iter=0, nus=None, S_out=None), ITERATION), (dict(sc=None), "null pointer or alpha_ld below n_nu"),
                       (dict(S_out=None), "null pointer or alpha_ld below n_nu"), (dict(S_out_ld=6), "a leading dimension below n_nu (scatter_ld: 0 or >= n_nu)"),
                       (dict(sc_ld=6), "a leading dimension below n_nu (scatter_ld: 0 or >= n_nu)"),
                       (dict(J_ld=6), "a leading dimension below n_nu (scatter_ld: 0 or >= n_nu)"), (dict(thermal_ld=6), THERMAL),
                       (dict(thermal=None, temps=None), THERMAL)],
    "mean_intensity_adjoint": [(dict(Lt=None, G=None), "no output requested"), (dict(z=None), "null pointer or a leading dimension of an input below n_nu"),
                               (dict(z_ld=6), "null pointer or a leading dimension of an input below n_nu"),
                               (dict(G_ld=6), "leading dimension of an output below n_nu"), (dict(source_ld=6), SOURCE)],
    "scatter_response": [(dict(tol=-1.0), ITERATION), (dict(tol=NAN), ITERATION), (dict(max_iter=0), ITERATION), (dict(tol=-1.0, n_nu=0), ITERATION),
                         (ALL_PLANES, "no output requested"), (dict(S=None), "null pointer or alpha_ld below n_nu"),
                         (dict(c=None), "null pointer or alpha_ld below n_nu"), (dict(c_ld=6), "a leading dimension of an input below n_nu (scatter_ld: 0 or >= n_nu)"),
                         (dict(direct_ld=6), "a leading dimension of an input below n_nu (scatter_ld: 0 or >= n_nu)"),
                         (dict(Rt_ld=6), "leading dimension of an output below n_nu"), (dict(thermal_ld=6), THERMAL), (dict(thermal=None, temps=None), THERMAL)],
}
# the same of the twins: host pointers, no leading dimensions; both response twins speak as "response" of pointers and outputs
TWIN_REFUSALS = {
    "contribution": [(dict(temps=None), "null pointer"), (dict(C=None), "null pointer")],
    "emergent_intensity": [(dict(temps=None), "null pointer"), (dict(I=None), "null pointer")],
    "response": [(dict(w=None), "null pointer"), (dict(Ra=None, Rs=None), "no output requested")],
    "response_angles": [(dict(cot=None), "response: null pointer"), (dict(Ra=None, Rs=None), "response: no output requested")],
    "mean_intensity": [(dict(temps=None), "null pointer"), (dict(J=None, L=None), "no output requested")],
    "scatter_source": [(dict(tol=-1.0), ITERATION), (dict(tol=NAN), ITERATION), (dict(max_iter=0), ITERATION), (dict(tol=-1.0, n_nu=0), ITERATION),
                       (dict(sc=None), "null pointer"), (dict(S_out=None), "null pointer")],
    "mean_intensity_adjoint": [(dict(z=None), "null pointer"), (dict(Lt=None, G=None), "no output requested")],
    "scatter_response": [(dict(tol=-1.0), ITERATION), (dict(tol=NAN), ITERATION), (dict(max_iter=0), ITERATION), (dict(max_iter=0, n_nu=0), ITERATION),
                         (dict(c=None), "null pointer"), (ALL_PLANES, "no output requested")],
}


def refused(p, entry, twin, over, message):
    """the call returns SDX_ERR_ARG and leaves exactly `message`; a name in place of a pointer: that input's address"""
    outs = p.outputs(entry, twin, {})
    arrays = p.host if twin else p.device
    over = {k: ((arrays[v].ctypes.data if twin else arrays[v].ptr) if isinstance(v, str) else v) for k, v in over.items()}
    name = f"sdx_{entry}_{'f64' if twin else 'dev'}"
    rc = getattr(p.ctx.lib, name)(p.ctx.handle, *p.arguments(entry, twin, {}, outs, **over))
    said = p.ctx.lib.sdx_last_error_string().decode()
    print(name, over, "->", rc, said)
    assert (rc, said) == (-1, message if message.split(":")[0] in DEVICE else f"{entry}: {message}"), (name, over)
    assert p.ctx.lib.sdx_last_error_code() == -1


@pytest.mark.parametrize("entry", PRODUCTS)
def test_refusals(ctx, entry):
    p = problem(ctx, 9, 7, 7)
    mixed, deep, (deep_depth, deep_theta) = GATE[entry]
    for twin in (False, True):
        shape_name = "response" if twin and entry == "response_angles" else entry  # (the response twins refuse a bad shape as "response")
        for n_nu in (7, 0):  # the gate, also at set-up time with an empty grid
            refused(p, entry, twin, dict(n_depth=1, n_nu=n_nu), f"{shape_name}: {NEED}")
            refused(p, entry, twin, dict(n_theta=0, n_nu=n_nu), f"{shape_name}: {NEED}")
            refused(p, entry, twin, dict(n_theta=65, n_nu=n_nu), ANGLES64)
            refused(p, entry, twin, dict(n_depth=deep_depth, n_theta=deep_theta, n_nu=n_nu), deep)
            # wrong in two ways: the gate speaks before the scalars, the pointers and the outputs (the twins of the contribution function,
            # the intensities and the responses looked at their pointers first until they took the order of the others)
            refused(p, entry, twin, dict(n_theta=65, n_nu=n_nu, nus=None, temps=None, alphas=None, tol=-1.0), ANGLES64)
        ctx.set_option("mixed_precision", 1)
        try:
            for n_nu in (7, 0):
                refused(p, entry, twin, dict(n_nu=n_nu), mixed)
            refused(p, entry, twin, dict(nus=None, max_iter=0), mixed)
        finally:
            ctx.set_option("mixed_precision", 0)
        for over, message in (TWIN_REFUSALS if twin else DEVICE_REFUSALS)[entry]:
            refused(p, entry, twin, over, message)
    # and the context still serves
    dev, twin = p.run(entry, False, {}), p.run(entry, True, {})
    assert all(dev[name].tobytes() == twin[name].tobytes() for name in OUTPUTS[entry].split())


def test_raytrace_twin_refusals(ctx):
    p = problem(ctx, 9, 7, 7)
    for over, message in ((dict(n_depth=1), NEED), (dict(n_theta=0, n_nu=0), NEED), (dict(F=None), "null pointer"), (dict(alphas=None), "null pointer")):
        refused(p, "raytrace", True, over, message)
