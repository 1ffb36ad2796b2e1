"""The nine host-pointer (*_f64) entry points on ONE context's arena and pinned buffer (HostIo and the HostPlan each call declares,
stardis_amd/csrc/sdx_host_plan.h): calls of every entry interleaved on one fresh context, sizes going up and down and the optional rows
coming and going, so that each call lays its rows out in buffers an earlier, differently shaped call sized — every result is that of
the same call made alone on a context of its own and, where a *_dev entry exists, of that entry on uploaded copies, bit for bit.  The
same sequence in a child process without pinned staging (SDX_NO_PINNED_STAGING=1: the copies go straight from / to the caller's pages,
the shard's columns by a 2-D copy) gives the same bytes; sdx_synthesize_sharded_f64's column downloads assemble sdx_synthesize_f64's planes."""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
from stardis_amd import _lib, synth
from stardis_amd import constants as K

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
N_DEPTH, N_THETA, DOPPLER = 5, 3, 1.000003


def P(a):
    return None if a is None else a.ctypes.data


@functools.lru_cache(maxsize=None)
def problem(n_nu, n_lines, n_pix):
    """every host array of a call at this shape (never modified: the calls copy what they hand over as in/out)"""
    rng = np.random.default_rng(1000 * n_nu + 10 * n_lines + n_pix)
    sun = synth.solar_atmosphere()
    idx = np.linspace(0, sun["temperatures"].size - 1, N_DEPTH).round().astype(int)
    r = sun["r"][idx]
    atm = dict(temperatures=sun["temperatures"][idx].copy(), r=r, dist=(r[1:] - r[:-1]).copy(), n_e=sun["n_e"][idx].copy(), n_h=sun["n_h"][idx].copy(),
               microturbulence=sun["microturbulence"])
    lam = 6560.0 + 0.05 * np.arange(n_nu)
    nus = K.C_CGS * 1.0e8 / lam
    th, w = synth.thetas_and_weights(N_THETA)
    p = NS(n_nu=n_nu, n_lines=n_lines, n_pix=n_pix, lam=lam, nus=nus, t=atm["temperatures"], w=np.ascontiguousarray(w),
           ray=np.ascontiguousarray(atm["dist"].reshape(-1, 1) / np.cos(th)))
    if n_lines:
        lines = synth.synth_lines(nus, atm, n_lines, seed=n_nu + n_lines)
        p.line_nus, p.doppler, p.gammas, p.alphas = lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"]
    else:
        p.line_nus, p.doppler, p.gammas, p.alphas = np.zeros(0), np.zeros((0, N_DEPTH)), np.zeros((0, 1)), np.zeros((0, N_DEPTH))
    p.gamma_cols = p.gammas.shape[1]
    plane = (N_DEPTH, n_nu)
    p.total = 1.0e-8 * (1.0 + rng.random(plane)) / np.abs(atm["dist"]).max() * 1.0e7
    p.source = 1.0e-5 * (1.0 + rng.random(plane))
    p.F0 = 1.0e-6 * (1.0 + rng.random(plane))  # (the flux the formal solution accumulates into)
    p.weight = rng.standard_normal(plane)
    p.flux, p.reference = 1.0 + rng.random(n_nu), 2.0 + rng.random(n_nu)
    p.edges = np.linspace(lam[0] + 0.5, lam[-1] - 0.5, n_pix + 1)
    p.sigma, p.pixel_weight = np.full(n_pix, 0.04), rng.standard_normal(n_pix)
    c = synth.synth_continuum_state(atm)
    cutoff = (c["ionization_energy"] - np.asarray(c["level_excitation"])) / K.H_CGS
    p.cont = dict(lambdas=lam, table_wavelength=c["hminus_bf_wavelength"], table_sigma=c["hminus_bf_cross_section"], table_density=c["n_hminus"],
                  bf_species_offsets=np.array([0, cutoff.size], np.int32), bf_species_ion_number=np.array([0], np.int32), bf_cutoff=cutoff,
                  bf_level_density=c["level_density"], ff_species_ion_number=np.array([1], np.int32),
                  ff_number_density=np.asarray(c["n_e"]) * np.asarray(c["n_h2"]), ray_n_h=c["n_h1"], ray_n_he=c["n_he1"], ray_n_h2=1.0e-4 * c["n_h1"],
                  electron_density=c["n_e"], temperature=atm["temperatures"])
    p.cont = {k: np.ascontiguousarray(v) for k, v in p.cont.items()}
    return p


def continuum_struct(p, pointer, without=()):
    """struct sdx_continuum over p.cont's arrays, their addresses by `pointer` (host: the array's own; device: an uploaded copy's)"""
    s = _lib.Continuum()
    s.n_table, s.bf_n_species, s.bf_n_levels, s.ff_n_species = p.cont["table_sigma"].size, 1, p.cont["bf_cutoff"].size, 1
    s.rayleigh_enabled = int(not set(RAYLEIGH) & set(without))  # (the kernels read the three densities whenever it is set)
    for name, a in p.cont.items():
        if name not in without:
            setattr(s, name, pointer(a))
    return s


class Uploads:
    """device copies that live as long as the call that reads them"""

    def __init__(self, ctx):
        self.ctx, self.keep = ctx, []

    def __call__(self, a):
        if a is None:
            return None
        d = self.ctx.upload(a, a.dtype) if a.size else self.ctx.empty(a.shape, a.dtype)
        self.keep.append(d)
        return d.ptr

    def empty(self, shape, dtype=np.float64):
        d = self.ctx.empty(shape, dtype)
        self.keep.append(d)
        return d


def nan(*shape):
    return np.full(shape, np.nan)


# ---- the entries: host(ctx, p, ...) through the *_f64 entry point, dev(ctx, p, ...) through the *_dev entry on uploaded copies --------
def line_opacity_host(ctx, p, empty_grid=False):
    n_nu = 0 if empty_grid else p.n_nu
    out, ev = nan(N_DEPTH, n_nu), C.c_int64(-1)
    rc = ctx.lib.sdx_line_opacity_f64(ctx.handle, N_DEPTH, n_nu, P(p.nus), p.n_lines, P(p.line_nus), P(p.doppler), P(p.gammas), p.gamma_cols, P(p.alphas),
                                      None if empty_grid else P(out), C.byref(ev))
    assert rc == 0, ctx.lib.sdx_last_error_string()
    return dict(out=out, evaluations=np.int64(ev.value))


def line_opacity_dev(ctx, p, empty_grid=False):
    if empty_grid:
        return dict(out=nan(N_DEPTH, 0), evaluations=np.int64(0))
    up = Uploads(ctx)
    out, ev = up.empty((N_DEPTH, p.n_nu)), up.empty(1, np.int64)
    ctx.call("sdx_line_opacity_dev", N_DEPTH, p.n_nu, up(p.nus), 0, p.n_nu, p.n_lines, up(p.line_nus), up(p.doppler), up(p.gammas), p.gamma_cols, up(p.alphas),
             out.ptr, p.n_nu, 0, ev.ptr)
    return dict(out=out.numpy(), evaluations=ev.numpy()[0])


def raytrace_host(ctx, p, i_nus):
    F, I = p.F0.copy(), nan(N_THETA * N_DEPTH * p.n_nu) if i_nus else None
    ctx.call("sdx_raytrace_f64", N_DEPTH, p.n_nu, N_THETA, P(p.nus), P(p.t), P(p.ray), P(p.w), P(p.total), P(F), P(I))
    return dict(F=F, **({"I_nus": I} if i_nus else {}))


def raytrace_dev(ctx, p, i_nus):
    up = Uploads(ctx)
    F, I = up(p.F0), up.empty(N_THETA * N_DEPTH * p.n_nu) if i_nus else None
    ctx.call("sdx_raytrace_dev", N_DEPTH, p.n_nu, N_THETA, up(p.nus), up(p.t), up(p.ray), up(p.w), up(p.total), p.n_nu, F, p.n_nu, I.ptr if i_nus else None, 1)
    return dict(F=up.keep[0].numpy(), **({"I_nus": I.numpy()} if i_nus else {}))


def contribution_host(ctx, p, source):
    out = nan(N_DEPTH, p.n_nu)
    ctx.call("sdx_contribution_f64", N_DEPTH, p.n_nu, N_THETA, P(p.nus), P(p.t), P(p.ray), P(p.w), P(p.total), P(p.source) if source else None, P(out))
    return dict(C=out)


def contribution_dev(ctx, p, source):
    up = Uploads(ctx)
    out = up.empty((N_DEPTH, p.n_nu))
    ctx.call("sdx_contribution_dev", N_DEPTH, p.n_nu, N_THETA, up(p.nus), up(p.t), up(p.ray), up(p.w), up(p.total), p.n_nu, up(p.source) if source else None, p.n_nu,
             out.ptr, p.n_nu)
    return dict(C=out.numpy())


def response_host(ctx, p, source, r_alpha, r_source):
    a, s = nan(N_DEPTH, p.n_nu) if r_alpha else None, nan(N_DEPTH, p.n_nu) if r_source else None
    ctx.call("sdx_response_f64", N_DEPTH, p.n_nu, N_THETA, P(p.nus), P(p.t), P(p.ray), P(p.w), P(p.total), P(p.source) if source else None, P(a), P(s))
    return {k: v for k, v in (("R_alpha", a), ("R_source", s)) if v is not None}


def response_dev(ctx, p, source, r_alpha, r_source):
    up = Uploads(ctx)
    a, s = up.empty((N_DEPTH, p.n_nu)) if r_alpha else None, up.empty((N_DEPTH, p.n_nu)) if r_source else None
    ctx.call("sdx_response_dev", N_DEPTH, p.n_nu, N_THETA, up(p.nus), up(p.t), up(p.ray), up(p.w), up(p.total), p.n_nu, up(p.source) if source else None, p.n_nu,
             a.ptr if a else None, p.n_nu, s.ptr if s else None, p.n_nu)
    return {k: v.numpy() for k, v in (("R_alpha", a), ("R_source", s)) if v is not None}


def line_adjoint_host(ctx, p, out_line, out_line_depth):
    a, b = nan(p.n_lines) if out_line else None, nan(p.n_lines, N_DEPTH) if out_line_depth else None
    ctx.call("sdx_line_adjoint_f64", N_DEPTH, p.n_nu, P(p.nus), p.n_lines, P(p.line_nus), P(p.doppler), P(p.gammas), p.gamma_cols, P(p.alphas), P(p.weight), P(a), P(b))
    return {k: v for k, v in (("out_line", a), ("out_line_depth", b)) if v is not None}


def line_adjoint_dev(ctx, p, out_line, out_line_depth):
    up = Uploads(ctx)
    a, b = up.empty(p.n_lines) if out_line else None, up.empty((p.n_lines, N_DEPTH)) if out_line_depth else None
    ctx.call("sdx_line_adjoint_dev", N_DEPTH, p.n_nu, up(p.nus), 0, p.n_nu, p.n_lines, up(p.line_nus), up(p.doppler), up(p.gammas), p.gamma_cols, up(p.alphas),
             up(p.weight), p.n_nu, a.ptr if a else None, b.ptr if b else None)
    return {k: v.numpy() for k, v in (("out_line", a), ("out_line_depth", b)) if v is not None}


def observe_host(ctx, p, reference):
    out = nan(p.n_pix)
    ctx.call("sdx_observe_f64", p.n_nu, P(p.lam), P(p.flux), P(p.reference) if reference else None, p.n_pix, P(p.edges), P(p.sigma), DOPPLER, P(out))
    return dict(out=out)


def observe_dev(ctx, p, reference):
    up = Uploads(ctx)
    out = up.empty(p.n_pix)
    if p.n_pix:
        ctx.call("sdx_observe_dev", p.n_nu, up(p.lam), up(p.flux), up(p.reference) if reference else None, p.n_pix, up(p.edges), up(p.sigma),
                 up(np.array([DOPPLER])), out.ptr)
    return dict(out=out.numpy() if p.n_pix else nan(0))


def observe_adjoint_host(ctx, p, reference, nus, w_reference):
    wf, wr = nan(p.n_nu), nan(p.n_nu) if w_reference else None
    ctx.call("sdx_observe_adjoint_f64", p.n_nu, P(p.lam), P(p.flux), P(p.reference) if reference else None, p.n_pix, P(p.edges), P(p.sigma), DOPPLER,
             P(p.pixel_weight), P(p.nus) if nus else None, P(wf), P(wr))
    return dict(w_flux=wf, **({"w_reference": wr} if w_reference else {}))


def observe_adjoint_dev(ctx, p, reference, nus, w_reference):
    up = Uploads(ctx)
    wf, wr = up.empty(p.n_nu), up.empty(p.n_nu) if w_reference else None
    ctx.call("sdx_observe_adjoint_dev", p.n_nu, up(p.lam), up(p.flux) if reference else None, up(p.reference) if reference else None, p.n_pix, up(p.edges),
             up(p.sigma) if p.n_pix else None, up(np.array([DOPPLER])), up(p.pixel_weight) if p.n_pix else None, up(p.nus) if nus else None, wf.ptr,
             wr.ptr if w_reference else None)
    return dict(w_flux=wf.numpy(), **({"w_reference": wr.numpy()} if w_reference else {}))


CONTINUUM_OUTPUTS = ("file", "bf", "ff", "rayleigh", "electron", "total")


def continuum_host(ctx, p, outputs):
    nus = p.nus.copy()  # (in and out: the Rayleigh source clips it in place)
    out = {k: nan(N_DEPTH, p.n_nu) for k in outputs}
    c = continuum_struct(p, P)
    ctx.call("sdx_continuum_f64", N_DEPTH, p.n_nu, P(nus), C.byref(c), *(P(out.get(k)) for k in CONTINUUM_OUTPUTS))
    return dict(out, nus=nus)


def synthesize_host(ctx, p, line, total, evaluations, without=()):
    F, a, b = nan(N_DEPTH, p.n_nu), nan(N_DEPTH, p.n_nu) if line else None, nan(N_DEPTH, p.n_nu) if total else None
    ev = C.c_int64(-1)
    c = continuum_struct(p, P, without=("temperature",) + tuple(without))
    ctx.call("sdx_synthesize_f64", N_DEPTH, p.n_nu, P(p.nus), p.n_lines, P(p.line_nus), P(p.doppler), P(p.gammas), p.gamma_cols, P(p.alphas), C.byref(c), N_THETA,
             P(p.t), P(p.ray), P(p.w), P(a), P(b), P(F), C.cast(C.byref(ev), C.c_void_p) if evaluations else None)
    got = {k: v for k, v in (("F_nu", F), ("alpha_line", a), ("total_alphas", b)) if v is not None}
    return dict(got, **({"evaluations": np.int64(ev.value)} if evaluations else {}))


def synthesize_dev(ctx, p, line, total, evaluations, without=()):
    up = Uploads(ctx)
    F, a, b = up.empty((N_DEPTH, p.n_nu)), up.empty((N_DEPTH, p.n_nu)) if line else None, up.empty((N_DEPTH, p.n_nu)) if total else None
    ev = up.empty(1, np.int64)
    t = up(p.t)
    c = continuum_struct(p, up, without=("temperature",) + tuple(without))
    c.temperature = t  # (the host entry points it at the rays' temperatures)
    ctx.call("sdx_synthesize_dev", N_DEPTH, p.n_nu, up(p.nus), 0, p.n_nu, p.n_lines, up(p.line_nus), up(p.doppler), up(p.gammas), p.gamma_cols, up(p.alphas),
             C.byref(c), N_THETA, t, up(p.ray), up(p.w), a.ptr if a else None, b.ptr if b else None, F.ptr, p.n_nu, ev.ptr if evaluations else None)
    got = {k: v.numpy() for k, v in (("F_nu", F), ("alpha_line", a), ("total_alphas", b)) if v is not None}
    return dict(got, **({"evaluations": ev.numpy()[0]} if evaluations else {}))


ENTRIES = dict(line_opacity=(line_opacity_host, line_opacity_dev), raytrace=(raytrace_host, raytrace_dev), contribution=(contribution_host, contribution_dev),
               response=(response_host, response_dev), line_adjoint=(line_adjoint_host, line_adjoint_dev), observe=(observe_host, observe_dev),
               observe_adjoint=(observe_adjoint_host, observe_adjoint_dev), continuum=(continuum_host, None), synthesize=(synthesize_host, synthesize_dev))

RAYLEIGH = ("ray_n_h", "ray_n_he", "ray_n_h2")
# (entry, (n_nu, n_lines, n_pix), arguments): the nine entries interleaved, sizes up and down, every optional row absent and present
SEQUENCE = [
    ("line_opacity", (400, 7, 0), dict()),
    ("observe", (33, 0, 5), dict(reference=False)),
    ("line_opacity", (400, 7, 0), dict(empty_grid=True)),  # n_nu = 0 between two calls that stage: returns 0, reports 0 evaluations
    ("line_opacity", (33, 7, 0), dict()),
    ("raytrace", (400, 0, 0), dict(i_nus=True)),
    ("contribution", (33, 0, 0), dict(source=False)),
    ("response", (400, 0, 0), dict(source=True, r_alpha=True, r_source=True)),
    ("line_adjoint", (33, 7, 0), dict(out_line=True, out_line_depth=True)),
    ("continuum", (400, 0, 0), dict(outputs=CONTINUUM_OUTPUTS)),
    ("observe_adjoint", (33, 0, 5), dict(reference=True, nus=True, w_reference=True)),
    ("synthesize", (400, 7, 0), dict(line=True, total=True, evaluations=True)),
    ("raytrace", (33, 0, 0), dict(i_nus=False)),
    ("contribution", (400, 0, 0), dict(source=True)),
    ("response", (33, 0, 0), dict(source=False, r_alpha=True, r_source=False)),
    ("response", (400, 0, 0), dict(source=True, r_alpha=False, r_source=True)),
    ("line_adjoint", (400, 7, 0), dict(out_line=True, out_line_depth=False)),
    ("line_adjoint", (33, 7, 0), dict(out_line=False, out_line_depth=True)),
    *[("continuum", (33 if k % 2 else 400, 0, 0), dict(outputs=(name,))) for k, name in enumerate(CONTINUUM_OUTPUTS)],
    ("observe", (400, 0, 5), dict(reference=True)),
    ("observe", (33, 0, 0), dict(reference=False)),
    ("observe_adjoint", (400, 0, 0), dict(reference=False, nus=False, w_reference=False)),
    ("synthesize", (33, 0, 0), dict(line=False, total=False, evaluations=False)),
    ("observe_adjoint", (400, 0, 5), dict(reference=False, nus=True, w_reference=False)),
    ("line_opacity", (400, 0, 0), dict()),
    ("observe_adjoint", (33, 0, 5), dict(reference=True, nus=False, w_reference=False)),
    ("synthesize", (33, 7, 0), dict(line=False, total=True, evaluations=False, without=RAYLEIGH)),
    ("synthesize", (400, 0, 0), dict(line=True, total=False, evaluations=True, without=("electron_density",))),
    ("line_opacity", (400, 7, 0), dict()),
]


def run_sequence(ctx):
    return [ENTRIES[name][0](ctx, problem(*shape), **kw) for name, shape, kw in SEQUENCE]


def same(a, b):
    """the same keys, and every array the same bytes (which np.array_equal follows from; NaN sentinels of unrequested cells included)"""
    assert a.keys() == b.keys()
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k], equal_nan=True)
               and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.fixture(scope="module")
def shared():
    """the sequence on one fresh context"""
    ctx = _lib.Context()
    out = run_sequence(ctx)
    ctx.close()
    return out


def test_one_arena_many_calls(shared, ctx):
    for (name, shape, kw), got in zip(SEQUENCE, shared):
        what = (name, shape, kw)
        host, dev = ENTRIES[name]
        own = _lib.Context()
        alone = host(own, problem(*shape), **kw)
        own.close()
        assert same(got, alone), what
        assert not any(np.isnan(np.asarray(v, dtype=np.float64)).any() for v in got.values()), what  # (every requested cell was written)
        if dev is not None:
            assert same(got, dev(ctx, problem(*shape), **kw)), what
    assert shared[2]["evaluations"] == 0 and shared[2]["out"].size == 0
    assert same(shared[0], shared[-1]) and shared[0]["evaluations"] > 0


# ---- the same in a child process: another staging mode (read once per process), the loop-back group -------------------------------------
def sharded(p, devices, shard_begin):
    """sdx_synthesize_sharded_f64 with explicit shards on a loop-back group of `devices`"""
    from stardis_amd.group import DeviceGroup

    grp = DeviceGroup(devices=devices)
    F, a, b, flux = nan(N_DEPTH, p.n_nu), nan(N_DEPTH, p.n_nu), nan(N_DEPTH, p.n_nu), nan(p.n_nu)
    ev = C.c_int64(-1)
    begin = np.array(shard_begin, dtype=np.int64)
    c = continuum_struct(p, P, without=("temperature",))
    _lib.check(grp.lib.sdx_synthesize_sharded_f64(grp.handle, N_DEPTH, p.n_nu, P(p.nus), p.n_lines, P(p.line_nus), P(p.doppler), P(p.gammas), p.gamma_cols, P(p.alphas),
                                                  C.byref(c), N_THETA, P(p.t), P(p.ray), P(p.w), P(begin), P(a), P(b), P(F), P(flux),
                                                  C.cast(C.byref(ev), C.c_void_p)))
    assert grp.last_gather()["backend"] == "loopback-test-hook"
    grp.close()
    return dict(F_nu=F, alpha_line=a, total_alphas=b, evaluations=np.int64(ev.value), emergent_flux=flux)


SHARDS = (([0], (0, 33)), ([0, 0], (0, 7, 33)))  # one rank with explicit shard_begin; an unequal two-way split on the same device


def child_main(path, sequence):
    arrays = {}
    if sequence:
        ctx = _lib.Context()
        arrays = {f"{i}.{k}": v for i, got in enumerate(run_sequence(ctx)) for k, v in got.items()}
        ctx.close()
    for j, (devices, begin) in enumerate(SHARDS):
        arrays.update({f"shard{j}.{k}": v for k, v in sharded(problem(33, 7, 0), devices, begin).items()})
    np.savez(path, **arrays)


def child(tmp_path, sequence, **env):
    """-> the arrays of child_main in a fresh process under SDX_EXPERIMENT=1, the loop-back group and `env`"""
    path = str(tmp_path / "child.npz")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\nfrom test_gpu_host_entries import child_main\nchild_main({path!r}, {sequence!r})\n"
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SDX_")}
    proc = subprocess.run([sys.executable, "-c", code], env=dict(clean, SDX_EXPERIMENT="1", SDX_GROUP_LOOPBACK="1", **env), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def check_shards(arrays, ctx):
    whole = synthesize_host(ctx, problem(33, 7, 0), line=True, total=True, evaluations=True)
    for j in range(len(SHARDS)):
        got = {k[len(f"shard{j}."):]: v for k, v in arrays.items() if k.startswith(f"shard{j}.")}
        assert np.array_equal(got.pop("emergent_flux"), whole["F_nu"][-1]), SHARDS[j]
        assert same(got, whole), SHARDS[j]


def test_without_pinned_staging(shared, ctx, tmp_path):
    arrays = child(tmp_path, True, SDX_NO_PINNED_STAGING="1")
    for i, want in enumerate(shared):
        got = {k[len(f"{i}."):]: v for k, v in arrays.items() if k.startswith(f"{i}.")}
        assert same(got, want), SEQUENCE[i]
    check_shards(arrays, ctx)  # (the shard's columns by hipMemcpy2DAsync)


def test_shard_columns(ctx, tmp_path):
    check_shards(child(tmp_path, False), ctx)
