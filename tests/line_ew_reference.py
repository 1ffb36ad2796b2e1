"""Isolated-line equivalent widths restated on the CPU from the reference's own terms (no test in here; tests/test_line_ew_cpu.py checks
the restatement, tests/test_gpu_line_ew.py judges the kernels by it).

For line l of a model of tests/line_adjoint_truth.py and a strength factor s, the line's plane is oracle.calc_alan_entries of the
one-line list with alphas * s: the reference's window with the terms of voigt.py inside and zeros outside.  F of background + plane and
F_B of the background come from oracle.raytrace (fp64) and from formal_solution_truth.truth (80-bit); r = (F_B - F) / F_B, the union U of
the windows over depth, the node weights h on lambda in Angstrom and W = sum h r, depth = max r are formed in the matching precision, as
include/stardis_hip.h defines them.

The judge: |W - W_80| <= 2 formal_solution_truth.bound(d, n_depth) span + 2 OPACITY_RTOL |W_80|, with d the fp64 oracle's largest flux
distance (formal_solution_truth.distance) over the item's columns, for F and F_B, and span = |x_hi - x_lo| of the union (for a shard's part of
it: the sum of the node weights of the points summed, which for the whole union is that span).  r
carries the error of two fluxes, each held to the formal solution's own criterion; a relative error in the line's terms moves W by about
that fraction of itself; the factor 2 is margin for windows whose truncation makes the curve of growth locally steeper than 1.  depth:
the same without the factor span."""
import functools
import types

import numpy as np

import formal_solution_truth as T
import line_adjoint_truth as A
import oracle
from stardis_amd import constants as K, synth

L = np.longdouble
OPACITY_RTOL = A.OPACITY_RTOL
SCALES = (0.1, 1.0, 10.0)


@functools.lru_cache(maxsize=None)
def model(name):
    """a model of tests/line_adjoint_truth.py by its name, or "deep<N>": N depth points interpolated through the solar structure (more
    than it has rows: no two points coincide), 64 frequencies, 3 lines — the shapes around the depth at which EwColumns lowers the
    points per wave; or "edge" """
    if name == "edge":  # two lines of `small` moved beyond the ends of the grid: centre index 0 and n_nu, the windows reach in
        m = A.model("small")
        lines = {k: np.ascontiguousarray(v[[31, 12]]) for k, v in m.lines.items()}
        lines["line_nus"] = np.array([m.nus[-1] * (1 - 2e-6), m.nus[0] * (1 + 2e-6)])
        return types.SimpleNamespace(name=name, n_depth=m.n_depth, n_nu=m.n_nu, n_lines=2, atm=m.atm, nus=m.nus, lines=lines)
    if not name.startswith("deep"):
        return A.model(name)
    n_depth = int(name[4:])
    sun = synth.solar_atmosphere()
    rows = np.arange(sun["temperatures"].size, dtype=np.float64)
    pos = np.linspace(0.0, rows[-1], n_depth)
    atm = {k: (np.interp(pos, rows, v) if isinstance(v, np.ndarray) and v.size == rows.size else v) for k, v in sun.items()}
    nus = synth.tracing_grid(6560.0, 6562.0, n_override=64)
    lines = synth.synth_lines(nus, atm, 3, seed=41, mix=(0.3, 0.5, 0.2))
    return types.SimpleNamespace(name=name, n_depth=n_depth, n_nu=64, n_lines=3, atm=atm, nus=nus, lines=lines)


def background(m):
    """an opacity plane that needs no continuum state: 1e-8 (T / T_min)^6 (1 + 0.05 sin 3 lambda); it puts the lists' lines between
    depths of 1e-11 and 0.6"""
    t = m.atm["temperatures"]
    lam = K.nu_to_angstrom(m.nus)
    return np.ascontiguousarray(1e-8 * ((t / t.min()) ** 6)[:, None] * (1.0 + 0.05 * np.sin(3.0 * lam))[None, :])


@functools.lru_cache(maxsize=None)
def setup(name, n_theta):
    """-> namespace: the model, its background, the geometry (ray distances |diff r| of the picked depths: the models sub-sample the
    atmosphere, atm["dist"] keeps all 55 entries), lambda, and the background's fluxes in both precisions, computed once"""
    m = model(name)
    B = background(m)
    temps = np.ascontiguousarray(m.atm["temperatures"])
    dist = np.abs(np.diff(m.atm["r"]))
    thetas, weights = synth.thetas_and_weights(n_theta)
    ray = np.ascontiguousarray(dist.reshape(-1, 1) / np.cos(thetas))
    x = K.nu_to_angstrom(m.nus)
    with np.errstate(all="ignore"):
        FB64 = oracle.raytrace(m.nus, temps, dist, thetas, weights, B)[0]
        FB80 = T.truth(m.nus, temps, dist, thetas, weights, B)[0]
    for a in (B, FB64, FB80):
        a.setflags(write=False)
    return types.SimpleNamespace(m=m, B=B, temps=temps, dist=dist, thetas=thetas, weights=weights, ray=ray, x=x, FB64=FB64, FB80=FB80, n_theta=n_theta)


def union(m, l, s):
    """-> (ulo, uhi): the union over depth of the reference's windows of line l with alphas * s (an interval)"""
    Ls = m.lines
    g = Ls["gammas"]
    w = [oracle.window(m.nus, Ls["line_nus"][l], g[l, d if g.shape[1] > 1 else 0], Ls["doppler_widths"][l, d], Ls["alphas"][l, d] * s) for d in range(m.n_depth)]
    return min(lo for lo, _ in w), max(hi for _, hi in w)


def node_weights(x, ulo, uhi, cols, dtype):
    x = np.asarray(x).astype(dtype)
    right = np.where(cols + 1 < uhi, np.abs(x[np.minimum(cols + 1, x.size - 1)] - x[cols]), dtype(0))
    left = np.where(cols - 1 >= ulo, np.abs(x[cols] - x[np.maximum(cols - 1, 0)]), dtype(0))
    return (right + left) * dtype(0.5)


@functools.lru_cache(maxsize=None)
def item(name, n_theta, l, s):
    """one (line, strength factor) on the whole grid -> namespace(ulo, uhi, r64, r80 over [ulo, uhi), d): computed once"""
    S = setup(name, n_theta)
    m = S.m
    Ls = m.lines
    sel = slice(l, l + 1)
    plane = oracle.calc_alan_entries(m.n_depth, m.nus, Ls["line_nus"][sel], Ls["doppler_widths"][sel], Ls["gammas"][sel], Ls["alphas"][sel] * s)
    ulo, uhi = union(m, l, s)
    assert not plane[:, :ulo].any() and not plane[:, uhi:].any()
    c = slice(ulo, uhi)
    Acols = np.ascontiguousarray(S.B[:, c] + plane[:, c])
    nus = np.ascontiguousarray(m.nus[c])
    with np.errstate(all="ignore"):
        F64 = oracle.raytrace(nus, S.temps, S.dist, S.thetas, S.weights, Acols)[0]
        F80 = T.truth(nus, S.temps, S.dist, S.thetas, S.weights, Acols)[0]
    FB64, FB80 = S.FB64[:, c], S.FB80[:, c]
    d = max(float(T.distance(F64, F80, np.isfinite(F64)).max()), float(T.distance(FB64, FB80, np.isfinite(FB64)).max()))
    r64 = (FB64[-1] - F64[-1]) / FB64[-1]
    r80 = (FB80[-1] - F80[-1]) / FB80[-1]
    return types.SimpleNamespace(ulo=ulo, uhi=uhi, r64=r64, r80=r80, d=d)


def restated(name, n_theta, lines=None, scales=SCALES, shard=None):
    """-> namespace of (n_sel, K) arrays: W64, depth64 (float64), W80, depth80 (longdouble), bound_W, bound_depth (the judge), terms
    (sum |h r|, fp64) and points (the number of points summed), over the columns of `shard` = (begin, count) (default: all)"""
    S = setup(name, n_theta)
    m = S.m
    lines = list(range(m.n_lines)) if lines is None else [int(v) for v in lines]
    b, n = (0, m.n_nu) if shard is None else shard
    shape = (len(lines), len(scales))
    out = types.SimpleNamespace(W64=np.zeros(shape), depth64=np.zeros(shape), W80=np.zeros(shape, dtype=L), depth80=np.zeros(shape, dtype=L),
                                bound_W=np.zeros(shape), bound_depth=np.zeros(shape), terms=np.zeros(shape), points=np.zeros(shape, dtype=np.int64))
    for j, l in enumerate(lines):
        for k, s in enumerate(scales):
            it = item(name, n_theta, l, float(s))
            lo, hi = max(it.ulo, b), min(it.uhi, b + n)
            if hi <= lo:
                continue
            cols = np.arange(lo, hi)
            r64, r80 = it.r64[lo - it.ulo:hi - it.ulo], it.r80[lo - it.ulo:hi - it.ulo]
            h64, h80 = node_weights(S.x, it.ulo, it.uhi, cols, np.float64), node_weights(S.x, it.ulo, it.uhi, cols, L)
            out.W64[j, k], out.depth64[j, k] = (h64 * r64).sum(), r64.max()
            out.W80[j, k], out.depth80[j, k] = (h80 * r80).sum(), r80.max()
            out.terms[j, k], out.points[j, k] = np.abs(h64 * r64).sum(), hi - lo
            # span = |x_hi - x_lo| of the union; of a shard's part of it, the sum of its node weights (the whole union's sum IS that span)
            span = abs(float(S.x[hi - 1] - S.x[lo])) if (lo, hi) == (it.ulo, it.uhi) else float(h64.sum())
            fb = T.bound(it.d, m.n_depth)
            out.bound_W[j, k] = 2 * fb * span + 2 * OPACITY_RTOL * abs(float(out.W80[j, k]))
            out.bound_depth[j, k] = 2 * fb + 2 * OPACITY_RTOL * abs(float(out.depth80[j, k]))
    return out


def judge(label, W, depth, ref):
    """print the worst distance over its bound, then assert the judge for W and depth (host arrays (n_sel, K))"""
    rW = np.abs(np.asarray(W).astype(L) - ref.W80).astype(np.float64) / ref.bound_W
    rD = np.abs(np.asarray(depth).astype(L) - ref.depth80).astype(np.float64) / ref.bound_depth
    print(f"{label}: worst |W - W_80| / bound {rW.max():.3e}, worst |depth - depth_80| / bound {rD.max():.3e}; "
          f"depths from {float(ref.depth80.min()):.2e} to {float(ref.depth80.max()):.2e}")
    assert np.isfinite(np.asarray(W)).all() and np.isfinite(np.asarray(depth)).all()
    assert (rW <= 1.0).all() and (rD <= 1.0).all(), (label, float(rW.max()), float(rD.max()))
    return float(rW.max()), float(rD.max())
