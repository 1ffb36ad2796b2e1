"""Array-level Python front-end of the C ABI: numpy (host) in, numpy out, all arithmetic on the GPU.

Each function names the reference callable it stands in for (paths relative to
stardis/radiation_field/).  These are what the reference-named modules under
stardis_amd/radiation_field/ call; they add no numerics of their own.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceArray, default_context, ptr_of

F8 = np.float64


def _host(a, dtype=F8):
    a = np.asarray(_lib.plain(a), dtype=dtype)
    return a if a.ndim == 0 else np.ascontiguousarray(a)  # ascontiguousarray would turn a scalar into shape (1,)


def _on_device(a):
    return isinstance(a, DeviceArray) or hasattr(a, "data_ptr")


def _dev(ctx, a, dtype=F8):
    """DeviceArray for a host array (uploads) or pass a DeviceArray / CUDA tensor through."""
    if a is None or _on_device(a):
        return a
    return ctx.upload(_host(a, dtype), dtype)


def _shape(a):
    """the shape of a host or device array as a tuple of ints"""
    return tuple(int(v) for v in (a.shape if hasattr(a, "shape") else np.shape(a)))


def _source_plane(source, shape):
    """a caller's source-function plane on the host, its shape checked (None stays None)"""
    if source is None:
        return None
    src = _host(source)
    if src.shape != shape:
        raise ValueError(f"source function must return shape {shape}, got {src.shape}")
    return src


# ------------------------------------------------------------------------------------------------ voigt.py
def faddeeva(z, ctx=None):
    """opacities/opacities_solvers/voigt.py:89-91"""
    ctx = ctx or default_context()
    zz = np.ascontiguousarray(np.asarray(z), dtype=np.complex128)
    d_z = ctx.upload(zz.view(F8).reshape(-1), F8)
    d_w = ctx.empty(zz.size * 2)
    ctx.call("sdx_faddeeva_dev", zz.size, d_z.ptr, d_w.ptr)
    out = d_w.numpy().view(np.complex128).reshape(zz.shape)
    return out if out.ndim else out[()]


def voigt_profile(delta_nu, doppler_width, gamma, ctx=None):
    """opacities/opacities_solvers/voigt.py:153-155"""
    ctx = ctx or default_context()
    a, b, c = np.broadcast_arrays(_host(delta_nu), _host(doppler_width), _host(gamma))
    if np.any(b == 0):
        raise ZeroDivisionError("float division by zero")  # voigt.py:148; reference test_voigt.py:130-148
    d = [ctx.upload(np.ascontiguousarray(x)) for x in (a, b, c)]
    out = ctx.empty(a.shape)
    ctx.call("sdx_voigt_profile_dev", a.size, d[0].ptr, d[1].ptr, d[2].ptr, out.ptr)
    r = out.numpy()
    return r if r.ndim else r[()]


def voigt_term(delta_nu, doppler_width, gamma, alpha=1.0, ctx=None, fp32=False):
    """alpha * voigt_profile(delta_nu, doppler_width, gamma) through the routine the LINE KERNELS evaluate (real part only,
    FMA arithmetic, one reciprocal per point; sdx_math.h voigt_term) instead of the reference-order element-wise one.
    The derived constants are formed exactly as the pre-pass forms them (voigt.py:148-149, base.py:627).
    fp32=True: the packed-fp32 routine the mixed_precision option uses for narrow windows (sdx_math.h voigt_add32)."""
    ctx = ctx or default_context()
    dnu, dw, g, a = (np.ascontiguousarray(v) for v in np.broadcast_arrays(_host(delta_nu), _host(doppler_width), _host(gamma), _host(alpha)))
    if np.any(dw == 0):
        raise ZeroDivisionError("float division by zero")
    sqrt_pi = np.float64(1.7724538509055159)
    inv = 1.0 / dw
    y = (g / (sqrt_pi * np.float64(np.pi))) / dw
    amp = a / (sqrt_pi * dw)
    d = [ctx.upload(v) for v in (dnu, inv, y, amp)]
    out = ctx.empty(dnu.shape)
    ctx.call("sdx_voigt_term_f32_dev" if fp32 else "sdx_voigt_term_dev", dnu.size, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out.ptr)
    r = out.numpy()
    return r if r.ndim else r[()]


def voigt_grad(delta_nu, doppler_width, gamma, alpha=1.0, ctx=None):
    """-> (K amp, K_x amp, K_y amp): voigt_term's value and its partial derivatives to x = delta_nu / doppler_width and to
    y = (gamma / (sqrt(pi) pi)) / doppler_width, K = Re w(x + i y), amp = alpha / (sqrt(pi) doppler_width) (voigt.py:148-149) — the
    derivative of the reference's formula in the Humlicek region it picks (voigt.py:39-84), through the routine the line-profile
    sensitivities evaluate (sdx_voigt_grad_dev; sdx_math.h voigt_grad_x)."""
    ctx = ctx or default_context()
    both = np.broadcast_arrays(_host(delta_nu), _host(doppler_width), _host(gamma), _host(alpha))
    shape = both[0].shape
    dnu, dw, g, a = (np.ascontiguousarray(v).reshape(-1) for v in both)
    if np.any(dw == 0):
        raise ZeroDivisionError("float division by zero")
    sqrt_pi = np.float64(1.7724538509055159)
    inv = 1.0 / dw
    y = (g / (sqrt_pi * np.float64(np.pi))) / dw
    amp = a / (sqrt_pi * dw)
    d = [ctx.upload(v) for v in (dnu, inv, y, amp)]
    out = [ctx.empty(dnu.shape) for _ in range(3)]
    ctx.call("sdx_voigt_grad_dev", dnu.size, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out[0].ptr, out[1].ptr, out[2].ptr)
    r = tuple(o.numpy().reshape(shape) for o in out)
    return r if shape else tuple(v[()] for v in r)


# ------------------------------------------------------------------------------------------------ line opacity
def _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas_array, sort=True):
    """The four line arrays as contiguous float64 in the kernels' shapes.  sort=True: stably sorted by frequency when they
    are not (the line-opacity kernels want an ascending list); sort=False leaves the caller's order alone (per-line outputs)."""
    ln = _host(line_nus).reshape(-1)
    nd = int(no_of_depth_points)
    dw = _host(doppler_widths).reshape(ln.size, nd)  # may arrive F-ordered from DataFrame.to_numpy() (base.py:403-407)
    al = _host(alphas_array).reshape(ln.size, nd)
    g = _host(gammas)
    g = g.reshape(ln.size, -1) if ln.size else g.reshape(0, 1)
    if g.shape[1] not in (1, nd):
        raise ValueError(f"gammas must have shape (n_lines, {nd}) or (n_lines, 1), got {g.shape}")
    if sort and ln.size > 1 and np.any(ln[1:] < ln[:-1]):
        # The reference treats every line independently (base.py:548-590), so any order is legal there; the kernels want
        # ascending frequency (what calc_alpha_line_at_nu hands over, :392-397).  A stable sort changes only the order of
        # the per-point sum, which differs from the reference's per-thread slabs anyway.
        order = np.argsort(ln, kind="stable")
        ln, dw, g, al = (np.ascontiguousarray(a[order]) for a in (ln, dw, g, al))
    return ln, dw, g, al


def calc_alan_entries(no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array,
                      return_evaluations=False, ctx=None):
    """opacities/opacities_solvers/base.py:487-592 through sdx_line_opacity_f64 (host buffers in and out)."""
    ctx = ctx or default_context()
    nus = _host(tracing_nus_values).reshape(-1)
    ln, dw, g, al = _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas_array)
    nd = int(no_of_depth_points)
    out = np.empty((nd, nus.size))
    ev = C.c_int64(0)
    _lib.check(
        ctx.lib.sdx_line_opacity_f64(
            ctx.handle, nd, nus.size, nus.ctypes.data, ln.size, ln.ctypes.data, dw.ctypes.data, g.ctypes.data,
            g.shape[1], al.ctypes.data, out.ctypes.data, C.byref(ev),
        )
    )
    return (out, ev.value) if return_evaluations else out


def line_windows(no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, ctx=None):
    """Window bounds [lower, upper) per (line, depth): opacities/opacities_solvers/base.py:556-575.  Row k belongs to line k
    of the caller's list whatever its order (the window rule is per line; sdx_line_windows_dev does not need a sorted list)."""
    ctx = ctx or default_context()
    nus = _host(tracing_nus_values).reshape(-1)
    ln, dw, g, al = _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas_array, sort=False)
    nd = int(no_of_depth_points)
    d = [ctx.upload(x) for x in (nus, ln, dw, g, al)]
    lo = ctx.empty((ln.size, nd), np.int32)
    hi = ctx.empty((ln.size, nd), np.int32)
    ctx.call("sdx_line_windows_dev", nd, nus.size, d[0].ptr, ln.size, d[1].ptr, d[2].ptr, d[3].ptr, g.shape[1], d[4].ptr,
             lo.ptr, hi.ptr)
    return lo.numpy(), hi.numpy()


def line_adjoint(no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, weight, per_depth=False,
                 ctx=None, device=False, shard=None):
    """The adjoint of calc_alan_entries (sdx_line_adjoint_dev): per line l, sum_d sum_i weight[d, i] * (the term line l adds to
    alpha_line_at_nu[d, i]) over the reference's window of (l, d) -> (n_lines,), or with per_depth=True the sums per depth point
    (n_lines, N_d).  Row k belongs to line k of the caller's list whatever its order.  weight: (N_d, N_nu) host array, DeviceArray or
    CUDA tensor; shard = (begin, count): only these columns of the global grid are summed and weight is (N_d, count) — shards add.
    device=True: a DeviceArray instead of a host array."""
    ctx, head, held, shape = _adjoint_inputs(ctx, no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, weight, per_depth, shard)
    out = ctx.empty(shape)
    ctx.call("sdx_line_adjoint_dev", *head, None if per_depth else out.ptr, out.ptr if per_depth else None)
    return out if device else out.numpy()


def _adjoint_inputs(ctx, no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, weight, per_depth, shard):
    """What line_adjoint and line_param_adjoint share: the grid, the tables, the shard and the weight checked and on the device ->
    (the context, the arguments of either entry up to weight_ld, the device arrays they point into, the shape of an output)."""
    nus = _host(tracing_nus_values).reshape(-1)
    ln, dw, g, al = _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas_array, sort=False)
    nd = int(no_of_depth_points)
    begin, count = (0, nus.size) if shard is None else (int(v) for v in shard)
    if begin < 0 or count < 0 or begin + count > nus.size:
        raise ValueError(f"shard {(begin, count)} lies outside the grid of {nus.size} frequencies")
    shape = tuple(int(v) for v in (weight.shape if hasattr(weight, "shape") else np.shape(weight)))
    if shape != (nd, count):
        raise ValueError(f"weight must have shape {(nd, count)}, got {shape}")
    ctx = ctx or default_context()
    d_w = _dev(ctx, weight)
    d = [ctx.upload(x) for x in (nus, ln, dw, g, al)]
    head = (nd, nus.size, d[0].ptr, begin, count, ln.size, d[1].ptr, d[2].ptr, d[3].ptr, g.shape[1], d[4].ptr, ptr_of(d_w), count)
    return ctx, head, d + [d_w], ((ln.size, nd) if per_depth else (ln.size,))


def line_selection(n_lines, lines=None, ln_strength=None):
    """The selection of equivalent_widths as host arrays -> (line_index int64 (n_sel,) or None for every line, scale (n_sel, K)):
    lines None (all) or indices into the caller's list, repeats allowed, ValueError for one outside [0, n_lines); ln_strength None
    (no change), a scalar, (K,) or (n_sel, K): the natural logarithm of the factor on the line's strength, exponentiated here."""
    n_lines = int(n_lines)
    index = None
    if lines is not None:
        index = np.ascontiguousarray(np.asarray(lines).reshape(-1), dtype=np.int64)
        if index.size and (index.min() < 0 or index.max() >= n_lines):
            raise ValueError(f"lines must index the list of {n_lines} lines, got an index outside [0, {n_lines})")
    n_sel = n_lines if index is None else index.size
    ln_s = np.zeros((1,)) if ln_strength is None else _host(ln_strength)
    if ln_s.ndim == 0:
        ln_s = ln_s.reshape(1)
    if ln_s.ndim == 1:
        ln_s = np.broadcast_to(ln_s[None, :], (n_sel, ln_s.size))
    if ln_s.ndim != 2 or ln_s.shape[0] != n_sel or ln_s.shape[1] < 1:
        raise ValueError(f"ln_strength must be a scalar, (K,) or ({n_sel}, K) with K >= 1, got shape {ln_s.shape}")
    return index, np.ascontiguousarray(np.exp(ln_s))


def equivalent_widths(no_of_depth_points, nus, line_nus, doppler_widths, gammas, alphas, background, temperatures, ray_distances,
                      theta_weights, x=None, lines=None, ln_strength=None, shard=None, ctx=None, device=False):
    """Isolated-line equivalent widths and line depths (sdx_line_equivalent_widths_dev; the definition stands in include/stardis_hip.h)
    -> (W, depth), each (n_sel, K): for every selected line and strength factor exp(ln_strength), the trapezoid integral over the
    points the line reaches of r = (F_B - F) / F_B and the largest r — F the emergent flux of the plane-parallel formal solution of
    background + this line alone, F_B that of the background.  Row j belongs to lines[j] of the caller's list, whatever its order.
    background (N_d, count): host array, DeviceArray or CUDA tensor; ray_distances (N_d - 1, N_theta) as raytrace forms them
    (dist / cos(theta)); x: the abscissa of the integral on the whole grid, None: lambda in Angstrom (W in Angstrom).  lines: None
    (all) or indices, checked here before anything is uploaded; ln_strength: None, a scalar, (K,) or (n_sel, K).  shard = (begin,
    count): only these columns of the global grid — W of the shards adds, depth combines by max.  device=True: DeviceArrays."""
    nus = _host(nus).reshape(-1)
    ln, dw, g, al = _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas, sort=False)
    nd = int(no_of_depth_points)
    begin, count = (0, nus.size) if shard is None else (int(v) for v in shard)
    if begin < 0 or count < 0 or begin + count > nus.size:
        raise ValueError(f"shard {(begin, count)} lies outside the grid of {nus.size} frequencies")
    shape = tuple(int(v) for v in (background.shape if hasattr(background, "shape") else np.shape(background)))
    if shape != (nd, count):
        raise ValueError(f"background must have shape {(nd, count)}, got {shape}")
    index, scale = line_selection(ln.size, lines, ln_strength)
    t = _host(temperatures).reshape(-1)
    w = _host(theta_weights).reshape(-1)
    ray = _host(ray_distances)
    if t.size != nd or ray.shape != (nd - 1, w.size):
        raise ValueError(f"temperatures must hold {nd} values and ray_distances have shape {(nd - 1, w.size)}, got {t.size} and {ray.shape}")
    from . import constants as K

    xs = K.nu_to_angstrom(nus) if x is None else _host(x).reshape(-1)
    if xs.size != nus.size:
        raise ValueError(f"x must hold one value per frequency ({nus.size}), got {xs.size}")
    ctx = ctx or default_context()
    d_b = _dev(ctx, background)
    d = [ctx.upload(v) for v in (nus, xs, ln, dw, g, al, scale, t, ray, w)]
    d_index = None if index is None else ctx.upload(index, np.int64)
    n_sel, k = scale.shape
    out_w, out_d = ctx.empty((n_sel, k)), ctx.empty((n_sel, k))
    ctx.call("sdx_line_equivalent_widths_dev", nd, nus.size, d[0].ptr, begin, count, d[1].ptr, ln.size, d[2].ptr, d[3].ptr, d[4].ptr, g.shape[1],
             d[5].ptr, n_sel, ptr_of(d_index), k, d[6].ptr, ptr_of(d_b), count, w.size, d[7].ptr, d[8].ptr, d[9].ptr, out_w.ptr, out_d.ptr)
    return (out_w, out_d) if device else (out_w.numpy(), out_d.numpy())


LINE_PARAMS = ("damping", "doppler", "centre")


def line_param_adjoint(no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, weight, per_depth=False,
                       ctx=None, device=False, shard=None, wrt=LINE_PARAMS):
    """The line-profile twin of line_adjoint (sdx_line_param_adjoint_dev) -> dict with the keys "damping", "doppler", "centre" (those
    named in wrt): the derivative of  sum_d sum_i weight[d, i] alpha_line_at_nu[d, i]  with respect to ln gamma, ln doppler_width and
    the rest frequency (per Hz) of every line, at fixed windows and fixed Humlicek regions -> (n_lines,) each, or with per_depth=True
    with respect to the value at each depth point (n_lines, N_d).  Arguments as for line_adjoint."""
    wrt = tuple(wrt)
    if not wrt or any(k not in LINE_PARAMS for k in wrt):
        raise ValueError(f"wrt must name some of {LINE_PARAMS}, got {wrt}")
    ctx, head, held, shape = _adjoint_inputs(ctx, no_of_depth_points, tracing_nus_values, line_nus, doppler_widths, gammas, alphas_array, weight, per_depth, shard)
    out = {k: ctx.empty(shape) for k in wrt}
    ptrs = [ptr_of(out.get(k)) for k in LINE_PARAMS]
    none = [None] * 3
    ctx.call("sdx_line_param_adjoint_dev", *head, *(none + ptrs if per_depth else ptrs + none))
    return out if device else {k: v.numpy() for k, v in out.items()}


LINE_DIRECTIONS = ("strength", "damping", "doppler", "centre")


def line_directions(n_lines, no_of_depth_points, strength=None, damping=None, doppler=None, centre=None):
    """The directions of line_tangent as host arrays -> (list of four (n_lines, cols) arrays or None, cols): each direction None, a
    scalar, (n_lines,) or (n_lines, N_d); cols is N_d when any of them is per depth, else 1."""
    n_lines, nd = int(n_lines), int(no_of_depth_points)
    given = []
    for name, v in zip(LINE_DIRECTIONS, (strength, damping, doppler, centre)):
        if v is None:
            given.append(None)
            continue
        v = _host(v)
        if v.ndim == 0:
            v = np.full((n_lines, 1), float(v))
        elif v.shape == (n_lines,):
            v = v.reshape(n_lines, 1)
        elif v.shape != (n_lines, nd):
            raise ValueError(f"direction {name!r} must be a scalar or have shape {(n_lines,)} or {(n_lines, nd)}, got {v.shape}")
        given.append(v)
    if all(v is None for v in given):
        raise ValueError(f"line_tangent needs a direction: one of {LINE_DIRECTIONS}")
    cols = nd if any(v is not None and v.shape[1] == nd for v in given) else 1  # ((n_lines, 1) with N_d = 1 is both)
    return [None if v is None else np.ascontiguousarray(np.broadcast_to(v, (n_lines, cols))) for v in given], cols


def line_tangent(no_of_depth_points, nus, line_nus, doppler_widths, gammas, alphas, strength=None, damping=None, doppler=None, centre=None,
                 ctx=None, device=False, shard=None):
    """The tangent of calc_alan_entries (sdx_line_tangent_dev), the transpose of line_adjoint and line_param_adjoint: the plane
    (N_d, N_nu) by which alpha_line_at_nu moves, at fixed windows and fixed Humlicek regions, when every line moves along
    strength = d ln alpha, damping = d ln gamma, doppler = d ln doppler_width and centre = d line_nu (Hz) — each None (zero), a scalar,
    (n_lines,) or (n_lines, N_d) in the order of the caller's list, which may be any (sorted here as for calc_alan_entries, the
    directions with it).  A direction may also be a DeviceArray or CUDA tensor of shape (n_lines,), (n_lines, 1) or (n_lines, N_d): it is
    read where it lies, so the list must then be ascending and every direction of the call have that many columns.
    shard = (begin, count): only these columns, bit for bit those of the whole grid.  device=True: a DeviceArray."""
    nus = _host(nus).reshape(-1)
    ln, dw, g, al = _line_inputs(no_of_depth_points, line_nus, doppler_widths, gammas, alphas, sort=False)
    nd = int(no_of_depth_points)
    given = dict(zip(LINE_DIRECTIONS, (strength, damping, doppler, centre)))
    resident = {k: v for k, v in given.items() if isinstance(v, DeviceArray) or hasattr(v, "data_ptr")}
    unsorted = ln.size > 1 and bool(np.any(ln[1:] < ln[:-1]))
    if resident:
        shapes = [tuple(int(s) for s in v.shape) for v in resident.values()]
        widths = {1 if s == (ln.size,) else (s[1] if len(s) == 2 and s[0] == ln.size and s[1] in (1, nd) else None) for s in shapes}
        if None in widths or len(widths) != 1:
            raise ValueError(f"directions on the device must share one width: {(ln.size,)}, {(ln.size, 1)} or {(ln.size, nd)}, got {shapes}")
        if unsorted:
            raise ValueError("directions on the device are read where they lie: the line list must be ascending in frequency")
        cols = widths.pop()
        on_host = {k: v for k, v in given.items() if k not in resident and v is not None}
        dirs = [None] * 4
        if on_host:
            dirs, host_cols = line_directions(ln.size, nd, **on_host)
            if host_cols != cols and not (host_cols == 1 and cols == nd):
                raise ValueError(f"direction on the host with {host_cols} columns beside directions on the device with {cols}")
            dirs = [None if v is None else np.ascontiguousarray(np.broadcast_to(v, (ln.size, cols))) for v in dirs]
    else:
        dirs, cols = line_directions(ln.size, nd, strength, damping, doppler, centre)
    begin, count = (0, nus.size) if shard is None else (int(v) for v in shard)
    if begin < 0 or count < 0 or begin + count > nus.size:
        raise ValueError(f"shard {(begin, count)} lies outside the grid of {nus.size} frequencies")
    if unsorted:
        order = np.argsort(ln, kind="stable")
        ln, dw, g, al = (np.ascontiguousarray(a[order]) for a in (ln, dw, g, al))
        dirs = [None if v is None else np.ascontiguousarray(v[order]) for v in dirs]
    ctx = ctx or default_context()
    d = [ctx.upload(x) for x in (nus, ln, dw, g, al)]
    d_dirs = [resident[k] if k in resident else (None if v is None else ctx.upload(v)) for k, v in zip(LINE_DIRECTIONS, dirs)]
    out = ctx.empty((nd, count))
    ctx.call("sdx_line_tangent_dev", nd, nus.size, d[0].ptr, begin, count, ln.size, d[1].ptr, d[2].ptr, d[3].ptr, g.shape[1], d[4].ptr,
             *(ptr_of(v) for v in d_dirs), cols, out.ptr, count)
    return out if device else out.numpy()


# ------------------------------------------------------------------------------------------------ broadening
def _flags(linear_stark, quadratic_stark, van_der_waals, radiation):
    return (1 if linear_stark else 0) | (2 if quadratic_stark else 0) | (4 if van_der_waals else 0) | (8 if radiation else 0)


def calc_gamma(atomic_number, ion_number, ionization_energy, upper_level_energy, lower_level_energy, A_ul,
               electron_density, temperature, h_density, linear_stark=True, quadratic_stark=True, van_der_waals=True,
               radiation=True, ctx=None):
    """opacities/opacities_solvers/broadening.py:550-656; per-line inputs (N_l,) or (N_l,1), per-depth (N_d,)"""
    ctx = ctx or default_context()
    z = _host(atomic_number, np.int32).reshape(-1)
    ion = _host(ion_number, np.int32).reshape(-1)
    per_line = [_host(x).reshape(-1) for x in (ionization_energy, upper_level_energy, lower_level_energy, A_ul)]
    per_depth = [_host(x).reshape(-1) for x in (electron_density, temperature, h_density)]
    nd = per_depth[0].size
    d = [ctx.upload(z, np.int32), ctx.upload(ion, np.int32)] + [ctx.upload(x) for x in per_line + per_depth]
    out = ctx.empty((z.size, nd))
    ctx.call("sdx_calc_gamma_dev", z.size, nd, *[x.ptr for x in d],
             _flags(linear_stark, quadratic_stark, van_der_waals, radiation), out.ptr)
    return out.numpy()


def doppler_widths(line_nus, atomic_mass, temperature, microturbulence, ctx=None):
    """opacities/opacities_solvers/broadening.py:69-71 broadcast (N_l,1) x (N_d,) as at :723-730"""
    ctx = ctx or default_context()
    ln = _host(line_nus).reshape(-1)
    m = _host(atomic_mass).reshape(-1)
    t = _host(temperature).reshape(-1)
    d = [ctx.upload(x) for x in (ln, m, t)]
    out = ctx.empty((ln.size, t.size))
    ctx.call("sdx_doppler_widths_dev", ln.size, t.size, d[0].ptr, d[1].ptr, d[2].ptr, float(microturbulence), out.ptr)
    return out.numpy()


def calc_vald_gamma_arrays(atomic_number, ion_number, ionization_energy, upper_level_energy, lower_level_energy, A_ul,
                           stark, waals, atomic_mass, electron_density, temperature, h_density, linear_stark,
                           quadratic_stark, van_der_waals, radiation, ctx=None, halve=True):
    """opacities/opacities_solvers/broadening.py:1009-1085 on plain arrays (halve=False: the sum as :771-799 leaves it)"""
    ctx = ctx or default_context()
    z = _host(atomic_number, np.int32).reshape(-1)
    ion = _host(ion_number, np.int32).reshape(-1)
    per_line = [_host(x).reshape(-1) for x in (ionization_energy, upper_level_energy, lower_level_energy, A_ul, stark, waals, atomic_mass)]
    per_depth = [_host(x).reshape(-1) for x in (electron_density, temperature, h_density)]
    nd = per_depth[0].size
    d = [ctx.upload(z, np.int32), ctx.upload(ion, np.int32)] + [ctx.upload(x) for x in per_line + per_depth]
    out = ctx.empty((z.size, nd))
    ctx.call("sdx_calc_vald_gamma_dev", z.size, nd, *[x.ptr for x in d],
             _flags(linear_stark, quadratic_stark, van_der_waals, radiation) | (0 if halve else 16), out.ptr)
    return out.numpy()


def broadening_scalar(op, *operands, ctx=None):
    """The reference's element-wise broadening ufuncs (broadening.py:69-71,140-146,232-234,346-360,476-490)."""
    ctx = ctx or default_context()
    arrs = np.broadcast_arrays(*[_host(x) for x in operands])
    shape = arrs[0].shape
    d = [ctx.upload(np.ascontiguousarray(a)) for a in arrs]
    while len(d) < 5:
        d.append(None)
    out = ctx.empty(shape)
    ctx.call("sdx_broadening_scalar_dev", int(op), int(np.prod(shape, dtype=np.int64)), *[ptr_of(x) for x in d], out.ptr)
    r = out.numpy()
    return r if r.ndim else r[()]


# ------------------------------------------------------------------------------------------------ continuum
def alpha_file_1d(lambdas, table_wavelength, table_sigma, density, ctx=None):
    """opacities/opacities_solvers/base.py:40-70 with util.py:94-103 (np.interp table, e.g. Hminus_bf)"""
    ctx = ctx or default_context()
    lam, x, y, n = (_host(a).reshape(-1) for a in (lambdas, table_wavelength, table_sigma, density))
    d = [ctx.upload(a) for a in (lam, x, y, n)]
    out = ctx.empty((n.size, lam.size))
    ctx.call("sdx_alpha_file_1d_dev", n.size, lam.size, d[0].ptr, x.size, d[1].ptr, d[2].ptr, d[3].ptr, out.ptr, lam.size)
    return out


def alpha_file_2d(sigma, density, ctx=None):
    """opacities/opacities_solvers/base.py:70 with a (N_d, N_nu) sigma (util.py:35-91); sigma may already be on the device"""
    ctx = ctx or default_context()
    d_s = sigma if isinstance(sigma, DeviceArray) else ctx.upload(_host(sigma))
    n = _host(density).reshape(-1)
    d_n = ctx.upload(n)
    out = ctx.empty(d_s.shape)
    ctx.call("sdx_alpha_file_2d_dev", d_s.shape[0], d_s.shape[1], d_s.ptr, d_s.shape[1], d_n.ptr, out.ptr, d_s.shape[1])
    return out


def upload_sigma_table(wave, axis2, cell_simplices, transform, simplex_values, ctx=None):
    """The table side of sigma_table_2d on the device, for callers that evaluate the same table again and again."""
    ctx = ctx or default_context()
    return tuple(ctx.upload(_host(x)) for x in (np.reshape(_host(wave), -1), np.reshape(_host(axis2), -1), transform, simplex_values)) + (
        ctx.upload(_host(cell_simplices, np.int32), np.int32),)


def sigma_table_2d(wave, axis2, cell_simplices, transform, simplex_values, lambdas, second, scale_kind=0, temperatures=None, ctx=None,
                   table_dev=None):
    """opacities/opacities_solvers/util.py:35-91: LinearNDInterpolator on the table's triangulation at the mesh
    (lambdas, second) -> (sigma DeviceArray (len(second), len(lambdas)), rows that contain an exact zero).
    table_dev: what upload_sigma_table returned for this table (skips five uploads)."""
    ctx = ctx or default_context()
    wave, axis2 = _host(wave).reshape(-1), _host(axis2).reshape(-1)
    lam, sec = _host(lambdas).reshape(-1), _host(second).reshape(-1)
    if table_dev is None:
        table_dev = upload_sigma_table(wave, axis2, cell_simplices, transform, simplex_values, ctx)
    d = list(table_dev[:4]) + [ctx.upload(lam), ctx.upload(sec)]
    d_cells = table_dev[4]
    d_t = ctx.upload(_host(temperatures).reshape(-1)) if temperatures is not None else None
    out = ctx.empty((sec.size, lam.size))
    zero = ctx.empty((sec.size,), np.int32)
    ctx.call("sdx_sigma_table_2d_dev", wave.size, d[0].ptr, axis2.size, d[1].ptr, d_cells.ptr, d[2].ptr, d[3].ptr, sec.size, lam.size,
             d[4].ptr, d[5].ptr, int(scale_kind), d_t.ptr if d_t is not None else None, out.ptr, lam.size, zero.ptr)
    return out, np.flatnonzero(zero.numpy())


def alpha_bf(tracing_nus, species_offsets, species_ion_number, cutoff_frequency, level_number_density, n_depth, ctx=None):
    """opacities/opacities_solvers/base.py:178-271"""
    ctx = ctx or default_context()
    nus = _host(tracing_nus).reshape(-1)
    off = _host(species_offsets, np.int32).reshape(-1)
    ion = _host(species_ion_number, np.int32).reshape(-1)
    cut = _host(cutoff_frequency).reshape(-1)
    ld = _host(level_number_density).reshape(cut.size, n_depth)
    d_nus = ctx.upload(nus)
    d = [ctx.upload(off, np.int32), ctx.upload(ion, np.int32), ctx.upload(cut), ctx.upload(ld)]
    out = ctx.empty((n_depth, nus.size))
    ctx.call("sdx_alpha_bf_dev", n_depth, nus.size, d_nus.ptr, ion.size, *[x.ptr for x in d], out.ptr, nus.size)
    return out


def alpha_ff(tracing_nus, temperature, species_ion_number, number_density, ctx=None):
    """opacities/opacities_solvers/base.py:274-317"""
    ctx = ctx or default_context()
    nus = _host(tracing_nus).reshape(-1)
    t = _host(temperature).reshape(-1)
    ion = _host(species_ion_number, np.int32).reshape(-1)
    n = _host(number_density).reshape(ion.size, t.size) if ion.size else np.zeros((0, t.size))
    d = [ctx.upload(nus), ctx.upload(t), ctx.upload(ion, np.int32), ctx.upload(n)]
    out = ctx.empty((t.size, nus.size))
    ctx.call("sdx_alpha_ff_dev", t.size, nus.size, d[0].ptr, d[1].ptr, ion.size, d[2].ptr, d[3].ptr, out.ptr, nus.size)
    return out


def alpha_rayleigh(tracing_nus_inout, n_depth, n_h=None, n_he=None, n_h2=None, ctx=None):
    """opacities/opacities_solvers/base.py:74-135; returns (alpha_dev, clipped_nus) — the caller writes the
    clipped frequencies back into its own array to reproduce the in-place mutation at :99"""
    ctx = ctx or default_context()
    nus = _host(tracing_nus_inout).reshape(-1)
    d_nus = ctx.upload(nus)
    dens = [None if a is None else ctx.upload(_host(a).reshape(-1)) for a in (n_h, n_he, n_h2)]
    out = ctx.empty((n_depth, nus.size))
    ctx.call("sdx_alpha_rayleigh_dev", n_depth, nus.size, d_nus.ptr, *[ptr_of(x) for x in dens], out.ptr, nus.size)
    return out, d_nus.numpy()


def alpha_electron(n_nu, electron_density, ctx=None):
    """opacities/opacities_solvers/base.py:139-174"""
    ctx = ctx or default_context()
    ne = _host(electron_density).reshape(-1)
    d = ctx.upload(ne)
    out = ctx.empty((ne.size, int(n_nu)))
    ctx.call("sdx_alpha_electron_dev", ne.size, int(n_nu), d.ptr, out.ptr, int(n_nu))
    return out


def accumulate(total_dev, src_dev, ctx=None):
    """opacities/base.py:24-28: total += src, both (N_d, N_nu) device arrays"""
    ctx = ctx or default_context()
    nd, nn = total_dev.shape
    ctx.call("sdx_accumulate_dev", nd, nn, total_dev.ptr, nn, src_dev.ptr, nn)


# ------------------------------------------------------------------------------------------------ formal solution
def blackbody_flux_at_nu(tracing_nus, temps, ctx=None):
    """source_functions/blackbody.py:10-35; temps (N_d,1) or (N_d,)"""
    ctx = ctx or default_context()
    nus = _host(tracing_nus).reshape(-1)
    t = _host(temps).reshape(-1)
    d_n, d_t = ctx.upload(nus), ctx.upload(t)
    out = ctx.empty((t.size, nus.size))
    ctx.call("sdx_blackbody_dev", t.size, nus.size, d_n.ptr, d_t.ptr, out.ptr, nus.size)
    return out.numpy()


def calc_weights_parallel(delta_tau, ctx=None):
    """radiation_field_solvers/base.py:6-47"""
    ctx = ctx or default_context()
    tau = _host(delta_tau)
    d = ctx.upload(tau)
    w = [ctx.empty(tau.shape) for _ in range(3)]
    ctx.call("sdx_calc_weights_dev", tau.size, d.ptr, w[0].ptr, w[1].ptr, w[2].ptr)
    return tuple(x.numpy() for x in w)


def raytrace_arrays(tracing_nus, temperatures, ray_distances, theta_weights, total_alphas, F_nu=None, track=False, ctx=None,
                    inward_rays=False, photospheric_correction=1.0, want_flux=True, source=None):
    """radiation_field_solvers/base.py:271-346 on arrays.

    ray_distances is the (N_d-1, N_theta) table of :302-305 (plane-parallel) or of calculate_spherical_ray
    (:296-300; pass inward_rays=True and the photospheric correction of :340-344).  total_alphas may be a host
    array or a device array.  source: optional (N_d, N_nu) source-function plane (a foreign RadiationField.source_function
    evaluated by the caller, :133); default: the Planck function in the kernel.
    Returns (F_nu host array — accumulated into when given —, I_nus or None)."""
    ctx = ctx or default_context()
    nus = _host(tracing_nus).reshape(-1)
    t = _host(temperatures).reshape(-1)
    rd = _host(ray_distances).reshape(t.size - 1, -1)
    w = _host(theta_weights).reshape(-1)
    n_theta = w.size
    d_alpha = _dev(ctx, total_alphas)
    d = [ctx.upload(nus), ctx.upload(t), ctx.upload(rd), ctx.upload(w)]
    d_F = None
    if want_flux:
        d_F = ctx.zeros((t.size, nus.size)) if F_nu is None else ctx.upload(_host(F_nu))
    d_I = ctx.empty((t.size, nus.size, n_theta)) if track else None
    # accumulate only into a flux the caller handed over (base.py:336 adds to F_nu); a fresh one is written — the entry point
    # then picks its kernel freely (the segmented formal solution needs nothing to add to)
    args = (t.size, nus.size, n_theta, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, ptr_of(d_alpha), nus.size, ptr_of(d_F), nus.size,
            ptr_of(d_I), 0 if F_nu is None else 1)
    if source is not None:
        d_S = ctx.upload(_source_plane(source, (t.size, nus.size)))
        ctx.call("sdx_raytrace_source_dev", *args[:9], d_S.ptr, nus.size, *args[9:], 1 if inward_rays else 0, float(photospheric_correction))
    elif inward_rays:
        ctx.call("sdx_raytrace_spherical_dev", *args, float(photospheric_correction))
    else:
        ctx.call("sdx_raytrace_dev", *args)
    return (d_F.numpy() if want_flux else None), (d_I.numpy() if track else None)


def _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=None, cotangent=None, source=None, what=None, planes=None,
                   checked=True):
    """The host-side intake of the products of the formal solution, before any device is asked for -> namespace(nus, t, rd, w, n_theta,
    shape, source, planes).  The number of angles is that of `weights`, else of the rows of `cotangent` (response_angles' (N_theta, N_nu)),
    else of ray_distances' columns.  source: a host source-function plane; planes: {name: plane or None}, host or device (with `what`,
    the name the scattering entries refuse more than 64 or no angles under).  checked=False (contribution_arrays: arguments as
    raytrace_arrays): no shape is checked but the source plane's."""
    import types

    nus = _host(tracing_nus).reshape(-1)
    t = _host(temperatures).reshape(-1)
    rd = _host(ray_distances)
    shape = (t.size, nus.size)
    w = None
    if weights is not None:
        w = _host(weights).reshape(-1)
        n_theta = w.size
        if what and n_theta > 64:
            raise ValueError(f"{what}: more than 64 angles are not supported, got {n_theta}")
    elif cotangent is not None:
        cshape = _shape(cotangent)
        if len(cshape) != 2 or cshape[1] != nus.size or cshape[0] < 1:
            raise ValueError(f"cotangent must have shape (n_theta, {nus.size}), got {cshape}")
        n_theta = cshape[0]
    else:
        if t.size < 2 or rd.ndim != 2 or rd.shape[0] != t.size - 1 or rd.shape[1] < 1:
            raise ValueError(f"ray_distances must have shape ({t.size - 1}, N_theta), got {rd.shape}")
        n_theta = rd.shape[1]
        if n_theta > 64:
            raise ValueError(f"at most 64 angles are traced in one launch, got {n_theta}")
    if checked:
        if t.size < 2 or (what and n_theta == 0) or rd.size != (t.size - 1) * n_theta:
            raise ValueError(f"ray_distances must have shape {(t.size - 1, n_theta)}, got {rd.shape}")
        if _shape(total_alphas) != shape:
            raise ValueError(f"total_alphas must have shape {shape}, got {_shape(total_alphas)}")
    rd = rd.reshape(t.size - 1, n_theta if checked else -1)
    out = {}
    for name, plane in (planes or {}).items():
        if plane is not None and not _on_device(plane):
            plane = _host(plane)
        if plane is not None and _shape(plane) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(plane.shape)}")
        out[name] = plane
    return types.SimpleNamespace(nus=nus, t=t, rd=rd, w=w, n_theta=n_theta, shape=shape, source=_source_plane(source, shape), planes=out)


def _column_uploads(ctx, p, total_alphas, *planes):
    """total_alphas, `planes`, then the grid, the temperatures, the ray table and the weights on the device (what is there already is passed
    through) -> (the arguments every entry begins with, as far as the weights; total_alphas; the planes).  p keeps the uploads alive."""
    d_alpha = _dev(ctx, total_alphas)
    d_planes = [_dev(ctx, plane) for plane in planes]
    p.uploads = [ctx.upload(a) for a in (p.nus, p.t, p.rd, p.w) if a is not None]
    return (p.t.size, p.nus.size, p.n_theta, *(a.ptr for a in p.uploads)), d_alpha, d_planes


def _scatter_inputs(what, alpha_scatter, shape, tol, max_iter):
    """alpha_scatter, (N_d,) or (N_d, N_nu), host or device, and the iteration's scalars -> (alpha_scatter, its leading dimension)"""
    sc = alpha_scatter if _on_device(alpha_scatter) else _host(alpha_scatter)
    if _shape(sc) not in (shape[:1], shape):
        raise ValueError(f"alpha_scatter must have shape {shape[:1]} or {shape}, got {_shape(sc)}")
    if not float(tol) >= 0.0:
        raise ValueError(f"{what}: tol must be >= 0, got {tol}")
    if int(max_iter) < 1:
        raise ValueError(f"{what}: max_iter must be >= 1, got {max_iter}")
    return sc, shape[1] if len(_shape(sc)) == 2 else 0


NG_DEFAULTS = dict(start=4, period=4)


def acceleration_options(what, acceleration):
    """acceleration: None (the plain iteration), "ng", or a dict with start and / or period -> None or dict(start, period); raises
    ValueError on anything else.  Host code alone: no device is asked for."""
    if acceleration is None:
        return None
    if isinstance(acceleration, str):
        if acceleration != "ng":
            raise ValueError(f'{what}: acceleration must be None, "ng" or a dict(start=, period=), got {acceleration!r}')
        return dict(NG_DEFAULTS)
    if not isinstance(acceleration, dict):
        raise ValueError(f'{what}: acceleration must be None, "ng" or a dict(start=, period=), got {acceleration!r}')
    unknown = sorted(set(acceleration) - set(NG_DEFAULTS))
    if unknown:
        raise ValueError(f"{what}: unknown acceleration option {unknown}; known: {sorted(NG_DEFAULTS)}")
    o = dict(NG_DEFAULTS)
    o.update({k: int(v) for k, v in acceleration.items()})
    if o["start"] < 4:
        raise ValueError(f"{what}: acceleration start must be >= 4 (an extrapolation reads four iterates), got {o['start']}")
    if o["period"] < 1:
        raise ValueError(f"{what}: acceleration period must be >= 1, got {o['period']}")
    return o


def _results(out, device):
    """a tuple or a namespace of device outputs as it is, or with every one of them on the host (None stays None)"""
    if device:
        return out
    if isinstance(out, tuple):
        return tuple(None if x is None else x.numpy() for x in out)
    for name, x in vars(out).items():
        setattr(out, name, None if x is None else x.numpy())
    return out


def contribution_arrays(tracing_nus, temperatures, ray_distances, theta_weights, total_alphas, ctx=None, source=None, device=False):
    """Flux contribution function C (N_d, N_nu) of the plane-parallel formal solution (sdx_contribution_dev): what the layer below
    row k adds to the emergent flux, sum_k C[k] = F_nu[-1] up to rounding.  Arguments as raytrace_arrays (ray_distances is the
    (N_d-1, N_theta) table of radiation_field_solvers/base.py:302-305; total_alphas a host or device array; source an optional
    (N_d, N_nu) source-function plane).  device=True: the DeviceArray instead of a host array."""
    ctx = ctx or default_context()
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=theta_weights, source=source, checked=False)
    head, d_alpha, (d_S,) = _column_uploads(ctx, p, total_alphas, p.source)
    n_nu = p.nus.size
    d_C = ctx.empty(p.shape)
    ctx.call("sdx_contribution_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_S), n_nu, d_C.ptr, n_nu)
    return d_C if device else d_C.numpy()


def emergent_intensity(tracing_nus, temperatures, ray_distances, total_alphas, ctx=None, source=None, inward_rays=False, device=False):
    """Emergent intensity of every ray (sdx_emergent_intensity_dev) -> (N_theta, N_nu): row N_d - 1 of the I_nus that raytrace_arrays
    (track=True) returns from the plain kernel, bit for bit, without the (N_d, N_nu, N_theta) volume.  Intensities: no theta weights,
    no photospheric correction.  ray_distances is the (N_d-1, N_theta) table of radiation_field_solvers/base.py:302-305, or of
    calculate_spherical_ray with inward_rays=True; total_alphas a host or device array; source an optional (N_d, N_nu)
    source-function plane.  The shapes are checked before any device work.  device=True: the DeviceArray instead of a host array."""
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, source=source)
    ctx = ctx or default_context()
    head, d_alpha, (d_S,) = _column_uploads(ctx, p, total_alphas, p.source)
    n_nu = p.nus.size
    d_I = ctx.empty((p.n_theta, n_nu))
    ctx.call("sdx_emergent_intensity_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_S), n_nu, 1 if inward_rays else 0, d_I.ptr, n_nu)
    return d_I if device else d_I.numpy()


def response(tracing_nus, temperatures, ray_distances, theta_weights, total_alphas, ctx=None, source=None, device=False,
             want_opacity=True, want_source=True):
    """Response functions of the plane-parallel formal solution (sdx_response_dev) -> (R_alpha, R_source), each (N_d, N_nu): the
    derivative of the emergent flux F_nu[-1] with respect to ln alpha[k] and to the source function S[k] at every depth point
    (sum_k R_source[k] S[k] = F_nu[-1] up to rounding).  Arguments as contribution_arrays; want_opacity / want_source = False: that
    output is not formed (None in its place).  device=True: DeviceArrays instead of host arrays."""
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=theta_weights, source=source)
    if not (want_opacity or want_source):
        raise ValueError("response: no output requested")
    ctx = ctx or default_context()
    head, d_alpha, (d_S,) = _column_uploads(ctx, p, total_alphas, p.source)
    n_nu = p.nus.size
    d_Ra = ctx.empty(p.shape) if want_opacity else None
    d_Rs = ctx.empty(p.shape) if want_source else None
    ctx.call("sdx_response_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_S), n_nu, ptr_of(d_Ra), n_nu, ptr_of(d_Rs), n_nu)
    return _results((d_Ra, d_Rs), device)


def response_angles(tracing_nus, temperatures, ray_distances, cotangent, total_alphas, ctx=None, source=None, device=False,
                    want_opacity=True, want_source=True):
    """The response for a cotangent per (angle, frequency) (sdx_response_angles_dev) -> (R_alpha, R_source), each (N_d, N_nu): the
    derivatives of sum_theta cotangent[theta, nu] I_theta(nu), I the emergent intensities (ops.emergent_intensity), with respect to
    ln alpha[k] and to S[k].  cotangent (N_theta, N_nu), host or device; the other arguments as response.  A cotangent that holds the
    flux weights in every column gives response's bits."""
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, cotangent=cotangent, source=source)
    if not (want_opacity or want_source):
        raise ValueError("response_angles: no output requested")
    ctx = ctx or default_context()
    head, d_alpha, (d_cot, d_S) = _column_uploads(ctx, p, total_alphas, cotangent, p.source)
    n_nu = p.nus.size
    d_Ra = ctx.empty(p.shape) if want_opacity else None
    d_Rs = ctx.empty(p.shape) if want_source else None
    ctx.call("sdx_response_angles_dev", *head, ptr_of(d_cot), n_nu, ptr_of(d_alpha), n_nu, ptr_of(d_S), n_nu, ptr_of(d_Ra), n_nu, ptr_of(d_Rs), n_nu)
    return _results((d_Ra, d_Rs), device)


def mean_weights(thetas, theta_weights):
    """Weights m (N_theta,) of the mean intensity J = sum_k m_k (I_k up + I_k down) for the field's Gauss-Legendre nodes in theta:
    m_k = w_k sin(theta_k) / (2 sum_j w_j sin(theta_j)) with w = I_nus_weights, normalised so that sum_k 2 m_k = 1 to rounding (an
    isotropic field gives J = I).  Host arithmetic on N_theta numbers; the sum is exact (math.fsum) and every quotient correctly rounded."""
    import math

    th, w = _host(thetas).reshape(-1), _host(theta_weights).reshape(-1)
    if th.size == 0 or th.size != w.size:
        raise ValueError(f"thetas and theta_weights must hold the same number of angles, got {th.size} and {w.size}")
    x = w * np.sin(th)
    return x / (2.0 * math.fsum(x))


def mean_intensity(tracing_nus, temperatures, ray_distances, mean_weights, total_alphas, ctx=None, source=None, device=False,
                   want_J=True, want_L=True):
    """Mean intensity of the plane-parallel formal solution (sdx_mean_intensity_dev) -> (J, L), each (N_d, N_nu): J over both
    hemispheres for the source plane (default: Planck) with a thermalised lower boundary, and L, the diagonal of that operator.
    mean_weights: ops.mean_weights(thetas, theta_weights); the other arguments as for response().  want_J / want_L = False: that
    output is not formed (None in its place).  device=True: DeviceArrays instead of host arrays."""
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=mean_weights, what="mean_intensity", planes=dict(source=source))
    if not (want_J or want_L):
        raise ValueError("mean_intensity: no output requested")
    ctx = ctx or default_context()
    head, d_alpha, (d_S,) = _column_uploads(ctx, p, total_alphas, p.planes["source"])
    n_nu = p.nus.size
    d_J = ctx.empty(p.shape) if want_J else None
    d_L = ctx.empty(p.shape) if want_L else None
    ctx.call("sdx_mean_intensity_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_S), n_nu, ptr_of(d_J), n_nu, ptr_of(d_L), n_nu)
    return _results((d_J, d_L), device)


def scatter_source(tracing_nus, temperatures, ray_distances, mean_weights, total_alphas, alpha_scatter, ctx=None, thermal=None,
                   tol=1e-12, max_iter=2000, device=False, want_J=True, acceleration=None):
    """Source function with coherent continuum scattering (sdx_scatter_source_dev): S = (1 - albedo) B + albedo J[S], albedo =
    alpha_scatter / total_alphas, by Jacobi iteration with the local operator, every column on its own until it meets
    max |dS| <= tol max |S| (status 0), has taken max_iter iterations (1) or its change is not finite (2).
    alpha_scatter: (N_d,) — one value per depth point, e.g. Thomson — or (N_d, N_nu), host or device; thermal: optional plane B
    (default: Planck).  -> namespace(S, J, iterations, status, change): S and J (N_d, N_nu) (J of the returned S; None with
    want_J=False), per column the iteration count and status (int32) and the last change.  device=True: DeviceArrays.
    acceleration: None — the plain iteration, the call above —, "ng" or dict(start=4, period=4): Ng acceleration with its safeguard
    (sdx_scatter_source_ng_dev); the namespace then also holds `accelerations`, the extrapolations applied per column (int32).  The
    same fixed point by the same stopping rule in fewer updates where the albedo is high; not the same bits."""
    import types

    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=mean_weights, what="scatter_source", planes=dict(thermal=thermal))
    sc, sc_ld = _scatter_inputs("scatter_source", alpha_scatter, p.shape, tol, max_iter)
    ng = acceleration_options("scatter_source", acceleration)
    ctx = ctx or default_context()
    head, d_alpha, (d_sc, d_B) = _column_uploads(ctx, p, total_alphas, sc, p.planes["thermal"])
    n_nu = p.nus.size
    out = types.SimpleNamespace(S=ctx.empty(p.shape), J=ctx.empty(p.shape) if want_J else None, iterations=ctx.empty((n_nu,), np.int32),
                                status=ctx.empty((n_nu,), np.int32), change=ctx.empty((n_nu,)))
    args = (*head, ptr_of(d_alpha), n_nu, ptr_of(d_sc), sc_ld, ptr_of(d_B), n_nu, float(tol), int(max_iter), out.S.ptr, n_nu,
            ptr_of(out.J), n_nu, out.iterations.ptr, out.status.ptr, out.change.ptr)
    if ng is None:
        ctx.call("sdx_scatter_source_dev", *args)
    else:
        out.accelerations = ctx.empty((n_nu,), np.int32)
        ctx.call("sdx_scatter_source_ng_dev", *args, ng["start"], ng["period"], out.accelerations.ptr)
    return _results(out, device)


def mean_intensity_adjoint(tracing_nus, temperatures, ray_distances, mean_weights, total_alphas, z, ctx=None, source=None, device=False,
                           want_Lt=True, want_G=True):
    """The transpose of mean_intensity's operator (sdx_mean_intensity_adjoint_dev) -> (Lt, G), each (N_d, N_nu): Lt = Lambda^T z for
    the plane z, and G[k] = d(z^T J[S]) / d ln alpha[k] at the fixed source plane S (default: Planck).  Arguments as mean_intensity;
    want_Lt / want_G = False: that output is not formed (None in its place).  device=True: DeviceArrays instead of host arrays."""
    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=mean_weights, what="mean_intensity_adjoint",
                       planes=dict(z=z, source=source))
    if p.planes["z"] is None:
        raise ValueError("mean_intensity_adjoint: z is required")
    if not (want_Lt or want_G):
        raise ValueError("mean_intensity_adjoint: no output requested")
    ctx = ctx or default_context()
    head, d_alpha, (d_z, d_S) = _column_uploads(ctx, p, total_alphas, p.planes["z"], p.planes["source"])
    n_nu = p.nus.size
    d_Lt = ctx.empty(p.shape) if want_Lt else None
    d_G = ctx.empty(p.shape) if want_G else None
    ctx.call("sdx_mean_intensity_adjoint_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_z), n_nu, ptr_of(d_S), n_nu, ptr_of(d_Lt), n_nu, ptr_of(d_G), n_nu)
    return _results((d_Lt, d_G), device)


def scatter_response(tracing_nus, temperatures, ray_distances, mean_weights, total_alphas, alpha_scatter, S, cotangent, ctx=None, direct=None,
                     thermal=None, tol=1e-12, max_iter=2000, device=False, want_y=True):
    """Derivatives of a functional Phi of the scattering solution (sdx_scatter_response_dev): the adjoint solve y = c + Lambda^T (W y)
    by scatter_source's own iteration, transposed, and from it the responses.  S: the source plane of scatter_source; cotangent:
    dPhi/dS; direct: dPhi/d ln alpha at fixed S (default 0) — for the emergent flux, R_source and R_alpha of response(source=S).
    alpha_scatter, thermal, tol, max_iter as for scatter_source.  -> namespace(y, R_thermal, R_absorption, R_scatter, iterations,
    status, change): (N_d, N_nu) planes — dPhi/dB, dPhi/d ln alpha for added true absorption (what takes R_alpha's place), dPhi/d ln
    alpha_scatter — and per column the iteration count and status (int32) and the last change.  device=True: DeviceArrays."""
    import types

    p = _column_inputs(tracing_nus, temperatures, ray_distances, total_alphas, weights=mean_weights, what="scatter_response",
                       planes=dict(S=S, cotangent=cotangent, direct=direct, thermal=thermal))
    if p.planes["S"] is None or p.planes["cotangent"] is None:
        raise ValueError("scatter_response: S and cotangent are required")
    sc, sc_ld = _scatter_inputs("scatter_response", alpha_scatter, p.shape, tol, max_iter)
    ctx = ctx or default_context()
    head, d_alpha, d_in = _column_uploads(ctx, p, total_alphas, sc, *(p.planes[name] for name in ("thermal", "S", "cotangent", "direct")))
    n_nu = p.nus.size
    out = types.SimpleNamespace(y=ctx.empty(p.shape) if want_y else None, R_thermal=ctx.empty(p.shape), R_absorption=ctx.empty(p.shape),
                                R_scatter=ctx.empty(p.shape), iterations=ctx.empty((n_nu,), np.int32), status=ctx.empty((n_nu,), np.int32),
                                change=ctx.empty((n_nu,)))
    ctx.call("sdx_scatter_response_dev", *head, ptr_of(d_alpha), n_nu, ptr_of(d_in[0]), sc_ld, *(v for d in d_in[1:] for v in (ptr_of(d), n_nu)),
             float(tol), int(max_iter), ptr_of(out.y), n_nu, out.R_thermal.ptr, n_nu, out.R_absorption.ptr, n_nu, out.R_scatter.ptr, n_nu,
             out.iterations.ptr, out.status.ptr, out.change.ptr)
    return _results(out, device)


def formation_mean(contribution, x, ctx=None, device=False):
    """Formation mean of a per-depth quantity x (N_d) under a contribution function (N_d, N_nu; host or device array):
    (sum_{k>=1} C[k] m_k) / (sum_{k>=1} C[k]), m_k = (x[k-1] + x[k]) / 2 (sdx_formation_mean_dev) -> (N_nu,)."""
    ctx = ctx or default_context()
    d_C = _dev(ctx, contribution)
    n_depth, n_nu = (int(s) for s in d_C.shape)
    d_x = _dev(ctx, x)
    if int(np.prod(d_x.shape)) != n_depth:
        raise ValueError(f"x must hold one value per depth point ({n_depth}), got shape {tuple(d_x.shape)}")
    d_out = ctx.empty((n_nu,))
    ctx.call("sdx_formation_mean_dev", n_depth, n_nu, ptr_of(d_C), n_nu, ptr_of(d_x), d_out.ptr)
    return d_out if device else d_out.numpy()


# ------------------------------------------------------------------------------------------------ instrument model
def _rotation_keywords(v_rot, limb_darkening, v_mac=0.0):
    """the Instrument's broadening keywords: none for v_rot = 0 and v_mac = 0 (the defaults), so that the call is the one it was"""
    from .instrument import macroturbulence_zeta, rotation_pair

    V, eps = rotation_pair(v_rot, limb_darkening)
    zeta = macroturbulence_zeta(v_mac)
    return dict(dict(v_rot=V, limb_darkening=eps) if V else {}, **(dict(v_mac=zeta) if zeta else {}))


def rotate(lambdas, flux, v_rot, limb_darkening=0.6, reference=None, ctx=None):
    """Rotational broadening in velocity space on any ascending grid (sdx_rotate_f64): Gray's profile for v sin i = v_rot (km/s) and
    a linear limb-darkening coefficient, out_i = sum_j K_ij h_j flux_j / sum_j K_ij h_j over the points within lambda_i v_rot / c of
    lambda_i -> (n,); with a reference -> (flux, reference), both broadened.  Windows that reach past an end of the grid sum what
    exists.  v_rot = 0 is a copy.  (postprocess.rotation_broadening mirrors the reference instead: one kernel at integer pixel
    offsets, a rotation profile on a log-uniform grid only.)"""
    from .instrument import rotate_host

    return rotate_host(ctx, lambdas, flux, v_rot, limb_darkening, reference)


def macroturbulence(lambdas, flux, zeta, reference=None, derivative=False, ctx=None):
    """Radial-tangential macroturbulence in velocity space on any ascending grid (sdx_macroturbulence_f64): Gray's profile with equal
    areas and zeta_R = zeta_T = zeta (km/s), disk-integrated without limb darkening, K(u) = exp(-u^2) - sqrt(pi) u erfc(u) with u =
    |dv| / zeta, out_i = sum_j K_ij h_j flux_j / sum_j K_ij h_j over the points within 6 zeta of lambda_i -> (n,); with a reference ->
    (flux, reference), both broadened.  derivative=True appends d / d ln zeta of each, from the same launch.  Windows that reach past
    an end of the grid sum what exists.  zeta = 0 is a copy."""
    from .instrument import macroturbulence_host

    return macroturbulence_host(ctx, lambdas, flux, zeta, reference, derivative)


def observe(lambdas, flux, pixel_edges, sigma, v_rad=0.0, reference=None, ctx=None, v_rot=0.0, limb_darkening=0.6, v_mac=0.0):
    """What a spectrograph records of a spectrum (sdx_observe_dev): the wavelengths shifted by the radial velocity v_rad (km/s), a
    Gaussian line-spread function of width sigma (Angstrom; a scalar or one value per pixel) and integration over the pixels between
    pixel_edges -> (n_pix,).  With a reference the continuum-normalised observed spectrum, observe(flux) / observe(reference).  A
    pixel whose window (its edges -+ 8 sigma) the shifted grid does not cover is NaN.  v_rot > 0 (km/s): the star's rotation first
    (ops.rotate with limb_darkening, on the rest-frame grid); v_mac > 0 (km/s): then the macroturbulence (ops.macroturbulence).
    stardis_amd.instrument.Instrument keeps the pixels on the device for repeated calls."""
    from .instrument import Instrument

    inst = Instrument(pixel_edges, sigma=sigma, ctx=ctx, **_rotation_keywords(v_rot, limb_darkening, v_mac))
    if v_rad:
        inst.set_radial_velocity(v_rad)
    return inst.observe_host(lambdas, flux, reference)


def observe_adjoint(lambdas, pixel_weights, pixel_edges, sigma, v_rad=0.0, flux=None, reference=None, nus=None, ctx=None, v_rot=0.0,
                    limb_darkening=0.6, v_mac=0.0):
    """The transpose of observe (sdx_observe_adjoint_f64): pixel_weights c (n_pix,) -> weights w (n,) over the grid points with
    sum_j c_j observe(flux)_j = sum_i w_i flux_i over the pixels the shifted grid covers (c of a NaN pixel is never read) — the
    derivative of any functional of the observed pixels pulled back to the model's grid.  With a reference (which needs the flux) ->
    (weights to the flux, weights to the reference) of the normalised spectrum.  nus: the weights then apply to F_nu instead of
    F_lambda.  v_rot > 0, v_mac > 0: the transpose of observe with the same v_rot, limb_darkening and v_mac, the broadenings
    included.  Arguments of the
    wrong length raise ValueError naming them, before any device work."""
    from .instrument import Instrument, adjoint_host_arguments, pixel_sigma

    edges, _ = pixel_sigma(pixel_edges, sigma=sigma)
    adjoint_host_arguments(edges.size - 1, lambdas, pixel_weights, flux, reference, nus)
    inst = Instrument(pixel_edges, sigma=sigma, ctx=ctx, **_rotation_keywords(v_rot, limb_darkening, v_mac))
    if v_rad:
        inst.set_radial_velocity(v_rad)
    return inst.adjoint_host(lambdas, pixel_weights, flux, reference, nus)


def observe_response_grad(e0, e1, x, sigma, ctx=None):
    """-> (r, dr/dx, dr/d ln sigma): the Gaussian of width sigma around x integrated from e0 to e1, and its two partial derivatives, point
    by point through the routines the instrument's tangent evaluates (sdx_observe_response_grad_dev; sdx_kernels.h obs_response,
    obs_response_grad).  The arguments broadcast."""
    ctx = ctx or default_context()
    both = np.broadcast_arrays(_host(e0), _host(e1), _host(x), _host(sigma))
    shape = both[0].shape
    d = [ctx.upload(np.ascontiguousarray(v).reshape(-1)) for v in both]
    out = [ctx.empty((both[0].size,)) for _ in range(3)]
    ctx.call("sdx_observe_response_grad_dev", both[0].size, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out[0].ptr, out[1].ptr, out[2].ptr)
    r = tuple(o.numpy().reshape(shape) for o in out)
    return r if shape else tuple(v[()] for v in r)


def rotate_tangent(lambdas, flux, v_rot, limb_darkening=0.6, reference=None, ctx=None):
    """ops.rotate with its derivative to the limb-darkening coefficient from the same pass (sdx_rotate_tangent_f64) -> (out, dout_eps), or
    (out, out_reference, dout_eps, dout_eps_reference) with a reference.  v_rot = 0 copies and the derivatives are zeros."""
    from .instrument import _public, _stage_host, rotation_pair

    pair = rotation_pair(v_rot, limb_darkening)
    return _public(_stage_host(ctx, "sdx_rotate_tangent_f64", _lib.plain(lambdas), flux, reference, pair, 4, 4))


def observe_tangent(lambdas, flux, pixel_edges, sigma, v_rad=0.0, reference=None, dflux=None, dreference=None, ctx=None):
    """The pixel stage's tangents (sdx_observe_tangent_f64) -> a dict of (n_pix,) arrays: "out" (ops.observe's own bits), "v_rad"
    (d out / d v_rad per km/s), "lsf" (d out / d ln kappa of a common factor on sigma) and, with dflux (and dreference, which needs a
    reference), "flux": the tangent of out for that direction of (flux, reference).  NaN where out is NaN.  No rotation or
    macroturbulence here: stardis_amd.instrument.Instrument.tangent and parameter_tangents run the whole chain."""
    from .instrument import _grid, _host_ptr as host, _host_vector, doppler_factor, pixel_sigma

    edges, sig = pixel_sigma(pixel_edges, sigma=sigma)
    lam = _grid(_lib.plain(lambdas))
    if dreference is not None and reference is None:
        raise ValueError("dreference needs a reference")
    if dreference is not None and dflux is None:
        raise ValueError("dreference needs dflux")
    f = _host_vector("flux", flux, lam.size, "grid point")
    g, df, dg = (None if a is None else _host_vector(name, a, lam.size, "grid point")
                 for name, a in (("reference", reference), ("dflux", dflux), ("dreference", dreference)))
    n_pix = edges.size - 1
    res = {"out": np.empty(n_pix), "v_rad": np.empty(n_pix), "lsf": np.empty(n_pix)}
    if df is not None:
        res["flux"] = np.empty(n_pix)
    (ctx or default_context()).call("sdx_observe_tangent_f64", lam.size, host(lam), host(f), host(g), n_pix, host(edges), host(sig),
                                    doppler_factor(v_rad), host(df), host(dg), host(res["out"]), host(res["v_rad"]), host(res["lsf"]),
                                    host(res.get("flux")))
    return res


def rotate_integrated(lambdas, flux, v_rot, limb_darkening=0.6, reference=None, derivatives=False, ctx=None):
    """Rotational broadening with the profile integrated over the grid's cells (sdx_rotate_integrated_f64): the flux is piecewise
    linear between the nodes and Gray's profile is integrated against it exactly, so the result is differentiable in v_rot and tends
    to the identity as v_rot -> 0 -> (n,), or (flux, reference) with a reference.  derivatives=True appends d / d ln v_rot and
    d / d limb_darkening of each, from the same launch: (out, dout_lnv, dout_eps), or (out, out_reference, dout_lnv,
    dout_lnv_reference, dout_eps, dout_eps_reference).  v_rot = 0 copies and the derivatives are zeros."""
    from .instrument import rotate_integrated_host

    return rotate_integrated_host(ctx, lambdas, flux, v_rot, limb_darkening, reference, derivatives)


def rotate_integrated_adjoint(lambdas, u, v_rot, limb_darkening=0.6, u_reference=None, nus=None, ctx=None):
    """The transpose of rotate_integrated (sdx_rotate_integrated_adjoint_f64): weights u over the broadened points -> weights w over
    the grid points with sum_i u_i rotate_integrated(flux)_i = sum_j w_j flux_j, or (w, w_reference) with u_reference.  nus: the
    weights then apply to F_nu instead of F_lambda."""
    from .instrument import _grid, _host_ptr as host, _host_vector, rotation_pair

    V, eps = rotation_pair(v_rot, limb_darkening)
    lam = _grid(_lib.plain(lambdas))
    uu = _host_vector("u", u, lam.size, "grid point")
    ur, nu = (None if a is None else _host_vector(name, a, lam.size, "grid point") for name, a in (("u_reference", u_reference), ("nus", nus)))
    w, w_ref = np.empty(lam.size), None if ur is None else np.empty(lam.size)
    (ctx or default_context()).call("sdx_rotate_integrated_adjoint_f64", lam.size, host(lam), V, eps, host(uu), host(ur), host(nu), host(w),
                                    host(w_ref))
    return w if w_ref is None else (w, w_ref)


def _disk_arguments(lambdas, ring_scale, ring_weights, v_rot):
    """The checked arguments the disk entries share -> (lam, V, scale, w)"""
    from .instrument import _grid, _host_vector, rotation_pair

    lam = _grid(_lib.plain(lambdas))
    V, _ = rotation_pair(v_rot)
    scale = np.ascontiguousarray(_lib.plain(ring_scale), dtype=F8).reshape(-1)
    n_rings = scale.size
    if not 1 <= n_rings <= 64:
        raise ValueError(f"ring_scale must hold 1 to 64 rings, got {n_rings}")
    if not np.all((scale >= 0.0) & (scale <= 1.0)):
        raise ValueError("ring_scale must lie in [0, 1]")
    w = _host_vector("ring_weights", _lib.plain(ring_weights), n_rings, "ring")
    return lam, V, scale, w


def disk_integrate(lambdas, intensities, ring_scale, ring_weights, v_rot, reference=None, ctx=None, derivative=False):
    """Disk integration with rigid rotation (sdx_disk_integrate_f64): per-ring spectra intensities (n_rings, n) on the ascending grid
    lambdas, ring r at the projected radius ring_scale[r] = sin theta_r in [0, 1] with the flux weight ring_weights[r]; every ring is
    convolved with the arcsine density of half-width v_rot ring_scale[r] / c, integrated exactly against the piecewise-linear spectrum,
    and the rings are summed in the flux's order -> (n,), or (out, out_reference) with a reference (n_rings, n).  v_rot = 0 is the
    flux sum itself.  No limb-darkening coefficient: the centre-to-limb variation is in the spectra (ops.emergent_intensity).
    derivative=True (sdx_disk_integrate_deriv_f64) appends d / d ln v_rot of each from the same launch: (out, dout_lnv), or (out,
    out_reference, dout_lnv, dout_lnv_reference); exact for the discrete operator, zeros at v_rot = 0, and not meant where an end of
    the grid lies within 1e-5 of a ring's edge.  The arguments are checked before any device work (ValueError naming the argument)."""
    from .instrument import _host_ptr as host

    lam, V, scale, w = _disk_arguments(lambdas, ring_scale, ring_weights, v_rot)
    n_rings = scale.size

    def rings(name, a):
        a = np.ascontiguousarray(_lib.plain(a), dtype=F8)
        if a.shape != (n_rings, lam.size):
            raise ValueError(f"{name} must have shape {(n_rings, lam.size)}, got {a.shape}")
        return a

    I = rings("intensities", intensities)
    G = None if reference is None else rings("reference", reference)
    out, out_ref = np.empty(lam.size), None if G is None else np.empty(lam.size)
    if not derivative:
        (ctx or default_context()).call("sdx_disk_integrate_f64", lam.size, host(lam), n_rings, host(scale), host(w), host(I), host(G), V, host(out),
                                        host(out_ref))
        return out if out_ref is None else (out, out_ref)
    d, d_ref = np.empty(lam.size), None if G is None else np.empty(lam.size)
    (ctx or default_context()).call("sdx_disk_integrate_deriv_f64", lam.size, host(lam), n_rings, host(scale), host(w), host(I), host(G), V,
                                    host(out), host(out_ref), host(d), host(d_ref))
    return (out, d) if out_ref is None else (out, out_ref, d, d_ref)


def disk_integrate_adjoint(lambdas, u, ring_scale, ring_weights, v_rot, u_reference=None, nus=None, ctx=None):
    """The transpose of disk_integrate (sdx_disk_integrate_adjoint_f64): weights u (n,) over the disk-integrated points -> the plane W
    (n_rings, n) over (ring, grid point) with sum_i u_i disk_integrate(I)_i = sum_r sum_j W[r, j] I[r, j], or (W, W_reference) with
    u_reference.  v_rot = 0: W[r, j] = ring_weights[r] u[j].  nus: the plane then applies to I_nu instead of I_lambda."""
    from .instrument import _host_ptr as host, _host_vector

    lam, V, scale, w = _disk_arguments(lambdas, ring_scale, ring_weights, v_rot)
    uu = _host_vector("u", u, lam.size, "grid point")
    ur, nu = (None if a is None else _host_vector(name, a, lam.size, "grid point") for name, a in (("u_reference", u_reference), ("nus", nus)))
    W, W_ref = np.empty((scale.size, lam.size)), None if ur is None else np.empty((scale.size, lam.size))
    (ctx or default_context()).call("sdx_disk_integrate_adjoint_f64", lam.size, host(lam), scale.size, host(scale), host(w), V, host(uu), host(ur),
                                    host(nu), host(W), host(W_ref))
    return W if W_ref is None else (W, W_ref)


def rotate_moments(ya, yb, limb_darkening=0.6, ctx=None):
    """-> (M0, M1): the integrals of K(y) and y K(y), K Gray's rotation profile 2 (1 - eps) sqrt(1 - y^2) + (pi / 2) eps (1 - y^2), over
    [ya, yb] clamped to [-1, 1], point by point through the routine the integrated rotation evaluates (sdx_rotate_moments_f64;
    sdx_kernels.h rot_moments).  The arguments broadcast."""
    both = np.broadcast_arrays(_host(ya), _host(yb), _host(limb_darkening))
    shape = both[0].shape
    a, b, e = (np.ascontiguousarray(v, dtype=F8).reshape(-1) for v in both)
    m0, m1 = np.empty(a.size), np.empty(a.size)
    (ctx or default_context()).call("sdx_rotate_moments_f64", a.size, a.ctypes.data, b.ctypes.data, e.ctypes.data, m0.ctypes.data,
                                    m1.ctypes.data)
    r = (m0.reshape(shape), m1.reshape(shape))
    return r if shape else tuple(v[()] for v in r)
