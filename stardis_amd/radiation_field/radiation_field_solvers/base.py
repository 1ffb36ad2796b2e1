"""LTE formal solution on MI355X, call-compatible with
stardis/radiation_field/radiation_field_solvers/base.py (van Noort 2002 eq. 14 short characteristics).

The per-angle, per-frequency depth recurrence runs in one HIP kernel (k_raytrace in
stardis_amd/csrc/sdx_kernels.h); this module builds the ray-length table and moves arrays."""
import numpy as np

from stardis_amd import ops
from stardis_amd._lib import default_context, plain


def calc_weights_parallel(delta_tau):
    """w0, w1, w2 of eq. 14 for an array of optical depths.  Reference :6-47."""
    return ops.calc_weights_parallel(delta_tau)


calc_weights = calc_weights_parallel  # the reference keeps an unused numpy twin (:50-82) with the same contract


def _source_plane(source_function, tracing_nus, temps):
    """None for the Planck function (evaluated inside the kernel), else the caller's source function evaluated on the host
    the way the reference calls it — source_function(tracing_nus, temps) with temps shaped (N_d, 1), :133 — as a plain
    (N_d, N_nu) array for the kernel to read."""
    if source_function is None or getattr(source_function, "__name__", "") == "blackbody_flux_at_nu":
        return None
    nus = np.asarray(plain(tracing_nus), dtype=np.float64).reshape(-1)
    t = np.asarray(plain(temps), dtype=np.float64).reshape(-1, 1)
    plane = np.asarray(plain(source_function(nus, t)), dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(plane, (t.size, nus.size)))


def single_theta_trace_parallel(ray_dist_to_next_depth_point, temps, alphas, tracing_nus, source_function=None,
                                inward_rays=False):
    """Specific intensity (N_d, N_nu) along one ray direction.  Reference :85-268; inward_rays adds the
    surface-to-centre sweep of spherical geometry (:141-198) before the outward pass."""
    rd = np.asarray(plain(ray_dist_to_next_depth_point), dtype=np.float64).reshape(-1, 1)
    _, I = ops.raytrace_arrays(tracing_nus, temps, rd, np.ones(1), alphas, track=True, inward_rays=bool(inward_rays), want_flux=False,
                               source=_source_plane(source_function, tracing_nus, temps))
    return I[:, :, 0]


def calculate_spherical_ray(thetas, depth_points_radii):
    """Chord length of each ray through each shell (N_d-1, N_theta).  Reference :349-381.  Geometry set-up,
    a (N_d x N_theta) table built once on the host."""
    thetas = np.asarray(thetas, dtype=np.float64)
    r = np.asarray(plain(depth_points_radii), dtype=np.float64)
    out = np.zeros((len(r) - 1, len(thetas)))
    for k, theta in enumerate(thetas):
        b = r[-1] * np.sin(theta)
        with np.errstate(invalid="ignore"):
            z = np.sqrt(r**2 - b**2)
        dz = np.diff(z)
        ok = ~np.isnan(dz)
        out[ok, k] = dz[ok]
    return out


def raytrace(stellar_model, stellar_radiation_field):
    """Trace every angle and accumulate the Gauss-Legendre flux sum into stellar_radiation_field.F_nu
    (in place, like the reference :324-338).  Fills I_nus when track_individual_intensities is set."""
    field = stellar_radiation_field
    thetas = np.asarray(field.thetas, dtype=np.float64)
    correction = 1.0
    if stellar_model.spherical:  # :296-300, :340-344
        radii = np.asarray(plain(stellar_model.geometry.r), dtype=np.float64)
        ray_distances = calculate_spherical_ray(thetas, radii)
        correction = (radii[-1] / float(plain(stellar_model.geometry.reference_r))) ** 2
    else:
        dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
        ray_distances = dist.reshape(-1, 1) / np.cos(thetas)  # :302-305
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    track = bool(getattr(field, "track_individual_intensities", False))
    # F_nu is accumulated into (:336); a freshly created field holds zeros, which need no upload
    f_in = field.F_nu if np.any(field.F_nu) else None
    F, I = ops.raytrace_arrays(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, field.I_nus_weights, alphas, F_nu=f_in,
        track=track, ctx=ctx, inward_rays=bool(stellar_model.spherical), photospheric_correction=correction,
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )
    field.F_nu[...] = F
    if track:
        field.I_nus[...] = I
    return field.F_nu


def continuum_flux(stellar_model, stellar_radiation_field, continuum_alphas):
    """The raytrace above applied to a continuum plane (N_d, N_nu; host or device array) into a fresh zero flux: the same angles,
    source function and geometry as the field's own F_nu, no intensities.  -> F_nu_continuum (N_d, N_nu)."""
    field = stellar_radiation_field
    thetas = np.asarray(field.thetas, dtype=np.float64)
    correction = 1.0
    if stellar_model.spherical:
        radii = np.asarray(plain(stellar_model.geometry.r), dtype=np.float64)
        ray_distances = calculate_spherical_ray(thetas, radii)
        correction = (radii[-1] / float(plain(stellar_model.geometry.reference_r))) ** 2
    else:
        dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
        ray_distances = dist.reshape(-1, 1) / np.cos(thetas)
    F, _ = ops.raytrace_arrays(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, field.I_nus_weights, continuum_alphas,
        ctx=default_context(), inward_rays=bool(stellar_model.spherical), photospheric_correction=correction,
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )
    return F


def _ray_table(stellar_model, field):
    """-> (ray_distances (N_d-1, N_theta), photospheric correction) of the field's angles, as raytrace() builds them"""
    thetas = np.asarray(field.thetas, dtype=np.float64)
    if stellar_model.spherical:  # :296-300, :340-344
        radii = np.asarray(plain(stellar_model.geometry.r), dtype=np.float64)
        return calculate_spherical_ray(thetas, radii), (radii[-1] / float(plain(stellar_model.geometry.reference_r))) ** 2
    dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
    return dist.reshape(-1, 1) / np.cos(thetas), 1.0  # :302-305


def emergent_intensities(stellar_model, stellar_radiation_field):
    """Emergent intensity (N_theta, N_nu) of every angle of the field's formal solution (sdx_emergent_intensity_dev): the last row of
    the I_nus that track_individual_intensities would fill, without the (N_d, N_nu, N_theta) volume.  The same angles, source
    function, geometry (plane-parallel or spherical) and total opacity as raytrace() above; no weights and no photospheric correction
    are applied.  The reference has no counterpart."""
    field = stellar_radiation_field
    ray_distances, _ = _ray_table(stellar_model, field)
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    return ops.emergent_intensity(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, alphas, ctx=ctx, inward_rays=bool(stellar_model.spherical),
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )


def disk_integrated_flux(stellar_model, stellar_radiation_field, v_rot):
    """F_lambda (N_nu,) on the field's grid, integrated over the disk of a rigid rotator with v sin i = v_rot (km/s): every angle's
    emergent intensity (emergent_intensities above) converted to per Angstrom (I nu / lambda, sdx_flux_nu_to_lambda_dev's operation),
    the ring at the projected radius sin(theta) convolved with its own arcsine density and the rings summed with the field's
    I_nus_weights (sdx_disk_integrate_dev); for a spherical model times the photospheric correction.  The field's frequencies descend,
    so its wavelengths ascend as the operator needs.  v_rot = 0 gives the F_lambda of raytrace()'s F_nu[-1]."""
    from stardis_amd import constants as K

    field = stellar_radiation_field
    nus = np.asarray(plain(field.frequencies), dtype=np.float64).reshape(-1)
    lambdas = K.nu_to_angstrom(nus)
    I_lambda = emergent_intensities(stellar_model, field) * nus / lambdas
    _, correction = _ray_table(stellar_model, field)
    thetas = np.asarray(field.thetas, dtype=np.float64)
    out = ops.disk_integrate(lambdas, I_lambda, np.sin(thetas), field.I_nus_weights, v_rot, ctx=default_context())
    return out * correction if stellar_model.spherical else out


SPHERICAL_CONTRIBUTION = ("the flux contribution function is defined for plane-parallel models: the inward sweep of the spherical formal "
                          "solution makes the intensity at the innermost point non-zero, and the emergent flux is then not a sum over layers alone")


def contribution_function(stellar_model, stellar_radiation_field):
    """Flux contribution function (N_d, N_nu) of the field's formal solution: row k is what the layer below depth point k adds to the
    emergent flux, sum over k = F_nu[-1] up to rounding (row 0 is 0; sdx_contribution_dev).  The same angles, weights, source function,
    geometry and total opacity as raytrace() above; the reference has no counterpart.  A spherical model raises NotImplementedError."""
    field = stellar_radiation_field
    if bool(getattr(stellar_model, "spherical", False)):
        raise NotImplementedError(SPHERICAL_CONTRIBUTION)
    thetas = np.asarray(field.thetas, dtype=np.float64)
    dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
    ray_distances = dist.reshape(-1, 1) / np.cos(thetas)  # :302-305
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    return ops.contribution_arrays(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, field.I_nus_weights, alphas, ctx=ctx,
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )


SPHERICAL_RESPONSE = ("the response functions are defined for plane-parallel models: the inward sweep of the spherical formal solution makes "
                      "the intensity at the innermost point depend on every layer, and the derivative is then not that of the outward chain alone")


def response_functions(stellar_model, stellar_radiation_field):
    """Response functions (R_alpha, R_source), each (N_d, N_nu), of the field's formal solution: the derivative of the emergent flux
    F_nu[-1] with respect to ln(total opacity) and to the source function at every depth point (sdx_response_dev); the sensitivity to
    any parameter is a weighted sum of them over depth.  The same angles, weights, source function, geometry and total opacity as
    raytrace() above; the reference has no counterpart.  A spherical model raises NotImplementedError."""
    field = stellar_radiation_field
    if bool(getattr(stellar_model, "spherical", False)):
        raise NotImplementedError(SPHERICAL_RESPONSE)
    thetas = np.asarray(field.thetas, dtype=np.float64)
    dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
    ray_distances = dist.reshape(-1, 1) / np.cos(thetas)  # :302-305
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    return ops.response(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, field.I_nus_weights, alphas, ctx=ctx,
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )


def ray_response(stellar_model, stellar_radiation_field, cotangent):
    """(R_alpha, R_source), each (N_d, N_nu), for a cotangent (N_theta, N_nu) on emergent_intensities() above: the derivatives of
    sum_theta cotangent[theta, nu] I_theta(nu) with respect to ln(total opacity) and to the source function at every depth point
    (sdx_response_angles_dev) — what carries the transpose of the disk integration (ops.disk_integrate_adjoint) back into the
    atmosphere.  With the field's I_nus_weights in every column it is response_functions() bit for bit.  A spherical model raises
    NotImplementedError."""
    field = stellar_radiation_field
    if bool(getattr(stellar_model, "spherical", False)):
        raise NotImplementedError(SPHERICAL_RESPONSE)
    thetas = np.asarray(field.thetas, dtype=np.float64)
    dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
    ray_distances = dist.reshape(-1, 1) / np.cos(thetas)  # :302-305
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    return ops.response_angles(
        field.frequencies, plain(stellar_model.temperatures), ray_distances, cotangent, alphas, ctx=ctx,
        source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures),
    )


SPHERICAL_SCATTERING = ("the mean intensity and the scattering source function are defined for plane-parallel models: the downward sweep "
                        "of a spherical model runs along chords that miss the inner shells, which the two-hemisphere quadrature here does not describe")


def _lambda_arguments(stellar_model, field):
    """what ops.mean_intensity and ops.scatter_source take from a model and its field: frequencies, temperatures, the ray table of
    :302-305, the mean weights of the field's angles, the total opacity (on the device where the field keeps it there), the context"""
    if bool(getattr(stellar_model, "spherical", False)):
        raise NotImplementedError(SPHERICAL_SCATTERING)
    thetas = np.asarray(field.thetas, dtype=np.float64)
    dist = np.asarray(plain(stellar_model.geometry.dist_to_next_depth_point), dtype=np.float64)
    ray_distances = dist.reshape(-1, 1) / np.cos(thetas)
    ctx = default_context()
    opac = field.opacities
    alphas = opac.total_alphas_device(ctx) if hasattr(opac, "total_alphas_device") else opac.total_alphas
    return (field.frequencies, plain(stellar_model.temperatures), ray_distances, ops.mean_weights(thetas, field.I_nus_weights), alphas), ctx


def mean_intensity(stellar_model, stellar_radiation_field):
    """Mean intensity J and the diagonal L of its operator, each (N_d, N_nu), of the field's formal solution over both hemispheres
    (sdx_mean_intensity_dev): the same angles, source function, geometry and total opacity as raytrace() above, the lower boundary
    thermalised.  The reference has no counterpart.  A spherical model raises NotImplementedError."""
    field = stellar_radiation_field
    args, ctx = _lambda_arguments(stellar_model, field)
    return ops.mean_intensity(*args, ctx=ctx, source=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures))


def _scatter_plane(field, shape):
    """the field's own Rayleigh + Thomson entries as one plane, summed in the order of the total"""
    entries = field.opacities.opacities_dict
    scatter = np.zeros(shape)
    for key in ("alpha_rayleigh", "alpha_electron"):  # (the order of the total: ... + rayleigh) + electron)
        if key not in entries:
            raise ValueError(f"the field's opacities carry no {key}: calc_alphas has not run")
        scatter = scatter + np.broadcast_to(np.asarray(plain(entries[key]), dtype=np.float64), shape)
    return scatter


def scattering_source(stellar_model, stellar_radiation_field, tol=1e-12, max_iter=2000, acceleration=None):
    """Source function with coherent continuum scattering, S = (1 - albedo) B + albedo J[S] (sdx_scatter_source_dev) -> namespace(S, J,
    iterations, status, change) as ops.scatter_source returns it.  The scattering opacity is the field's own Rayleigh + Thomson entries
    (opacities_dict["alpha_rayleigh"] + ["alpha_electron"], which the total holds as absorption); B is the field's source function.
    S feeds raytrace(), contribution_function() and response_functions() as a source plane: a field whose source_function returns it
    is traced with scattering.  acceleration: None, "ng" or dict(start=, period=) as ops.scatter_source takes it (Ng acceleration,
    sdx_scatter_source_ng_dev; the namespace then holds `accelerations`).  The reference has no counterpart.  A spherical model raises
    NotImplementedError."""
    ops.acceleration_options("scattering_source", acceleration)
    field = stellar_radiation_field
    args, ctx = _lambda_arguments(stellar_model, field)
    scatter = _scatter_plane(field, (np.size(args[1]), np.size(plain(field.frequencies))))
    return ops.scatter_source(*args, scatter, ctx=ctx, tol=tol, max_iter=max_iter, acceleration=acceleration,
                              thermal=_source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures))


def scattering_response(stellar_model, stellar_radiation_field, tol=1e-12, max_iter=2000, acceleration=None):
    """Response functions of the emergent flux WITH continuum scattering (sdx_scatter_response_dev): solves for the scattering source
    function S as scattering_source() does, takes the flux's cotangent and direct part from the response functions at source = S, and
    solves the adjoint problem -> namespace(y, R_thermal, R_absorption, R_scatter, iterations, status, change) as ops.scatter_response
    returns it, with S and the forward solve's own `source_iterations` and `source_status` beside them.  R_absorption takes the place
    of response_functions()'s R_alpha once scattering is on.  acceleration (as scattering_source takes it) accelerates the FORWARD solve
    alone — the adjoint solve has no accelerated kernel ("The scattering adjoint") —; `source_accelerations` then stands beside
    `source_iterations`.  A spherical model raises NotImplementedError."""
    ops.acceleration_options("scattering_response", acceleration)
    field = stellar_radiation_field
    args, ctx = _lambda_arguments(stellar_model, field)
    scatter = _scatter_plane(field, (np.size(args[1]), np.size(plain(field.frequencies))))
    thermal = _source_plane(getattr(field, "source_function", None), field.frequencies, stellar_model.temperatures)
    forward = ops.scatter_source(*args, scatter, ctx=ctx, tol=tol, max_iter=max_iter, thermal=thermal, want_J=False, acceleration=acceleration)
    R_alpha, R_source = ops.response(args[0], args[1], args[2], field.I_nus_weights, args[4], ctx=ctx, source=forward.S)
    out = ops.scatter_response(*args, scatter, forward.S, R_source, ctx=ctx, direct=R_alpha, thermal=thermal, tol=tol, max_iter=max_iter)
    out.S, out.source_iterations, out.source_status = forward.S, forward.iterations, forward.status
    if acceleration is not None:
        out.source_accelerations = forward.accelerations
    return out


def formation_mean(stellar_radiation_field, x):
    """Formation mean (N_nu,) of a per-depth quantity x (N_d: geometric depth, temperature, a reference log tau) under the field's
    contribution function: (sum_{k>=1} C[k] m_k) / (sum_{k>=1} C[k]), m_k = (x[k-1] + x[k]) / 2 (sdx_formation_mean_dev).  The field must
    carry contribution_function (create_stellar_radiation_field(..., contribution=True), or assign contribution_function()'s result)."""
    C = getattr(stellar_radiation_field, "contribution_function", None)
    if C is None:
        raise ValueError("the field carries no contribution_function: create it with contribution=True")
    return ops.formation_mean(C, np.asarray(plain(x), dtype=np.float64).reshape(-1))
