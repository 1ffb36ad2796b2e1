"""The instrument model on the device: radial-velocity shift, a Gaussian line-spread function whose width is given per pixel, and
integration over the detector's pixels — one launch of k_observe behind the synthesis (include/stardis_hip.h, sdx_observe_dev, states
the operator).  The reference has no counterpart; its rotation-broadening walk-through applies scipy.ndimage.gaussian_filter1d at one
sigma in grid points (postprocess.gaussian_filter1d mirrors that), which is a constant resolving power on a log-uniform grid only.
Instrument.adjoint is the operator transposed (sdx_observe_adjoint_dev): weights over the pixels pulled back to weights over the grid."""
import math

import numpy as np

from . import constants as K
from ._lib import default_context, ptr_of

FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


def doppler_factor(v_kms):
    """D = sqrt((1 + beta) / (1 - beta)), beta = v / c: observed wavelength over rest wavelength (v > 0 recedes)."""
    beta = float(v_kms) / K.C_KMS
    if not abs(beta) < 1.0:
        raise ValueError("radial velocity must lie strictly between -c and c")
    return math.sqrt((1.0 + beta) / (1.0 - beta))


def _ascending(name, a):
    if a.ndim != 1 or not np.all(np.isfinite(a)) or np.any(np.diff(a) <= 0):
        raise ValueError(f"{name} must be a finite, strictly ascending 1-d array")


def pixel_sigma(pixel_edges, resolving_power=None, sigma=None):
    """-> (edges, sigma): the validated pixel edges and the line-spread function's Gaussian width per pixel (Angstrom).  Exactly one of
    resolving_power (sigma_j = centre_j / (R 2 sqrt(2 ln 2))) and sigma is given, each a scalar or one value per pixel.  Needs no device."""
    edges = np.ascontiguousarray(getattr(pixel_edges, "value", pixel_edges), dtype=np.float64)
    if edges.ndim != 1 or edges.size < 1:
        raise ValueError("pixel_edges must be a 1-d array of n_pix + 1 values")
    _ascending("pixel_edges", edges)
    n_pix = edges.size - 1
    if (resolving_power is None) == (sigma is None):
        raise ValueError("give exactly one of resolving_power and sigma")
    name, given = ("sigma", sigma) if resolving_power is None else ("resolving_power", resolving_power)
    v = np.asarray(getattr(given, "value", given), dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.size != n_pix):
        raise ValueError(f"{name} must be a scalar or one value per pixel ({n_pix})")
    if not np.all(np.isfinite(v)) or np.any(v <= 0):
        raise ValueError(f"{name} must be finite and > 0")
    v = np.ascontiguousarray(np.broadcast_to(v, (n_pix,)))
    if resolving_power is not None:
        v = (edges[:-1] + edges[1:]) / 2 / (v * FWHM_PER_SIGMA)
    return edges, v


def _host_vector(name, a, n, what):
    v = np.ascontiguousarray(getattr(a, "value", a), dtype=np.float64).reshape(-1)
    if v.size != n:
        raise ValueError(f"{name} must hold one value per {what} ({n}), got {v.size}")
    return v


def adjoint_host_arguments(n_pix, lambdas, pixel_weights, flux=None, reference=None, nus=None):
    """The host arrays of Instrument.adjoint_host, validated (ValueError naming the argument; needs no device) ->
    (lambdas, pixel_weights, flux, reference, nus), the optional ones None where not given."""
    lam = np.ascontiguousarray(getattr(lambdas, "value", lambdas), dtype=np.float64).reshape(-1)
    _ascending("lambdas", lam)
    if lam.size < 2:
        raise ValueError("lambdas must hold at least two points")
    c = _host_vector("pixel_weights", pixel_weights, n_pix, "pixel")
    if reference is not None and flux is None:
        raise ValueError("a reference needs the flux: the normalised pixel value enters the weights")
    f = None if flux is None or reference is None else _host_vector("flux", flux, lam.size, "grid point")
    g = None if reference is None else _host_vector("reference", reference, lam.size, "grid point")
    nu = None if nus is None else _host_vector("nus", nus, lam.size, "grid point")
    return lam, c, f, g, nu


class Instrument:
    """A spectrograph: pixel edges (Angstrom, ascending), the line-spread function as a resolving power or a Gaussian sigma (Angstrom),
    and the star's radial velocity.  Edges, sigma, the Doppler factor and the output stay on the device; observe() is one launch, and a
    graph that recorded it follows set_radial_velocity() without being recorded again (the kernel reads the factor from device memory)."""

    def __init__(self, pixel_edges, resolving_power=None, sigma=None, ctx=None):
        self.edges, self.sigma = pixel_sigma(pixel_edges, resolving_power, sigma)  # (ValueError before any device work)
        self.n_pix = self.edges.size - 1
        self.ctx = ctx or default_context()
        self.d_edges = self.ctx.upload(self.edges)
        self.d_sigma = self.ctx.upload(self.sigma)
        self.d_doppler = self.ctx.empty((1,))
        self.d_out = self.ctx.empty((self.n_pix,))
        self.set_radial_velocity(0.0)

    def set_radial_velocity(self, v_kms):
        """Write the Doppler factor of v_kms into the device scalar, in order on the context's stream."""
        D = doppler_factor(v_kms)
        self.d_doppler.set(np.array([D]))
        self.v_kms, self.doppler = float(v_kms), D

    def observe(self, d_lambdas, d_flux, n, reference=None, out=None):
        """n points of (wavelength, flux[, reference]) already on the device (DeviceArrays, CUDA tensors or raw addresses) -> the
        DeviceArray (n_pix,) of the instrument (or `out`), enqueued on the context's stream: nothing is allocated, nothing waits."""
        addr = lambda a: a if isinstance(a, int) or a is None else ptr_of(a)  # noqa: E731
        out = self.d_out if out is None else out
        self.ctx.call("sdx_observe_dev", int(n), addr(d_lambdas), addr(d_flux), addr(reference), self.n_pix, self.d_edges.ptr,
                      self.d_sigma.ptr, self.d_doppler.ptr, out.ptr)
        return out

    def observe_host(self, lambdas, flux, reference=None):
        """numpy in, numpy out: (n,) wavelengths (ascending, Angstrom) and flux -> (n_pix,)."""
        lam = np.ascontiguousarray(getattr(lambdas, "value", lambdas), dtype=np.float64).reshape(-1)
        f = np.ascontiguousarray(getattr(flux, "value", flux), dtype=np.float64).reshape(-1)
        _ascending("lambdas", lam)
        if lam.size < 2 or f.size != lam.size:
            raise ValueError("lambdas and flux must hold the same number of points, at least two")
        d_ref = None
        if reference is not None:
            g = np.ascontiguousarray(getattr(reference, "value", reference), dtype=np.float64).reshape(-1)
            if g.size != lam.size:
                raise ValueError("reference must hold one value per grid point")
            d_ref = self.ctx.upload(g)
        d_lam, d_f = self.ctx.upload(lam), self.ctx.upload(f)
        return self.observe(d_lam, d_f, lam.size, d_ref).numpy()

    def adjoint(self, d_lambdas, n, pixel_weights, flux=None, reference=None, nus=None, out=None, out_reference=None):
        """The transpose of observe() (sdx_observe_adjoint_dev): pixel_weights c (n_pix,) on the device -> the DeviceArray (n,) of
        weights w over the grid points with  sum_j c_j observe(flux)_j = sum_i w_i flux_i  over the covered pixels (c of a NaN pixel
        is never read).  With a reference (which needs `flux`: the normalised pixel value enters) the weights are those of the
        normalised spectrum to the flux, and out_reference — given, or asked for with out_reference=True — receives the weights to
        the reference; then -> (w, w_reference).  nus: the grid's frequencies; the weights then apply to F_nu instead of F_lambda
        (the transpose of sdx_flux_nu_to_lambda_dev).  Device buffers in (DeviceArrays, CUDA tensors or raw addresses), enqueued on
        the context's stream: nothing waits, and nothing is allocated when `out` (and out_reference) are given."""
        addr = lambda a: a if isinstance(a, int) or a is None else ptr_of(a)  # noqa: E731
        if reference is None and out_reference is not None and out_reference is not False:
            raise ValueError("out_reference needs a reference")
        if reference is not None and flux is None:
            raise ValueError("a reference needs the flux: the normalised pixel value enters the weights")
        out = self.ctx.empty((int(n),)) if out is None else out
        if out_reference is True:
            out_reference = self.ctx.empty((int(n),))
        elif out_reference is False:
            out_reference = None
        self.ctx.call("sdx_observe_adjoint_dev", int(n), addr(d_lambdas), addr(flux) if reference is not None else None, addr(reference),
                      self.n_pix, self.d_edges.ptr, self.d_sigma.ptr, self.d_doppler.ptr, addr(pixel_weights), addr(nus), addr(out),
                      addr(out_reference))
        return out if out_reference is None else (out, out_reference)

    def adjoint_host(self, lambdas, pixel_weights, flux=None, reference=None, nus=None):
        """numpy in, numpy out: (n,) wavelengths and (n_pix,) pixel weights -> (n,) weights over the grid points; with a reference
        (and the flux) -> (weights to the flux, weights to the reference).  The host-buffer twin sdx_observe_adjoint_f64, which
        checks the arrays as observe_host's does."""
        lam, c, f, g, nu = adjoint_host_arguments(self.n_pix, lambdas, pixel_weights, flux, reference, nus)
        host = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        w = np.empty(lam.size)
        w_ref = np.empty(lam.size) if g is not None else None
        self.ctx.call("sdx_observe_adjoint_f64", lam.size, host(lam), host(f), host(g), self.n_pix, host(self.edges), host(self.sigma),
                      float(self.doppler), host(c), host(nu), host(w), host(w_ref))
        return w if w_ref is None else (w, w_ref)
