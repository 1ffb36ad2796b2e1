"""The instrument model on the device: radial-velocity shift, a Gaussian line-spread function whose width is given per pixel, and
integration over the detector's pixels — one launch of k_observe behind the synthesis (include/stardis_hip.h, sdx_observe_dev, states
the operator).  The reference has no counterpart; its rotation-broadening walk-through applies scipy.ndimage.gaussian_filter1d at one
sigma in grid points (postprocess.gaussian_filter1d mirrors that), which is a constant resolving power on a log-uniform grid only.
Instrument.adjoint is the operator transposed (sdx_observe_adjoint_dev): weights over the pixels pulled back to weights over the grid.
With v_rot the star's rotation (v sin i, Gray's profile with linear limb darkening; sdx_rotate_dev states the operator) is applied on
the rest-frame grid in front of k_observe, in velocity space on any ascending grid, and its transpose behind the instrument's: one more
launch forward, two more transposed.  postprocess.rotation_broadening, which mirrors the reference, is another thing: a kernel at
integer pixel offsets, a rotation profile on a log-uniform grid only.
With v_mac the radial-tangential macroturbulence zeta (sdx_macroturbulence_dev states the operator) follows the rotation and precedes
k_observe — the order is rotate -> macroturbulence -> observe, and the adjoint runs it in reverse; both broadenings are convolutions in
velocity, so on a log-uniform grid the order does not matter, and elsewhere this one is the definition.
Forward mode — one direction, every pixel — is Instrument.tangent (the Jacobian-vector product of observe(): sdx_observe_tangent_dev
behind the broadening stages, which carry a tangent as a (flux, reference) pair of their own) and Instrument.parameter_tangents (the
columns to the radial velocity, the line-spread function's width, zeta and the limb darkening); both on demand, with scratch of their
own that an instrument which never asks does not have."""
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


def _addr(a):
    """a device buffer's address: a DeviceArray or CUDA tensor through ptr_of, a raw address or None as it is"""
    return a if isinstance(a, int) or a is None else ptr_of(a)


def _host_ptr(a):
    return None if a is None else a.ctypes.data


def _grid(lambdas):
    """-> the grid as a contiguous fp64 vector, validated (ValueError): finite, strictly ascending, at least two points"""
    lam = np.ascontiguousarray(getattr(lambdas, "value", lambdas), dtype=np.float64).reshape(-1)
    _ascending("lambdas", lam)
    if lam.size < 2:
        raise ValueError("lambdas must hold at least two points")
    return lam


def _public(outs):
    """what a stage returns to the caller: the arrays that exist, the flux alone where it is the only one"""
    res = tuple(a for a in outs if a is not None)
    return res[0] if len(res) == 1 else res


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


def rotation_pair(v_rot, limb_darkening=0.6):
    """-> (V, eps) as floats, validated as sdx_rotate_f64 validates them: v sin i finite with 0 <= V < 3000 km/s, the linear
    limb-darkening coefficient in [0, 1].  Needs no device."""
    try:
        V, eps = float(getattr(v_rot, "value", v_rot)), float(limb_darkening)
    except (TypeError, ValueError):
        raise ValueError("v_rot and limb_darkening must be numbers") from None
    if not (math.isfinite(V) and 0.0 <= V < 3000.0):
        raise ValueError("v_rot must be finite with 0 <= v_rot < 3000 km/s")
    if not 0.0 <= eps <= 1.0:
        raise ValueError("limb_darkening must lie in [0, 1]")
    return V, eps


def macroturbulence_zeta(v_mac):
    """-> zeta as a float, validated as sdx_macroturbulence_f64 validates it: finite with 0 <= zeta < 500 km/s.  Needs no device."""
    try:
        zeta = float(getattr(v_mac, "value", v_mac))
    except (TypeError, ValueError):
        raise ValueError("v_mac must be a number") from None
    if not (math.isfinite(zeta) and 0.0 <= zeta < 500.0):
        raise ValueError("v_mac must be finite with 0 <= v_mac < 500 km/s")
    return zeta


MACROTURBULENCE_REACH = 6.0  # the profile's window in units of zeta (K(6) = 3e-18 of the peak)


def _host_vector(name, a, n, what):
    v = np.ascontiguousarray(getattr(a, "value", a), dtype=np.float64).reshape(-1)
    if v.size != n:
        raise ValueError(f"{name} must hold one value per {what} ({n}), got {v.size}")
    return v


def adjoint_host_arguments(n_pix, lambdas, pixel_weights, flux=None, reference=None, nus=None):
    """The host arrays of Instrument.adjoint_host, validated (ValueError naming the argument; needs no device) ->
    (lambdas, pixel_weights, flux, reference, nus), the optional ones None where not given."""
    lam = _grid(lambdas)
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
    graph that recorded it follows set_radial_velocity() without being recorded again (the kernel reads the factor from device memory).
    v_rot (km/s; None: no rotation, and nothing below exists or runs) and limb_darkening: the star's v sin i and linear limb-darkening
    coefficient.  The pair lives on the device like the Doppler factor (set_rotation); observe() then broadens flux and reference
    into scratch of the instrument's (k_rotate, sized at first use or by reserve(n)) and observes that.  A rotation window that reaches
    past an end of the grid is truncated and renormalised: edge_affected() names the pixels that see such points.
    v_mac (km/s; None: no macroturbulence, and nothing of it exists or runs): the radial-tangential macroturbulence zeta, one more
    device scalar (set_macroturbulence) and one more stage (k_macroturbulence) between the rotation and the pixels, with the same
    scratch rules and the same treatment of the grid's ends.
    rotation: "sampled" (the default: k_rotate, Gray's profile at the grid points under trapezoid weights) or "integrated"
    (k_rotate_integrated: the profile integrated exactly against the piecewise-linear flux, cell by cell; sdx_rotate_integrated_dev
    states the operator).  The mode routes every call that rotates — forward, adjoint and tangents — and only the integrated one has
    the column "v_rot" of parameter_tangents: it is differentiable in v sin i and tends to the identity as v sin i -> 0."""

    ROTATION_MODES = ("sampled", "integrated")
    rotation, v_mac = ROTATION_MODES[0], None  # (the class's defaults; __init__ sets the instance's)

    def __init__(self, pixel_edges, resolving_power=None, sigma=None, ctx=None, v_rot=None, limb_darkening=0.6, v_mac=None,
                 rotation="sampled"):
        self.edges, self.sigma = pixel_sigma(pixel_edges, resolving_power, sigma)  # (ValueError before any device work)
        if rotation not in self.ROTATION_MODES:
            raise ValueError(f"rotation must be one of {', '.join(self.ROTATION_MODES)}, got {rotation!r}")
        self.rotation = rotation
        self.rotates = v_rot is not None
        pair = rotation_pair(v_rot, limb_darkening) if self.rotates else None
        self.macroturbulent = v_mac is not None
        zeta = macroturbulence_zeta(v_mac) if self.macroturbulent else None
        self.broadens = self.rotates or self.macroturbulent  # a stage in front of k_observe
        self.n_pix = self.edges.size - 1
        self.ctx = ctx or default_context()
        self.d_edges = self.ctx.upload(self.edges)
        self.d_sigma = self.ctx.upload(self.sigma)
        self.d_doppler = self.ctx.empty((1,))
        self.d_out = self.ctx.empty((self.n_pix,))
        self.set_radial_velocity(0.0)
        self.v_rot, self.limb_darkening = None, float(limb_darkening)
        self._scratch_n, self._scratch, self._tangent_n = 0, None, 0
        if self.rotates:
            self.d_rot = self.ctx.empty((2,))
            self.set_rotation(*pair)
        self.v_mac = None
        if self.macroturbulent:
            self.d_mac = self.ctx.empty((1,))
            self.set_macroturbulence(zeta)

    def set_rotation(self, v_rot, limb_darkening=None):
        """Write (v sin i, limb darkening) into the device pair, in order on the context's stream; limb_darkening=None keeps the
        present coefficient.  Only for an instrument constructed with v_rot (0 allowed)."""
        if not self.rotates:
            raise RuntimeError("no rotation: construct the Instrument with v_rot= (0 allowed)")
        V, eps = rotation_pair(v_rot, self.limb_darkening if limb_darkening is None else limb_darkening)
        self.d_rot.set(np.array([V, eps]))
        self.v_rot, self.limb_darkening = V, eps

    def set_macroturbulence(self, zeta):
        """Write zeta (km/s) into the device scalar, in order on the context's stream.  Only for an instrument constructed with v_mac
        (0 allowed)."""
        if not self.macroturbulent:
            raise RuntimeError("no macroturbulence: construct the Instrument with v_mac= (0 allowed)")
        zeta = macroturbulence_zeta(zeta)
        self.d_mac.set(np.array([zeta]))
        self.v_mac = zeta

    def reserve(self, n):
        """Size the broadening stages' scratch for grids of up to n points now (per stage: broadened flux and reference, and the
        adjoint's two intermediate weight vectors), so that a later observe() or adjoint() — inside a graph capture, say — allocates
        nothing.  Without rotation and macroturbulence there is no scratch and this does nothing."""
        n = int(n)
        if self.broadens and n > self._scratch_n:
            self._scratch = tuple(self.ctx.empty((n,)) for _ in range(4 * (self.rotates + self.macroturbulent)))
            self._scratch_n = n

    def _pair(self, k, adjoint=False):
        """the scratch pair of the instrument's k-th stage (rotation first): its broadened (flux, reference), or, with adjoint, the
        k-th intermediate (weights, weights to the reference) of adjoint()"""
        first = 4 * k + 2 * adjoint
        return self._scratch[first], self._scratch[first + 1]

    def _stage_out(self, k, n, reference, out, out_reference):
        """where the k-th stage writes: the caller's buffers, else its scratch pair (sized here at first use); out_reference only with
        a reference"""
        self.reserve(n)
        s, s_ref = self._pair(k)
        return s if out is None else out, None if reference is None else (s_ref if out_reference is None else out_reference)

    def _integrated(self):
        """the rotation stage is the cell-integrated one"""
        return self.rotation == "integrated"

    def _stages(self):
        """the stages the instrument has, in their order: (0: rotation / 1: macroturbulence, the stage on device buffers, on host arrays)"""
        return ((0, self._rotate, self._rotate_host),) * self.rotates + ((1, self._macroturbulence, self._macroturbulence_host),) * self.macroturbulent

    def _rotate(self, d_lambdas, n, flux, reference, out=None, out_reference=None):
        """rotate() -> (out, out_reference or None)"""
        out, out_reference = self._stage_out(0, n, reference, out, out_reference)
        derivatives = (None,) * 4 if self._integrated() else ()
        self.ctx.call("sdx_rotate_integrated_dev" if self._integrated() else "sdx_rotate_dev", int(n), _addr(d_lambdas), _addr(flux),
                      _addr(reference), self.d_rot.ptr, _addr(out), _addr(out_reference), *derivatives)
        return out, out_reference

    def rotate(self, d_lambdas, d_flux, n, reference=None, out=None, out_reference=None):
        """The rotation stage alone (sdx_rotate_dev): n points of (rest-frame wavelength, flux[, reference]) on the device -> the
        broadened flux, or (flux, reference) with a reference; into the instrument's scratch unless `out` (and out_reference) are given."""
        if not self.rotates:
            raise RuntimeError("no rotation: construct the Instrument with v_rot= (0 allowed)")
        return _public(self._rotate(d_lambdas, n, d_flux, reference, out, out_reference))

    def _rotate_host(self, lam, f, g):
        """rotate_host() -> [out, out_reference or None]"""
        entry, n_outs = ("sdx_rotate_integrated_f64", 6) if self._integrated() else ("sdx_rotate_f64", 2)
        return _stage_host(self.ctx, entry, lam, f, g, (self.v_rot, self.limb_darkening), n_outs, 2)

    def rotate_host(self, lambdas, flux, reference=None):
        """numpy in, numpy out (sdx_rotate_f64, which checks the arrays): -> the broadened flux, or (flux, reference)."""
        if not self.rotates:
            raise RuntimeError("no rotation: construct the Instrument with v_rot= (0 allowed)")
        return _public(self._rotate_host(lambdas, flux, reference))

    def _macroturbulence(self, d_lambdas, n, flux, reference, out=None, out_reference=None, dout=None, dout_reference=None):
        """macroturbulence() -> (out, out_reference or None)"""
        out, out_reference = self._stage_out(int(self.rotates), n, reference, out, out_reference)  # (behind the rotation's scratch)
        self.ctx.call("sdx_macroturbulence_dev", int(n), _addr(d_lambdas), _addr(flux), _addr(reference), self.d_mac.ptr, _addr(out),
                      _addr(out_reference), _addr(dout), _addr(dout_reference))
        return out, out_reference

    def macroturbulence(self, d_lambdas, d_flux, n, reference=None, out=None, out_reference=None, dout=None, dout_reference=None):
        """The macroturbulence stage alone (sdx_macroturbulence_dev): n points of (rest-frame wavelength, flux[, reference]) on the
        device -> the broadened flux, or (flux, reference) with a reference; into the instrument's scratch unless `out` (and
        out_reference) are given.  dout (and dout_reference, with a reference): buffers that receive d out / d ln zeta from the
        same launch."""
        if not self.macroturbulent:
            raise RuntimeError("no macroturbulence: construct the Instrument with v_mac= (0 allowed)")
        return _public(self._macroturbulence(d_lambdas, n, d_flux, reference, out, out_reference, dout, dout_reference))

    def _macroturbulence_host(self, lam, f, g, derivative=False):
        """macroturbulence_host() -> [out, out_reference or None], with derivative [.., dout, dout_reference or None]"""
        return _stage_host(self.ctx, "sdx_macroturbulence_f64", lam, f, g, (self.v_mac,), 4, 4 if derivative else 2)

    def macroturbulence_host(self, lambdas, flux, reference=None, derivative=False):
        """numpy in, numpy out (sdx_macroturbulence_f64, which checks the arrays): -> the broadened flux, or (flux, reference);
        derivative=True appends d / d ln zeta of each."""
        if not self.macroturbulent:
            raise RuntimeError("no macroturbulence: construct the Instrument with v_mac= (0 allowed)")
        return _public(self._macroturbulence_host(lambdas, flux, reference, derivative))

    def _broaden(self, d_lambdas, n, flux, reference):
        """broaden() -> (flux, reference or None)"""
        for _, stage, _ in self._stages():
            flux, reference = stage(d_lambdas, n, flux, reference)
        return flux, reference

    def broaden(self, d_lambdas, d_flux, n, reference=None):
        """The stages in front of k_observe in their order — rotation, then macroturbulence, whichever the instrument has — into the
        instrument's scratch -> the broadened flux, or (flux, reference) with a reference: what observe(..., broadened=True) takes."""
        return _public(self._broaden(d_lambdas, n, d_flux, reference))

    def _broaden_host(self, lam, f, g):
        """broaden() through the host-buffer twins -> (flux, reference or None)"""
        for _, _, stage in self._stages():
            f, g = stage(lam, f, g)
        return f, g

    def edge_affected(self, lambdas, v_rot=None):
        """-> boolean host array (n_pix,): the pixels whose window [edges[j] - 8 sigma[j], edges[j+1] + 8 sigma[j]], taken back to the
        rest frame, comes within the broadening's reach of an end of the grid `lambdas` — lo (1 - beta) < lambdas[0] or hi (1 + beta) >
        lambdas[-1], beta = (v_rot + 6 v_mac) / c the combined reach of rotation and macroturbulence — so that a window of a point
        they may see is truncated there.  Without either (beta = 0) these are the pixels the grid does not cover.  v_rot: a rotation
        (km/s) in the place of the instrument's own — the disk integration's, which is no stage of the instrument; None: the
        instrument's.  Plain numpy."""
        lam = _grid(lambdas)
        rot = (self.v_rot or 0.0) if v_rot is None else float(v_rot)
        beta = rot / K.C_KMS
        if self.v_mac:
            beta = (rot + MACROTURBULENCE_REACH * self.v_mac) / K.C_KMS
        lo = (self.edges[:-1] - 8.0 * self.sigma) / self.doppler
        hi = (self.edges[1:] + 8.0 * self.sigma) / self.doppler
        return (lo * (1.0 - beta) < lam[0]) | (hi * (1.0 + beta) > lam[-1])

    def set_radial_velocity(self, v_kms):
        """Write the Doppler factor of v_kms into the device scalar, in order on the context's stream."""
        D = doppler_factor(v_kms)
        self.d_doppler.set(np.array([D]))
        self.v_kms, self.doppler = float(v_kms), D

    def observe(self, d_lambdas, d_flux, n, reference=None, out=None, broadened=False):
        """n points of (wavelength, flux[, reference]) already on the device (DeviceArrays, CUDA tensors or raw addresses) -> the
        DeviceArray (n_pix,) of the instrument (or `out`), enqueued on the context's stream: nothing is allocated, nothing waits.
        With rotation or macroturbulence, flux and reference are broadened first (broaden(), into the scratch: sized here at first
        use, or by reserve(n)); broadened=True says they are already — what broaden() returned — so that several outputs share one
        k_rotate and one k_macroturbulence."""
        out = self.d_out if out is None else out
        if self.broadens and not broadened:
            d_flux, reference = self._broaden(d_lambdas, n, d_flux, reference)
        self.ctx.call("sdx_observe_dev", int(n), _addr(d_lambdas), _addr(d_flux), _addr(reference), self.n_pix, self.d_edges.ptr,
                      self.d_sigma.ptr, self.d_doppler.ptr, out.ptr)
        return out

    def observe_host(self, lambdas, flux, reference=None):
        """numpy in, numpy out: (n,) wavelengths (ascending, Angstrom) and flux -> (n_pix,)."""
        lam = _grid(lambdas)
        f = np.ascontiguousarray(getattr(flux, "value", flux), dtype=np.float64).reshape(-1)
        if f.size != lam.size:
            raise ValueError("lambdas and flux must hold the same number of points, at least two")
        d_ref = None
        if reference is not None:
            g = np.ascontiguousarray(getattr(reference, "value", reference), dtype=np.float64).reshape(-1)
            if g.size != lam.size:
                raise ValueError("reference must hold one value per grid point")
        if self.broadens:  # (the host-buffer twins, then the pixels as without them)
            f, g = self._broaden_host(lam, f, g if reference is not None else None)
        if reference is not None:
            d_ref = self.ctx.upload(g)
        d_lam, d_f = self.ctx.upload(lam), self.ctx.upload(f)
        return self.observe(d_lam, d_f, lam.size, d_ref, broadened=True).numpy()

    def adjoint(self, d_lambdas, n, pixel_weights, flux=None, reference=None, nus=None, out=None, out_reference=None):
        """The transpose of observe() (sdx_observe_adjoint_dev): pixel_weights c (n_pix,) on the device -> the DeviceArray (n,) of
        weights w over the grid points with  sum_j c_j observe(flux)_j = sum_i w_i flux_i  over the covered pixels (c of a NaN pixel
        is never read).  With a reference (which needs `flux`: the normalised pixel value enters) the weights are those of the
        normalised spectrum to the flux, and out_reference — given, or asked for with out_reference=True — receives the weights to
        the reference; then -> (w, w_reference).  nus: the grid's frequencies; the weights then apply to F_nu instead of F_lambda
        (the transpose of sdx_flux_nu_to_lambda_dev).  Device buffers in (DeviceArrays, CUDA tensors or raw addresses), enqueued on
        the context's stream: nothing waits, and nothing is allocated when `out` (and out_reference) are given.
        With rotation the chain is transposed stage by stage: flux and reference are broadened here (the normalised pixel value
        enters), sdx_observe_adjoint_dev gives the weights over the BROADENED points, and sdx_rotate_adjoint_dev takes those back to
        the grid and applies nus — three stages where there was one, the scratch the instrument's (reserve(n)).  With
        macroturbulence sdx_macroturbulence_adjoint_dev stands between the two (the forward order reversed); the last stage applies nus."""
        if reference is None and out_reference is not None and out_reference is not False:
            raise ValueError("out_reference needs a reference")
        if reference is not None and flux is None:
            raise ValueError("a reference needs the flux: the normalised pixel value enters the weights")
        out = self.ctx.empty((int(n),)) if out is None else out
        if out_reference is True:
            out_reference = self.ctx.empty((int(n),))
        elif out_reference is False:
            out_reference = None
        if self.broadens:
            self.reserve(n)
            if reference is not None:
                flux, reference = self._broaden(d_lambdas, n, flux, reference)
            normal = out_reference is not None
            u, u_ref = self._pair(0, adjoint=True)
            u_ref = u_ref if normal else None
            self.ctx.call("sdx_observe_adjoint_dev", int(n), _addr(d_lambdas), _addr(flux) if reference is not None else None, _addr(reference),
                          self.n_pix, self.d_edges.ptr, self.d_sigma.ptr, self.d_doppler.ptr, _addr(pixel_weights), None, u.ptr, _addr(u_ref))
            if self.macroturbulent:
                last = not self.rotates  # (the last stage writes the caller's buffers and applies nus)
                t, t_ref = (out, out_reference) if last else self._pair(1, adjoint=True)
                t_ref = t_ref if normal else None
                self.ctx.call("sdx_macroturbulence_adjoint_dev", int(n), _addr(d_lambdas), self.d_mac.ptr, u.ptr, _addr(u_ref),
                              _addr(nus) if last else None, _addr(t), _addr(t_ref))
                u, u_ref = t, t_ref
            if self.rotates:
                self.ctx.call("sdx_rotate_integrated_adjoint_dev" if self._integrated() else "sdx_rotate_adjoint_dev", int(n), _addr(d_lambdas),
                              self.d_rot.ptr, u.ptr, _addr(u_ref), _addr(nus), _addr(out), _addr(out_reference))
            return out if out_reference is None else (out, out_reference)
        self.ctx.call("sdx_observe_adjoint_dev", int(n), _addr(d_lambdas), _addr(flux) if reference is not None else None, _addr(reference),
                      self.n_pix, self.d_edges.ptr, self.d_sigma.ptr, self.d_doppler.ptr, _addr(pixel_weights), _addr(nus), _addr(out),
                      _addr(out_reference))
        return out if out_reference is None else (out, out_reference)

    # -- forward mode: tangents of observe() ----------------------------------------------------------------------------------------
    PARAMETERS = ("v_rad", "lsf", "v_mac", "limb_darkening")
    INTEGRATED_PARAMETERS = ("v_rot",)  # only with rotation="integrated"

    def reserve_tangent(self, n):
        """Size the scratch of tangent() and parameter_tangents() for grids of up to n points now: per broadening stage the tangent
        pair that goes through it, and one pair for a stage's own parameter derivative.  Made at the first tangent call otherwise;
        an instrument that never asks has none, and reserve() keeps its sizes.  Without rotation and macroturbulence there is none."""
        n = int(n)
        self.reserve(n)
        if self.broadens and n > self._tangent_n:
            self._tangent_scratch = tuple(self.ctx.empty((n,)) for _ in range(2 * (self.rotates + self.macroturbulent) + 2))
            self._tangent_n = n

    def _tangent_pair(self, k):
        """the tangent scratch: the pair that leaves the instrument's k-th stage; k = -1: the pair of a stage's own parameter derivative"""
        return self._tangent_scratch[2 * k], self._tangent_scratch[2 * k + 1]

    def _push(self, d_lambdas, n, dflux, dreference, first_stage=0):
        """a tangent pair through the broadening stages from first_stage on (0: rotation, 1: macroturbulence), as a (flux, reference)
        pair of the stages themselves — they are linear in the flux and their denominators do not depend on it — into the tangent
        scratch -> (dflux, dreference or None) at the pixel stage's input"""
        for k, (index, stage, _) in enumerate(self._stages()):
            if index >= first_stage:
                dflux, dreference = stage(d_lambdas, n, dflux, dreference, *self._tangent_pair(k))
        return dflux, dreference

    def _observe_tangent(self, d_lambdas, n, flux, reference, dflux=None, dreference=None, out=None, dout_velocity=None, dout_lsf=None,
                         dout_flux=None):
        self.ctx.call("sdx_observe_tangent_dev", int(n), _addr(d_lambdas), _addr(flux), _addr(reference), self.n_pix, self.d_edges.ptr,
                      self.d_sigma.ptr, self.d_doppler.ptr, _addr(dflux), _addr(dreference), _addr(out), _addr(dout_velocity), _addr(dout_lsf),
                      _addr(dout_flux))

    def tangent(self, d_lambdas, n, flux, dflux, reference=None, dreference=None, out=None):
        """The Jacobian-vector product of observe(): the direction (dflux, dreference) of (flux, reference) on the grid -> the
        DeviceArray (n_pix,) (or `out`) of d observe(flux)_j, or of the normalised spectrum's tangent (sum w dflux - out_j sum w
        dreference) / den_j with a reference (dreference=None: the reference does not move).  NaN where observe() is NaN.  Rotation
        and macroturbulence are linear in the flux with denominators that do not depend on it, so the pair goes through each stage
        as a (flux, reference) pair of rotate() / macroturbulence() — one more launch per stage — and the pixel stage is
        sdx_observe_tangent_dev's dout_flux.  Device buffers in, enqueued on the context's stream; the scratch is made at the first
        call or by reserve_tangent(n), so a captured call allocates nothing when `out` is given, and follows set_radial_velocity()."""
        if dreference is not None and reference is None:
            raise ValueError("dreference needs a reference")
        if dflux is None:
            raise ValueError("tangent() needs dflux, the direction of the flux")
        out = self.ctx.empty((self.n_pix,)) if out is None else out
        if self.broadens:
            self.reserve_tangent(n)
            flux, reference = self._broaden(d_lambdas, n, flux, reference)
            dflux, dreference = self._push(d_lambdas, n, dflux, dreference)
        self._observe_tangent(d_lambdas, n, flux, reference, dflux, dreference, dout_flux=out)
        return out

    def _wrt(self, wrt):
        if wrt is None:  # every parameter this instrument has
            return ("v_rad", "lsf") + (("v_mac",) if self.macroturbulent and self.v_mac > 0.0 else ()) + (
                ("limb_darkening",) if self.rotates and self.v_rot > 0.0 else ()) + (
                self.INTEGRATED_PARAMETERS if self._integrated() and self.rotates and self.v_rot > 0.0 else ())
        names = (wrt,) if isinstance(wrt, str) else tuple(wrt)
        for name in names:
            if name in self.INTEGRATED_PARAMETERS:
                if not self._integrated():
                    raise ValueError(f'{name!r} needs the cell-integrated rotation profile: construct the Instrument with '
                                     'rotation="integrated" (the sampled sum has a square-root kink in v sin i wherever a point enters a window); '
                                     f"in the sampled mode wrt takes {', '.join(self.PARAMETERS)}")
            elif name not in self.PARAMETERS:
                raise ValueError(f"unknown parameter {name!r}: wrt takes {', '.join(self.PARAMETERS)}"
                                 f' (and {", ".join(self.INTEGRATED_PARAMETERS)} with rotation="integrated")')
        if "v_rot" in names:
            if not self.rotates:
                raise RuntimeError("no rotation: construct the Instrument with v_rot=")
            if not self.v_rot > 0.0:
                raise ValueError("the derivative to v sin i needs v_rot > 0 (at v_rot = 0 the stage is a copy)")
        if "v_mac" in names:
            if not self.macroturbulent:
                raise RuntimeError("no macroturbulence: construct the Instrument with v_mac=")
            if not self.v_mac > 0.0:
                raise ValueError("the derivative to zeta needs zeta > 0 (at zeta = 0 the stage is a copy)")
        if "limb_darkening" in names:
            if not self.rotates:
                raise RuntimeError("no rotation: construct the Instrument with v_rot=")
            if not self.v_rot > 0.0:
                raise ValueError("the derivative to the limb darkening needs v_rot > 0 (at v_rot = 0 the stage is a copy)")
        return names

    def parameter_tangents(self, d_lambdas, n, flux, reference=None, wrt=None):
        """-> {name: DeviceArray (n_pix,)}: the columns d observe(flux[, reference])_j / d p of the instrument's own parameters at
        fixed windows, NaN where observe() is NaN.
          "v_rad"           per km/s of the radial velocity   (sdx_observe_tangent_dev's dout_velocity)
          "lsf"             per ln kappa of a common factor kappa on every sigma; for a resolving power, -d / d ln R   (dout_lsf)
          "v_mac"           per km/s of zeta: k_macroturbulence's d / d ln zeta over zeta, through the pixel stage as a tangent
          "limb_darkening"  per unit of eps: k_rotate_tangent's d / d eps through the macroturbulence and the pixel stage
          "v_rot"           per km/s of v sin i, with rotation="integrated" only: k_rotate_integrated's exact d / d ln V over V, through
                            the macroturbulence and the pixel stage; "limb_darkening" then comes from the same launch
        In the sampled mode v sin i has no such column: on the trapezoid sum the forward model has a square-root kink in V wherever a
        point enters a window.  wrt=None: every column this instrument has.
        Unknown names are a ValueError; "v_mac" needs
        Instrument(v_mac > 0), "limb_darkening" Instrument(v_rot > 0).  On demand: it allocates its outputs (and the tangent scratch
        at the first call) and runs the stages in front of the pixels again."""
        names = self._wrt(wrt)
        res = {name: self.ctx.empty((self.n_pix,)) for name in names}
        normal = reference is not None
        d_par = d_par_ref = None  # a stage's own parameter derivative
        if self.broadens:
            self.reserve_tangent(n)
            d_par, d_par_ref = self._tangent_pair(-1)
            d_par_ref = d_par_ref if normal else None
        f, g = flux, reference
        eps_f = eps_g = None  # d / d eps at the pixel stage's input
        lnv_f = lnv_g = None  # d / d ln v_rot at the pixel stage's input
        want_eps, want_v = "limb_darkening" in names, "v_rot" in names  # (_wrt: "v_rot" with the integrated profile only)
        if self.rotates and (want_eps or want_v):
            # one launch gives the broadened pair and the derivatives: k_rotate_integrated both, k_rotate_tangent d / d eps
            rf, rg = self._pair(0)
            rg = rg if normal else None
            if self._integrated():
                d_lnv, d_lnv_ref = (self.ctx.empty((int(n),)), self.ctx.empty((int(n),)) if normal else None) if want_v else (None, None)
                self.ctx.call("sdx_rotate_integrated_dev", int(n), _addr(d_lambdas), _addr(f), _addr(g), self.d_rot.ptr, rf.ptr, _addr(rg),
                              _addr(d_lnv), _addr(d_lnv_ref), d_par.ptr if want_eps else None, _addr(d_par_ref) if want_eps else None)
            else:
                self.ctx.call("sdx_rotate_tangent_dev", int(n), _addr(d_lambdas), _addr(f), _addr(g), self.d_rot.ptr, rf.ptr, _addr(rg),
                              d_par.ptr, _addr(d_par_ref))
            f, g = rf, rg
            if want_eps:
                # (through the macroturbulence now: its own derivative takes the pair's place in the scratch below)
                eps_f, eps_g = self._push(d_lambdas, n, d_par, d_par_ref, first_stage=1)
            if want_v:
                lnv_f, lnv_g = d_lnv, d_lnv_ref
                if self.macroturbulent:  # (buffers of its own: the tangent scratch holds the limb darkening's pair)
                    t, t_ref = self.ctx.empty((int(n),)), self.ctx.empty((int(n),)) if normal else None
                    lnv_f, lnv_g = self._macroturbulence(d_lambdas, n, d_lnv, d_lnv_ref, out=t, out_reference=t_ref)
        elif self.rotates:
            f, g = self._rotate(d_lambdas, n, f, g)
        if self.macroturbulent:
            want = "v_mac" in names
            f, g = self._macroturbulence(d_lambdas, n, f, g, dout=d_par if want else None, dout_reference=d_par_ref if want else None)
            if want:
                per_ln, zeta = self.ctx.empty((self.n_pix,)), self.ctx.upload(np.full(self.n_pix, self.v_mac))
                self._observe_tangent(d_lambdas, n, f, g, d_par, d_par_ref, dout_flux=per_ln)
                self.ctx.call("sdx_divide_dev", self.n_pix, per_ln.ptr, zeta.ptr, res["v_mac"].ptr)
        if eps_f is not None:
            self._observe_tangent(d_lambdas, n, f, g, eps_f, eps_g, dout_flux=res["limb_darkening"])
        if lnv_f is not None:
            per_ln, V = self.ctx.empty((self.n_pix,)), self.ctx.upload(np.full(self.n_pix, self.v_rot))
            self._observe_tangent(d_lambdas, n, f, g, lnv_f, lnv_g, dout_flux=per_ln)
            self.ctx.call("sdx_divide_dev", self.n_pix, per_ln.ptr, V.ptr, res["v_rot"].ptr)
        if "v_rad" in names or "lsf" in names:
            self._observe_tangent(d_lambdas, n, f, g, dout_velocity=res.get("v_rad"), dout_lsf=res.get("lsf"))
        return res

    def tangent_host(self, lambdas, flux, dflux, reference=None, dreference=None):
        """numpy in, numpy out: tangent() through the host-buffer twins (sdx_rotate_f64, sdx_macroturbulence_f64,
        sdx_observe_tangent_f64, which check the arrays) -> (n_pix,)."""
        if dreference is not None and reference is None:
            raise ValueError("dreference needs a reference")
        lam = _grid(lambdas)
        f, df = _host_vector("flux", flux, lam.size, "grid point"), _host_vector("dflux", dflux, lam.size, "grid point")
        g = None if reference is None else _host_vector("reference", reference, lam.size, "grid point")
        dg = None if dreference is None else _host_vector("dreference", dreference, lam.size, "grid point")
        if self.broadens:
            f, g = self._broaden_host(lam, f, g)
            df, dg = self._broaden_host(lam, df, dg)
        return self._observe_tangent_host(lam, f, g, df, dg, flux_tangent=True)[0]

    def _observe_tangent_host(self, lam, f, g, df=None, dg=None, velocity=False, lsf=False, flux_tangent=False):
        outs = [np.empty(self.n_pix) if on else None for on in (flux_tangent, velocity, lsf)]
        self.ctx.call("sdx_observe_tangent_f64", lam.size, _host_ptr(lam), _host_ptr(f), _host_ptr(g), self.n_pix, _host_ptr(self.edges),
                      _host_ptr(self.sigma), float(self.doppler), _host_ptr(df), _host_ptr(dg), None, _host_ptr(outs[1]), _host_ptr(outs[2]),
                      _host_ptr(outs[0]))
        return outs

    def parameter_tangents_host(self, lambdas, flux, reference=None, wrt=None):
        """numpy in, numpy out: parameter_tangents() through the host-buffer twins -> {name: (n_pix,)}."""
        names = self._wrt(wrt)
        lam = _grid(lambdas)
        f = _host_vector("flux", flux, lam.size, "grid point")
        g = None if reference is None else _host_vector("reference", reference, lam.size, "grid point")
        res = {}
        want_eps, want_v = "limb_darkening" in names, "v_rot" in names  # (_wrt: "v_rot" with the integrated profile only)
        if self.rotates and (want_eps or want_v):
            # one launch gives the broadened pair and the derivatives: k_rotate_integrated both, k_rotate_tangent d / d eps
            pair = (self.v_rot, self.limb_darkening)
            if self._integrated():
                bf, bg, vf, vg, ef, eg = _stage_host(self.ctx, "sdx_rotate_integrated_f64", lam, f, g, pair, 6, 6)
            else:
                bf, bg, ef, eg = _stage_host(self.ctx, "sdx_rotate_tangent_f64", lam, f, g, pair, 4, 4)
            through = (lambda a, b: self._macroturbulence_host(lam, a, b)) if self.macroturbulent else (lambda a, b: (a, b))
            mf, mg = through(bf, bg)
            if want_eps:
                res["limb_darkening"] = self._observe_tangent_host(lam, mf, mg, *through(ef, eg), flux_tangent=True)[0]
            if want_v:
                res["v_rot"] = self._observe_tangent_host(lam, mf, mg, *through(vf, vg), flux_tangent=True)[0] / self.v_rot
            f, g = (bf, bg) if self._integrated() else self._rotate_host(lam, f, g)
        elif self.rotates:
            f, g = self._rotate_host(lam, f, g)
        if self.macroturbulent:
            if "v_mac" in names:
                f, g, tf, tg = self._macroturbulence_host(lam, f, g, derivative=True)
                res["v_mac"] = self._observe_tangent_host(lam, f, g, tf, tg, flux_tangent=True)[0] / self.v_mac
            else:
                f, g = self._macroturbulence_host(lam, f, g)
        if "v_rad" in names or "lsf" in names:
            _, v, k = self._observe_tangent_host(lam, f, g, velocity="v_rad" in names, lsf="lsf" in names)
            if v is not None:
                res["v_rad"] = v
            if k is not None:
                res["lsf"] = k
        return {name: res[name] for name in names}

    def adjoint_host(self, lambdas, pixel_weights, flux=None, reference=None, nus=None):
        """numpy in, numpy out: (n,) wavelengths and (n_pix,) pixel weights -> (n,) weights over the grid points; with a reference
        (and the flux) -> (weights to the flux, weights to the reference).  The host-buffer twin sdx_observe_adjoint_f64, which
        checks the arrays as observe_host's does."""
        lam, c, f, g, nu = adjoint_host_arguments(self.n_pix, lambdas, pixel_weights, flux, reference, nus)
        w = np.empty(lam.size)
        w_ref = np.empty(lam.size) if g is not None else None
        if self.broadens:  # (the stages of adjoint(), each through its host-buffer twin)
            if g is not None:
                f, g = self._broaden_host(lam, f, g)
            u, u_ref = np.empty(lam.size), np.empty(lam.size) if g is not None else None
            self.ctx.call("sdx_observe_adjoint_f64", lam.size, _host_ptr(lam), _host_ptr(f), _host_ptr(g), self.n_pix, _host_ptr(self.edges), _host_ptr(self.sigma),
                          float(self.doppler), _host_ptr(c), None, _host_ptr(u), _host_ptr(u_ref))
            if self.macroturbulent:
                last = not self.rotates
                t, t_ref = (w, w_ref) if last else (np.empty(lam.size), np.empty(lam.size) if g is not None else None)
                self.ctx.call("sdx_macroturbulence_adjoint_f64", lam.size, _host_ptr(lam), self.v_mac, _host_ptr(u), _host_ptr(u_ref), _host_ptr(nu) if last else None,
                              _host_ptr(t), _host_ptr(t_ref))
                u, u_ref = t, t_ref
            if self.rotates:
                self.ctx.call("sdx_rotate_integrated_adjoint_f64" if self._integrated() else "sdx_rotate_adjoint_f64", lam.size, _host_ptr(lam),
                              self.v_rot, self.limb_darkening, _host_ptr(u), _host_ptr(u_ref), _host_ptr(nu), _host_ptr(w), _host_ptr(w_ref))
            return w if w_ref is None else (w, w_ref)
        self.ctx.call("sdx_observe_adjoint_f64", lam.size, _host_ptr(lam), _host_ptr(f), _host_ptr(g), self.n_pix, _host_ptr(self.edges), _host_ptr(self.sigma),
                      float(self.doppler), _host_ptr(c), _host_ptr(nu), _host_ptr(w), _host_ptr(w_ref))
        return w if w_ref is None else (w, w_ref)


def _stage_host(ctx, entry, lambdas, flux, reference, scalars, n_outs, wanted):
    """The host-buffer twin `entry` of a stage's forward entry, which takes n_outs grid-sized outputs in pairs (of the flux, of the
    reference), on host arrays that are checked here before any device work (ValueError naming the argument) -> the list of the first
    `wanted` outputs, None in place of a reference's where there is no reference"""
    lam = _grid(lambdas)
    f = _host_vector("flux", flux, lam.size, "grid point")
    g = None if reference is None else _host_vector("reference", reference, lam.size, "grid point")
    outs = [np.empty(lam.size) if k < wanted and (k % 2 == 0 or g is not None) else None for k in range(n_outs)]
    (ctx or default_context()).call(entry, lam.size, _host_ptr(lam), _host_ptr(f), _host_ptr(g), *scalars, *map(_host_ptr, outs))
    return outs[:wanted]


def rotate_host(ctx, lambdas, flux, v_rot, limb_darkening=0.6, reference=None):
    """Rotational broadening of host arrays (sdx_rotate_f64) -> the broadened flux, or (flux, reference) with a reference.  The
    arguments are checked before any device work (ValueError naming the argument)."""
    return _public(_stage_host(ctx, "sdx_rotate_f64", lambdas, flux, reference, rotation_pair(v_rot, limb_darkening), 2, 2))


def rotate_integrated_host(ctx, lambdas, flux, v_rot, limb_darkening=0.6, reference=None, derivatives=False):
    """The cell-integrated rotation of host arrays (sdx_rotate_integrated_f64) -> the broadened flux, or (flux, reference) with a
    reference; derivatives=True appends d / d ln v_rot and d / d limb_darkening of each: (out, dout_lnv, dout_eps), or (out,
    out_reference, dout_lnv, dout_lnv_reference, dout_eps, dout_eps_reference).  The arguments are checked before any device work."""
    pair = rotation_pair(v_rot, limb_darkening)
    return _public(_stage_host(ctx, "sdx_rotate_integrated_f64", lambdas, flux, reference, pair, 6, 6 if derivatives else 2))


def macroturbulence_host(ctx, lambdas, flux, zeta, reference=None, derivative=False):
    """Radial-tangential macroturbulence of host arrays (sdx_macroturbulence_f64) -> the broadened flux, or (flux, reference) with a
    reference; derivative=True appends d / d ln zeta of each (flux, dflux) or (flux, reference, dflux, dreference).  The arguments are
    checked before any device work (ValueError naming the argument)."""
    zeta = macroturbulence_zeta(zeta)
    return _public(_stage_host(ctx, "sdx_macroturbulence_f64", lambdas, flux, reference, (zeta,), 4, 4 if derivative else 2))
