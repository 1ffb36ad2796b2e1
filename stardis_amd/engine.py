"""Device-resident spectral synthesis: line opacity + continuum + formal solution for data already in HBM.

This is the path bench.py times and the one a frequency-sharded multi-GPU run uses: inputs are
uploaded once, every step is a handful of kernel launches on one stream (optionally replayed as a
hipGraph), and the only host traffic is the final flux.  Numerically it is the same sequence as
calc_alphas + raytrace in stardis_amd.radiation_field (and hence the reference's
radiation_field/base.py:104-115): total = ((((file + bf) + ff) + rayleigh) + electron) + line.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from . import constants as K
from . import linelist as LL
from . import ops
from ._lib import Continuum, default_context, ptr_of

LINE_WRT = ("strength", "damping", "doppler", "centre")  # wrt= of the line sensitivities; the last three: sdx_line_param_adjoint_dev's outputs


def shard_bounds(n_nu, world_size, rank):
    """Contiguous block of the GLOBAL frequency index owned by `rank`."""
    per = -(-n_nu // world_size)
    begin = min(rank * per, n_nu)
    return begin, min(per, n_nu - begin)


def _require_f64_buffer(name, buf, n_min):
    """A DeviceArray or contiguous CUDA tensor of at least n_min float64 values."""
    ptr_of(buf)  # (type, contiguity)
    if isinstance(buf, _lib.DeviceArray):
        dtype_ok, numel = buf.dtype == np.dtype(np.float64), int(np.prod(buf.shape, dtype=np.int64))
    else:
        dtype_ok, numel = str(buf.dtype) == "torch.float64", int(buf.numel())
    if not dtype_ok:
        raise TypeError(f"{name} must hold float64 values")
    if numel < n_min:
        raise ValueError(f"{name} holds {numel} values, {n_min} are needed")


class _DeviceRow(_lib.DeviceArray):
    """One row of a plane that another DeviceArray owns (held here, so that it outlives this): a DeviceArray that frees nothing."""

    def __init__(self, plane, row):
        self.ctx, self.owner = plane.ctx, plane
        self.shape, self.dtype = tuple(plane.shape[1:]), plane.dtype
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = plane.ptr + int(row) * self.nbytes

    def free(self):
        self.ptr = None


class SpectralSynthesizer:
    keep_intensities = False  # (the class's default; __init__ sets the instance's)

    def __init__(self, nus, temperatures, dist, thetas, theta_weights, lines, continuum=None, ctx=None, shard=None,
                 flux_out=None, track_evaluations=True, keep_line=True, keep_total=True, classify_share=None, m_max=None, m_share_out=None,
                 keep_continuum_flux=False, keep_contribution=False, instrument=None, grid_plan=True, keep_response=False, scattering=None,
                 keep_intensities=False):
        """nus: global grid (descending).  lines: dict(line_nus, doppler_widths, gammas, alphas) in the
        reference layout (N_l, N_d), or a stardis_amd.linelist.LineList (per-line scalars; the pre-pass generates the
        three values per (line, depth) itself).  continuum: dict as produced by synth.synth_continuum_state or None.
        shard: (begin, count) of the global frequency index computed here (default: everything).
        flux_out: optional contiguous CUDA tensor (N_d, count) to receive F_nu (e.g. for an RCCL gather).
        classify_share, m_max: the two-collective mode of frequency shards of long lists (include/stardis_hip.h,
        sdx_synthesize_classify_dev) — classify_share = (first line, number of lines) this rank classifies, m_max = a device
        buffer of n_lines doubles (DeviceArray or CUDA tensor) that holds every rank's share once the caller has gathered it.
        m_share_out: optional device buffer that receives the share's values from its index 0 (the send buffer of the all-gather;
        default: they are written in place, m_max[first line ...]).
        A step is then enqueue_classify() [-> the caller's all-gather of m_max] -> enqueue().
        keep_continuum_flux: also trace the continuum flux (N_d, count) in the same formal solution (sdx_synthesis_options.
        F_nu_continuum): F_nu of the same step without lines, bit for bit (F_nu_continuum(), emergent_continuum()).
        keep_contribution: after the synthesis, every step also forms the flux contribution function C (N_d, count) of its own columns
        from the step's total_alphas (sdx_contribution_dev; implies keep_total): what the layer below row k adds to the emergent flux,
        sum_k C[k] = F_nu[-1] up to rounding (`contribution`, `formation_mean(x)`).  Plane-parallel, fp64, at most 64 angles: a context
        with mixed_precision = 1 or more angles are refused here.  Off, the step is unchanged.
        keep_response: after the synthesis (and the contribution function), every step also forms the response functions of its own
        columns from the step's total_alphas (sdx_response_dev; implies keep_total): `response_opacity` (N_d, count), the derivative of
        F_nu[-1] with respect to ln alpha at every depth point, and `response_source`, its derivative with respect to the source
        function there; `flux_derivative(alpha_part)` projects the first on one part of the opacity.  The limits of keep_contribution,
        and a depth whose stashed intensities fit LDS (include/stardis_hip.h).  Off, the step is unchanged.
        instrument: a stardis_amd.instrument.Instrument on this context.  Every step then also forms F_lambda of F_nu[-1]
        (sdx_flux_nu_to_lambda_dev) and passes it through the instrument (sdx_observe_dev: radial velocity, line-spread function,
        pixels) -> `observed` (n_pix,); with keep_continuum_flux also `observed_normalized`, the same with the continuum's F_lambda as
        reference.  Both launches are part of whatever capture() records, and a recorded step follows instrument.set_radial_velocity().
        An instrument with v_rot or v_mac broadens F_lambda (and the continuum's) once per step in front of the pixels — rotation,
        then macroturbulence — and a recorded step follows set_rotation() and set_macroturbulence() too.
        Needs the whole grid (a shard raises ValueError: gather first).  Off, the step is unchanged.
        grid_plan: build an sdx_grid_plan (include/stardis_hip.h) from the uploaded grid, line frequencies and cross-section table
        and pass it with every step: what the pre-pass launch forms from them alone is then formed once, here.  The same bits; dense
        line lists only (a line list of scalars and the two-collective mode step without one).  refresh_grid_plan() after changing the
        uploaded values in place; False: no plan.
        scattering: True, or dict(tol=1e-12, max_iter=2000, acceleration=None); acceleration="ng" or dict(start=4, period=4) solves
        with Ng acceleration (sdx_scatter_source_ng_dev, same buffers, `scattering_accelerations` beside them; the adjoint solve of
        keep_response stays the plain one — it has no accelerated kernel).  After the synthesis every step also solves S = (1 - albedo) B + albedo J[S]
        on its own columns (sdx_scatter_source_dev on the step's total_alphas; implies keep_total) with Thomson scattering — albedo =
        alpha_electron / total_alphas, the per-depth vector of sdx_alpha_electron_dev formed once here: the bits of the electron term in
        the total — and traces that source function (sdx_raytrace_source_dev) into a flux buffer of its own: `scattering_source`,
        `scattering_mean_intensity`, `scattering_flux`, `scattering_iterations`, `scattering_status`.  Needs continuum= (the electron
        densities); plane-parallel, fp64, at most 64 angles.  F_nu, the response functions and everything else stay the LTE ones.  Both
        launches are part of whatever capture() records.  Off, the synthesizer has no such buffer and the step is unchanged.
        With keep_response as well, the step also forms the derivatives of scattering_flux: sdx_response_dev at source = scattering_source
        into buffers of its own, then the adjoint solve (sdx_scatter_response_dev) — `scattering_response_opacity` (for added true
        absorption), `scattering_response_thermal`, `scattering_response_scatter`, `scattering_response_iterations`,
        `scattering_response_status`; flux_derivative(..., scattering=True) and line_sensitivities(..., scattering=True) use the first
        where they otherwise use response_opacity.  Without both options no buffer and no launch is added."""
        self.ctx = ctx or default_context()
        c = self.ctx
        nus = np.ascontiguousarray(nus, dtype=np.float64)
        if np.any(np.diff(nus) >= 0):
            raise ValueError("tracing frequencies must be strictly descending (stardis/base.py:34)")
        self.linelist = None
        self._line_order = None  # the stable sort applied to an unsorted dense list (line_sensitivities answers in the caller's order)
        self._line_tables = None  # (line_nus, doppler_widths, gammas, alphas) in the caller's order, on first use by line_sensitivities
        if isinstance(lines, (LL.LineList, LL.DeviceLineList)):
            (lines.host if isinstance(lines, LL.DeviceLineList) else lines).check_sorted()
            self.linelist = lines if isinstance(lines, LL.DeviceLineList) else lines.upload(c)
        elif np.any(np.asarray(lines["doppler_widths"]) == 0):
            raise ZeroDivisionError("float division by zero")  # voigt.py:148
        self.n_nu = nus.size
        self.begin, self.count = shard if shard is not None else (0, self.n_nu)
        if instrument is not None:  # (before anything is uploaded)
            if self.begin != 0 or self.count != self.n_nu:
                raise ValueError("the instrument needs the whole spectrum: gather the shards first")
            if instrument.ctx is not c:
                raise ValueError("the instrument and the synthesizer must share a context (one stream orders the launches)")
        t = np.ascontiguousarray(temperatures, dtype=np.float64).reshape(-1)
        self.n_depth = t.size
        thetas = np.asarray(thetas, dtype=np.float64)
        self.n_theta = thetas.size
        ray = np.asarray(dist, dtype=np.float64).reshape(-1, 1) / np.cos(thetas)  # radiation_field_solvers/base.py:302-305

        self.nus_host = nus
        self.d_nus = c.upload(nus)
        self.d_t = c.upload(t)
        self.d_ray = c.upload(ray)
        self.d_w = c.upload(np.asarray(theta_weights, dtype=np.float64))
        if self.linelist is not None:
            if self.linelist.n_depth != self.n_depth:
                raise ValueError("line list and model disagree on the number of depth points")
            self.n_lines, self.gamma_cols = self.linelist.n_lines, self.linelist.gamma_cols
        else:
            ln = np.ascontiguousarray(lines["line_nus"], dtype=np.float64)
            self.n_lines = ln.size
            g = np.ascontiguousarray(lines["gammas"], dtype=np.float64)
            g = g.reshape(self.n_lines, -1) if self.n_lines else np.zeros((0, 1))
            dw = np.ascontiguousarray(lines["doppler_widths"], dtype=np.float64)
            al = np.ascontiguousarray(lines["alphas"], dtype=np.float64)
            if ln.size > 1 and np.any(ln[1:] < ln[:-1]):
                # the kernels take the list in ascending frequency (what calc_alpha_line_at_nu passes, base.py:392-397); the
                # reference's calc_alan_entries accepts any order, so an unsorted list is sorted (stably) here, not refused
                order = np.argsort(ln, kind="stable")
                ln, g, dw, al = (np.ascontiguousarray(a[order]) for a in (ln, g, dw, al))
                self._line_order = order
            self.gamma_cols = g.shape[1]
            self.d_ln = c.upload(ln)
            self.d_dw = c.upload(dw)
            self.d_g = c.upload(g)
            self.d_a = c.upload(al)

        self._keep = []
        self.cont = self._build_continuum(continuum, nus, t)
        self._has_continuum = continuum is not None
        self._ew = None  # equivalent_widths: (abscissa, continuum plane) on the device, allocated at its first call

        # optional output planes: allocated only when asked for (0.5 GB each at 1.2e6 frequencies)
        self.keep_contribution = bool(keep_contribution)
        if self.keep_contribution:
            # the library's own refusals (mixed precision, angles, depth), asked with an empty grid: nothing is enqueued
            c.call("sdx_contribution_dev", self.n_depth, 0, self.n_theta, None, None, None, None, None, 0, None, 0, None, 0)
            keep_total = True
        self.keep_intensities = bool(keep_intensities)
        if self.keep_intensities:
            c.call("sdx_emergent_intensity_dev", self.n_depth, 0, self.n_theta, None, None, None, None, 0, None, 0, 0, None, 0)
            keep_total = True
        self.keep_response = bool(keep_response)
        if self.keep_response:
            c.call("sdx_response_dev", self.n_depth, 0, self.n_theta, None, None, None, None, None, 0, None, 0, None, 0, None, 0)
            keep_total = True
        self.scattering = self._scattering_options(scattering, continuum)
        if self.scattering is not None:
            ng = self.scattering.get("acceleration")
            c.call("sdx_scatter_source_dev" if ng is None else "sdx_scatter_source_ng_dev", self.n_depth, 0, self.n_theta, None, None, None, None, None, 0,
                   None, 0, None, 0, self.scattering["tol"], self.scattering["max_iter"], None, 0, None, 0, None, None, None,
                   *(() if ng is None else (ng["start"], ng["period"], None)))
            keep_total = True
        self._scattering_response = self.scattering is not None and self.keep_response
        if self._scattering_response:
            c.call("sdx_scatter_response_dev", self.n_depth, 0, self.n_theta, None, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0,
                   self.scattering["tol"], self.scattering["max_iter"], None, 0, None, 0, None, 0, None, 0, None, None, None)
        self.d_line = c.empty((self.n_depth, self.count)) if keep_line else None
        self.d_total = c.empty((self.n_depth, self.count)) if keep_total else None
        self._flux_tensor = flux_out
        self.d_F = None if flux_out is not None else c.empty((self.n_depth, self.count))
        self.d_evals = c.zeros((1,), np.int64) if track_evaluations else None
        self.keep_continuum_flux = bool(keep_continuum_flux)
        self.d_Fc = c.empty((self.n_depth, self.count)) if self.keep_continuum_flux else None
        self.d_C = c.empty((self.n_depth, self.count)) if self.keep_contribution else None
        self.d_I = c.empty((self.n_theta, self.count)) if self.keep_intensities else None
        self.ring_scale = np.sin(thetas).reshape(-1)  # the projected radius of each angle's ring on the disk
        self._disk = None  # disk_integrated's buffers, made at its first call
        self.d_Ra = c.empty((self.n_depth, self.count)) if self.keep_response else None
        self.d_Rs = c.empty((self.n_depth, self.count)) if self.keep_response else None
        if self.scattering is not None:
            from . import ops

            plane = (self.n_depth, self.count)
            self.d_mean_w = c.upload(ops.mean_weights(thetas, theta_weights))
            self.d_thomson = c.empty((self.n_depth,))  # one value per depth point: sdx_alpha_electron_dev at a single frequency
            c.call("sdx_alpha_electron_dev", self.n_depth, 1, self.cont.electron_density, self.d_thomson.ptr, 1)
            self.d_Ssc, self.d_Jsc, self.d_Fsc = c.empty(plane), c.empty(plane), c.empty(plane)
            self.d_sc_iterations, self.d_sc_status = c.empty((self.count,), np.int32), c.empty((self.count,), np.int32)
            self.d_sc_change = c.empty((self.count,))
            if self.scattering.get("acceleration") is not None:
                self.d_sc_accelerations = c.empty((self.count,), np.int32)
            if self._scattering_response:
                # the flux's direct part and cotangent at source = S, then the three response planes of the adjoint solve
                self.d_sc_direct, self.d_sc_cotangent = c.empty(plane), c.empty(plane)
                self.d_sc_Ra, self.d_sc_Rt, self.d_sc_Rs = c.empty(plane), c.empty(plane), c.empty(plane)
                self.d_scr_iterations, self.d_scr_status = c.empty((self.count,), np.int32), c.empty((self.count,), np.int32)
        self.instrument = instrument
        if instrument is not None:
            self.lambdas = K.nu_to_angstrom(nus)
            self.d_lambdas = c.upload(self.lambdas)
            instrument.reserve(self.n_nu)  # (a broadening instrument's scratch: a capture of the step allocates nothing)
            self.d_Flam = c.empty((self.n_nu,))
            self.d_observed = c.empty((instrument.n_pix,))
            if self.keep_continuum_flux:
                self.d_Fclam = c.empty((self.n_nu,))
                self.d_observed_normalized = c.empty((instrument.n_pix,))
        self._keep_line = keep_line  # also write the summed line opacity plane (alpha_line())
        self._keep_total = keep_total  # also write total_alphas (the reference keeps it on Opacities; the flux does not need it in HBM)
        self.count_evaluations = track_evaluations  # sum(hi - lo) per step costs a memset + copy: switch off when timing
        self.graph = None
        self.graph_classify = None
        self.graph_batch, self.batch = None, 1
        self.classify_share, self.m_max, self.m_share_out = classify_share, m_max, m_share_out
        if (classify_share is None) != (m_max is None):
            raise ValueError("classify_share and m_max go together")
        if m_max is not None and (self.linelist is not None or track_evaluations):
            raise ValueError("the two-collective mode takes dense line lists and no evaluation count")
        if m_max is not None:
            # the library writes m_max[first line ...] (or m_share_out[0 ...]) and reads all of m_max: check the buffers here, an
            # undersized one would be an out-of-bounds device access
            b, n = (int(v) for v in classify_share)
            if b < 0 or n < 0 or b + n > self.n_lines:
                raise ValueError("classify_share lies outside the line list")
            _require_f64_buffer("m_max", m_max, self.n_lines)
            if m_share_out is not None:
                _require_f64_buffer("m_share_out", m_share_out, n)
        c.call("sdx_reserve_line_workspace", self.n_depth, self.n_lines)
        self.plan = None
        if grid_plan and self.linelist is None and self.m_max is None and self.n_lines > 0:
            plan = C.c_void_p()
            c.call("sdx_grid_plan_create", self.n_nu, self.d_nus.ptr, self.n_lines, self.d_ln.ptr, C.byref(self.cont), C.byref(plan))
            self.plan = plan

    scattering = None  # (the class's default: a synthesizer without the option carries no attribute of it)

    @staticmethod
    def _scattering_options(scattering, continuum):
        """None (off), or dict(tol, max_iter, acceleration) checked on the host; acceleration: None or dict(start, period)"""
        if scattering is None or scattering is False:
            return None
        opts = dict(tol=1e-12, max_iter=2000, acceleration=None)
        if scattering is not True:
            unknown = set(scattering) - set(opts)
            if unknown:
                raise ValueError(f"scattering: unknown option(s) {sorted(unknown)} (tol, max_iter, acceleration)")
            opts.update(scattering)
        from . import ops

        ng = ops.acceleration_options("scattering", opts["acceleration"])
        opts = dict(tol=float(opts["tol"]), max_iter=int(opts["max_iter"]))
        if ng is not None:
            opts["acceleration"] = ng  # (without the key the options are what they were: dict(tol, max_iter))
        if not opts["tol"] >= 0.0 or opts["max_iter"] < 1:
            raise ValueError("scattering: need tol >= 0 and max_iter >= 1")
        if continuum is None:
            raise ValueError("scattering needs continuum=: the Thomson opacity comes from its electron densities")
        return opts

    def refresh_grid_plan(self):
        """Rebuild the plan's arrays (one launch on the context's stream) after the uploaded frequency grid, line frequencies or
        cross-section table were overwritten in place."""
        if self.plan is not None:
            _lib.check(self.ctx.lib.sdx_grid_plan_refresh(self.plan))

    # -- set-up ---------------------------------------------------------------------------------
    def _build_continuum(self, cont, nus, t):
        c = self.ctx
        s = Continuum()
        up = lambda a, dt=np.float64: self._hold(c.upload(np.ascontiguousarray(a, dtype=dt), dt))  # noqa: E731
        s.temperature = self.d_t.ptr
        if cont is None:
            return s
        lam = K.nu_to_angstrom(nus)  # tracing_nus.to(u.AA, u.spectral()) (opacities_solvers/base.py:62)
        s.lambdas = up(lam)
        s.n_table = len(cont["hminus_bf_wavelength"])
        s.table_wavelength = up(cont["hminus_bf_wavelength"])
        s.table_sigma = up(cont["hminus_bf_cross_section"])
        s.table_density = up(cont["n_hminus"])
        cutoff = (cont["ionization_energy"] - np.asarray(cont["level_excitation"])) / K.H_CGS
        s.bf_n_species = 1
        s.bf_n_levels = len(cutoff)
        s.bf_species_offsets = up([0, len(cutoff)], np.int32)
        s.bf_species_ion_number = up([0], np.int32)
        s.bf_cutoff = up(cutoff)
        s.bf_level_density = up(cont["level_density"])
        s.ff_n_species = 1
        s.ff_species_ion_number = up([1], np.int32)  # get_number_density("H_I_ff") returns ion_number + 1
        s.ff_number_density = up(np.asarray(cont["n_e"]) * np.asarray(cont["n_h2"]))  # util.py:160-164
        s.rayleigh_enabled = 0
        s.electron_density = up(cont["n_e"])
        return s

    @property
    def keep_line(self):
        return self._keep_line

    @keep_line.setter
    def keep_line(self, on):
        if on and self.d_line is None:
            self.d_line = self.ctx.empty((self.n_depth, self.count))
        self._keep_line = bool(on)

    @property
    def keep_total(self):
        return self._keep_total

    @keep_total.setter
    def keep_total(self, on):
        if not on and self.keep_contribution:
            raise ValueError("keep_contribution reads the step's total_alphas: keep_total stays on")
        if not on and self.keep_response:
            raise ValueError("keep_response reads the step's total_alphas: keep_total stays on")
        if not on and self.keep_intensities:
            raise ValueError("keep_intensities reads the step's total_alphas: keep_total stays on")
        if not on and self.scattering is not None:
            raise ValueError("scattering reads the step's total_alphas: keep_total stays on")
        if on and self.d_total is None:
            self.d_total = self.ctx.empty((self.n_depth, self.count))
        self._keep_total = bool(on)

    def _hold(self, dev):
        self._keep.append(dev)
        return dev.ptr

    @property
    def flux_ptr(self):
        return ptr_of(self._flux_tensor) if self._flux_tensor is not None else self.d_F.ptr

    def _device_vector(self, name, value, want, noun=None, at_least=False):
        """A caller's vector (host array, DeviceArray or CUDA tensor) -> a device buffer of float64 values, checked on the host before
        anything is uploaded; ValueError naming it.  want: a number — the values are flattened and there is one per `noun` — or a
        shape, which the value has as it stands.  at_least: a device buffer may hold more values than want."""
        shaped = isinstance(want, tuple)
        n = int(np.prod(want, dtype=np.int64)) if shaped else int(want)
        on_device = isinstance(value, _lib.DeviceArray) or hasattr(value, "data_ptr")
        if on_device:
            _require_f64_buffer(name, value, n if shaped or at_least else 0)
            got = tuple(int(v) for v in value.shape)
        else:
            value = np.ascontiguousarray(value, dtype=np.float64)
            got = value.shape if shaped else (value.size,)
        if shaped:
            if got != want:
                raise ValueError(f"{name} must have shape {want}, got {got}")
        elif not (on_device and at_least):
            size = int(np.prod(got, dtype=np.int64))
            if size != n:
                raise ValueError(f"{name} must hold one value per {noun} ({n}), got {size}")
        return value if on_device else self.ctx.upload(value if shaped else value.reshape(-1))

    # -- one step: everything from resident inputs to F_nu -----------------------------------------
    def enqueue_classify(self):
        """Two-collective mode, phase 1: this rank's share of the classification stream (+ grid spacing, line ranges and continuum
        plane of the step) -> m_max[share]; the caller gathers m_max before enqueue()."""
        c = self.ctx
        b, n = self.classify_share
        # (the library writes m_max[l] for the lines l of the share: with a send buffer, entry l lands at index l - b of it)
        base = ptr_of(self.m_max) if self.m_share_out is None else ptr_of(self.m_share_out) - 8 * int(b)
        c.call("sdx_synthesize_classify_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, self.count, self.n_lines, self.d_ln.ptr,
               self.d_dw.ptr, self.d_g.ptr, self.gamma_cols, self.d_a.ptr, C.byref(self.cont), int(b), int(n), base)

    def enqueue(self):
        """One fused step on the context's stream: sdx_synthesize_opt_dev (pre-pass, line gather, total, raytrace); with
        keep_contribution, sdx_contribution_dev on the step's total_alphas behind it; with keep_response, sdx_response_dev behind that;
        with scattering, sdx_scatter_source_dev and the flux of its source function; with an instrument, F_lambda and sdx_observe_dev last."""
        self._enqueue_synthesis()
        self._enqueue_tail()

    def _enqueue_tail(self):
        """what follows the synthesis of a step, fused or not: contribution, emergent intensities, response, scattering, the instrument"""
        if self.keep_contribution:
            self._enqueue_contribution()
        if self.keep_intensities:
            self._enqueue_intensities()
        if self.keep_response:
            self._enqueue_response()
        if self.scattering is not None:
            self._enqueue_scattering()
        if self.instrument is not None:
            self._enqueue_observe()

    def _enqueue_observe(self):
        c, n, inst = self.ctx, self.n_nu, self.instrument
        last = 8 * (self.n_depth - 1) * self.count  # row N_d - 1
        c.call("sdx_flux_nu_to_lambda_dev", n, self.flux_ptr + last, self.d_nus.ptr, self.d_lambdas.ptr, self.d_Flam.ptr)
        if self.keep_continuum_flux:
            c.call("sdx_flux_nu_to_lambda_dev", n, self.d_Fc.ptr + last, self.d_nus.ptr, self.d_lambdas.ptr, self.d_Fclam.ptr)
        if not inst.broadens:
            inst.observe(self.d_lambdas, self.d_Flam, n, out=self.d_observed)
            if self.keep_continuum_flux:
                inst.observe(self.d_lambdas, self.d_Flam, n, reference=self.d_Fclam, out=self.d_observed_normalized)
            return
        # rotation, macroturbulence: F_lambda (and the continuum's) broadened ONCE per step, whatever is observed of them
        if not self.keep_continuum_flux:
            inst.observe(self.d_lambdas, inst.broaden(self.d_lambdas, self.d_Flam, n), n, out=self.d_observed, broadened=True)
            return
        flux, cont = inst.broaden(self.d_lambdas, self.d_Flam, n, reference=self.d_Fclam)
        inst.observe(self.d_lambdas, flux, n, out=self.d_observed, broadened=True)
        inst.observe(self.d_lambdas, flux, n, reference=cont, out=self.d_observed_normalized, broadened=True)

    def _columns(self, weights=None):
        """what every formal solution of the step's columns is called with first: the shape, the shard's frequencies, the temperatures, the
        ray table, the angle weights (the intensities take none) and the step's total_alphas"""
        w = () if weights is None else (weights.ptr,)
        return (self.n_depth, self.count, self.n_theta, self.d_nus.ptr + 8 * self.begin, self.d_t.ptr, self.d_ray.ptr, *w, self.d_total.ptr, self.count)

    def _enqueue_contribution(self):
        self.ctx.call("sdx_contribution_dev", *self._columns(self.d_w), None, 0, self.d_C.ptr, self.count)

    def _enqueue_intensities(self):
        self.ctx.call("sdx_emergent_intensity_dev", *self._columns(), None, 0, 0, self.d_I.ptr, self.count)

    def _enqueue_response(self):
        self.ctx.call("sdx_response_dev", *self._columns(self.d_w), None, 0, self.d_Ra.ptr, self.count, self.d_Rs.ptr, self.count)

    def _enqueue_scattering(self):
        """the scattering source function of the step's columns from its total_alphas, then the flux of that source function"""
        c, cnt, flux, mean = self.ctx, self.count, self._columns(self.d_w), self._columns(self.d_mean_w)
        ng = self.scattering.get("acceleration")
        solve = (*mean, self.d_thomson.ptr, 0, None, 0, self.scattering["tol"], self.scattering["max_iter"], self.d_Ssc.ptr, cnt,
                 self.d_Jsc.ptr, cnt, self.d_sc_iterations.ptr, self.d_sc_status.ptr, self.d_sc_change.ptr)
        if ng is None:
            c.call("sdx_scatter_source_dev", *solve)
        else:
            c.call("sdx_scatter_source_ng_dev", *solve, ng["start"], ng["period"], self.d_sc_accelerations.ptr)
        c.call("sdx_raytrace_source_dev", *flux, self.d_Ssc.ptr, cnt, self.d_Fsc.ptr, cnt, None, 0, 0, 1.0)
        if self._scattering_response:
            # the derivative of that flux: the response functions at source = S are its direct part and cotangent, the adjoint solve the rest
            c.call("sdx_response_dev", *flux, self.d_Ssc.ptr, cnt, self.d_sc_direct.ptr, cnt, self.d_sc_cotangent.ptr, cnt)
            c.call("sdx_scatter_response_dev", *mean, self.d_thomson.ptr, 0, None, 0, self.d_Ssc.ptr, cnt, self.d_sc_cotangent.ptr, cnt,
                   self.d_sc_direct.ptr, cnt, self.scattering["tol"], self.scattering["max_iter"], None, 0, self.d_sc_Rt.ptr, cnt, self.d_sc_Ra.ptr, cnt,
                   self.d_sc_Rs.ptr, cnt, self.d_scr_iterations.ptr, self.d_scr_status.ptr, None)

    def _enqueue_synthesis(self):
        """The step, whatever its configuration: one sdx_synthesis_options, one sdx_synthesize_opt_dev call.  A line list of scalars
        goes in the options (the dense pointers are not read); the plan only with a dense list outside the two-collective mode, where
        the library would ignore it; phase 2 of the two-collective mode counts no evaluations."""
        opt = _lib.SynthesisOptions()
        m_max = self.m_max
        if self.keep_continuum_flux:
            opt.F_nu_continuum, opt.continuum_ld = self.d_Fc.ptr, self.count
        if m_max is not None:  # phase 2 of the two-collective mode: everything behind the classification launch
            opt.line_m_max = ptr_of(m_max)
        if self.linelist is not None:
            opt.linelist = C.cast(self.linelist.byref(), C.POINTER(_lib.LineListStruct))
            ln = dw = g = al = None
        else:
            ln, dw, g, al = self.d_ln.ptr, self.d_dw.ptr, self.d_g.ptr, self.d_a.ptr
            if self.plan is not None and m_max is None:
                opt.grid_plan = self.plan
        evals = ptr_of(self.d_evals) if self.count_evaluations and m_max is None else None
        self.ctx.call("sdx_synthesize_opt_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, self.count, self.n_lines, ln, dw, g,
                      self.gamma_cols, al, C.byref(self.cont), self.n_theta, self.d_t.ptr, self.d_ray.ptr, self.d_w.ptr,
                      self.d_line.ptr if self.keep_line else None, self.d_total.ptr if self.keep_total else None, self.flux_ptr, self.count,
                      C.byref(opt), evals)

    def enqueue_unfused(self):
        """The same step through the individual entry points (what calc_alphas + raytrace issue)."""
        c = self.ctx
        nd, cnt = self.n_depth, self.count
        self.keep_line = self.keep_total = True  # this path materialises both planes
        if self.linelist is not None:
            c.call("sdx_line_opacity_linelist_dev", nd, self.n_nu, self.d_nus.ptr, self.begin, cnt, self.linelist.byref(),
                   self.d_line.ptr, cnt, 0, ptr_of(self.d_evals))
        else:
            c.call("sdx_line_opacity_dev", nd, self.n_nu, self.d_nus.ptr, self.begin, cnt, self.n_lines, self.d_ln.ptr,
                   self.d_dw.ptr, self.d_g.ptr, self.gamma_cols, self.d_a.ptr, self.d_line.ptr, cnt, 0, ptr_of(self.d_evals))
        c.call("sdx_total_alphas_dev", nd, self.n_nu, self.d_nus.ptr, self.begin, cnt, C.byref(self.cont), self.d_line.ptr, cnt,
               self.d_total.ptr, cnt)
        nus_shard = self.d_nus.ptr + 8 * self.begin
        c.call("sdx_raytrace_dev", nd, cnt, self.n_theta, nus_shard, self.d_t.ptr, self.d_ray.ptr, self.d_w.ptr,
               self.d_total.ptr, cnt, self.flux_ptr, cnt, None, 0)
        self._enqueue_tail()

    def capture(self, eager_phase2=True, batch=1):
        """Record one step into a hipGraph (after one eager step has sized the scratch).  batch > 1: ALSO a graph of `batch` consecutive
        steps (step_batch()): successive graph launches are ~8.5 us apart on this runtime whatever they hold — a tenth of a 92 us step —
        so a caller with a queue of syntheses replays several steps per launch.  Two-collective mode: two graphs, the
        classification launch and the rest — the caller's all-gather of m_max goes between step_classify() and step(); m_max must
        hold every rank's share when capture() is called (the eager pass reads it) unless eager_phase2 is False (a re-capture
        after the scratch has moved: it is large enough already, and m_max may not have been gathered yet)."""
        c = self.ctx

        def record(enqueue):
            c.call("sdx_graph_begin")
            try:
                enqueue()
            finally:
                handle = C.c_void_p()
                _lib.check(c.lib.sdx_graph_end(c.handle, C.byref(handle)))
            return handle

        if self.m_max is not None:
            self.enqueue_classify()
            if eager_phase2:
                self.enqueue()
            c.synchronize()
            self.graph_classify = record(self.enqueue_classify)
            self.graph = record(self.enqueue)
            return self
        self.enqueue()
        c.synchronize()
        self.graph = record(self.enqueue)
        if batch > 1:
            def many():
                for _ in range(batch):
                    self.enqueue()
            self.graph_batch, self.batch = record(many), int(batch)
        return self

    def _replay(self, which, **capture_args):
        """Launch the recorded graph `which`.  Another, larger synthesis on this context may have made the library reallocate its
        scratch: the captured pointers are dead then.  Capture again with this graph's own arguments (the scratch is large enough
        for both now) and replay."""
        try:
            self.ctx.call("sdx_graph_launch", getattr(self, which))
        except _lib.StaleGraphError:
            self._destroy_graphs()
            self.capture(**capture_args)
            self.ctx.call("sdx_graph_launch", getattr(self, which))

    def step_classify(self):
        if self.graph_classify is not None:
            # (m_max holds the previous step's values or nothing yet: no eager phase 2 on it)
            self._replay("graph_classify", eager_phase2=False)
        else:
            self.enqueue_classify()

    def step(self):
        if self.graph is not None:
            self._replay("graph")
        else:
            self.enqueue()

    def step_batch(self):
        """`self.batch` consecutive steps as ONE graph launch (capture(batch=n)); -> the number of steps enqueued."""
        if self.graph_batch is None:
            self.step()
            return 1
        n = self.batch  # (read here: destroying a stale graph resets it)
        self._replay("graph_batch", batch=n)
        return n

    def synchronize(self):
        self.ctx.synchronize()

    # -- results ----------------------------------------------------------------------------------
    def F_nu(self):
        if self._flux_tensor is not None:
            self.ctx.synchronize()
            return self._flux_tensor.cpu().numpy()
        return self.d_F.numpy()

    def _require_continuum(self):
        if not self.keep_continuum_flux:
            raise RuntimeError("the continuum flux was not kept: construct the synthesizer with keep_continuum_flux=True")

    @property
    def F_nu_continuum(self):
        """-> (N_d, count) numpy array: the continuum flux of the last step."""
        self._require_continuum()
        return self.d_Fc.numpy()

    @property
    def emergent_continuum(self):
        """-> (count,) numpy array: the continuum flux of the outermost depth point, F_nu_continuum[-1]."""
        return self.F_nu_continuum[-1]

    @property
    def contribution(self):
        """-> DeviceArray (N_d, count): the flux contribution function of the last step (`.numpy()` for a host array)."""
        if not self.keep_contribution:
            raise RuntimeError("the contribution function was not kept: construct the synthesizer with keep_contribution=True")
        return self.d_C

    @property
    def emergent_intensities(self):
        """-> DeviceArray (N_theta, count): the emergent intensity of every ray of the last step, angle by angle (`.numpy()` for a host
        array): no theta weights applied."""
        if not self.keep_intensities:
            raise RuntimeError("the emergent intensities were not kept: construct the synthesizer with keep_intensities=True")
        return self.d_I

    def disk_integrated(self, v_rot):
        """-> DeviceArray (n_nu,): F_lambda of the last step integrated over the disk of a rigid rotator with v sin i = v_rot (km/s):
        every angle's emergent intensity converted to per Angstrom (sdx_flux_nu_to_lambda_dev's operation, ring by ring), the ring at
        the projected radius sin(theta) convolved with its own arcsine density and the rings summed with the flux weights in the flux's
        order (sdx_disk_integrate_dev) — the model's own centre-to-limb variation, line by line, in place of a limb-darkening
        coefficient.  v_rot = 0 is F_lambda itself.  Needs the whole spectrum (a shard raises ValueError: gather first).  The buffers
        are made at the first call and reused: the result is overwritten by the next call."""
        d = self._disk_rings(v_rot)  # (raises before anything else is looked at)
        c, n = self.ctx, self.n_nu
        c.call("sdx_disk_integrate_dev", n, d["lambdas"].ptr, self.n_theta, d["scale"].ptr, self.d_w.ptr, d["I_lambda"].ptr, n, None, d["rot"].ptr,
               d["out"].ptr, None)
        return d["out"]

    def _disk_buffers(self, v_rot):
        """the disk's buffers (made at the first call) with {V, 0} written into the device pair -> (dict, V); raises without
        keep_intensities or on a shard"""
        from .instrument import rotation_pair

        self.emergent_intensities
        if self.begin != 0 or self.count != self.n_nu:
            raise ValueError("the disk integration needs the whole spectrum: gather the shards first")
        V, _ = rotation_pair(v_rot)
        c, n = self.ctx, self.n_nu
        if self._disk is None:
            d_lam = self.d_lambdas if self.instrument is not None else c.upload(K.nu_to_angstrom(self.nus_host))
            self._disk = dict(lambdas=d_lam, scale=c.upload(self.ring_scale), I_lambda=c.empty((self.n_theta, n)), rot=c.empty((2,)), out=c.empty((n,)))
        self._disk["rot"].set(np.array([V, 0.0]))
        return self._disk, V

    def _disk_rings(self, v_rot):
        """_disk_buffers, and the last step's emergent intensities converted to per Angstrom ring by ring into I_lambda -> dict"""
        d, _ = self._disk_buffers(v_rot)
        c, n, d_I = self.ctx, self.n_nu, self.d_I
        for r in range(self.n_theta):
            c.call("sdx_flux_nu_to_lambda_dev", n, d_I.ptr + 8 * r * n, self.d_nus.ptr, d["lambdas"].ptr, d["I_lambda"].ptr + 8 * r * n)
        return d

    @staticmethod
    def _positive_rotation(v_rot):
        from .instrument import rotation_pair

        V, _ = rotation_pair(v_rot)
        if not V > 0.0:
            raise ValueError("the derivative to v sin i needs v_rot > 0 (at v_rot = 0 the disk integration is the flux sum)")
        return V

    def _disk_dlnv(self, V, out):
        """disk_integrated(V) into the disk's `out` (the same bits) and its derivative to ln V into `out` given, one launch
        (sdx_disk_integrate_deriv_dev)"""
        d = self._disk_rings(V)
        c, n = self.ctx, self.n_nu
        c.call("sdx_disk_integrate_deriv_dev", n, d["lambdas"].ptr, self.n_theta, d["scale"].ptr, self.d_w.ptr, d["I_lambda"].ptr, n, None,
               d["rot"].ptr, d["out"].ptr, None, out.ptr, None)
        return out

    def disk_integrated_derivative(self, v_rot):
        """-> (F_lambda, dF_lambda / dV), DeviceArrays (n_nu,): disk_integrated(v_rot) — the same bits — and its derivative to v sin i
        per km/s from the same launch (sdx_disk_integrate_deriv_dev: exact for the discrete operator; d / d ln V divided by V on the
        host: a diagnostic call, it waits for the stream).  v_rot > 0 is required (ValueError at 0, where the operator is a copy).
        Not meant where an end of the grid lies within 1e-5 of a ring's edge (include/stardis_hip.h).  The buffers are
        disk_integrated's and one more, reused: overwritten by the next call."""
        self.emergent_intensities
        V = self._positive_rotation(v_rot)
        d, _ = self._disk_buffers(V)
        if "dout" not in d:
            d["dout"] = self.ctx.empty((self.n_nu,))
        self._disk_dlnv(V, d["dout"])
        d["dout"].set(d["dout"].numpy() / V)
        return d["out"], d["dout"]

    def disk_weights_to_rays(self, u, v_rot):
        """-> DeviceArray (N_theta, n_nu): the cotangent on emergent_intensities of weights u (n_nu; host array, DeviceArray or CUDA
        tensor) over disk_integrated(v_rot) — sum_i u_i disk_integrated(v_rot)_i = sum_theta sum_j W[theta, j] emergent_intensities[theta,
        j] — the transpose of the disk integration ring by ring with the factor nu / lambda of F_lambda applied
        (sdx_disk_integrate_adjoint_dev with nus).  v_rot = 0: W[theta, j] = w_theta u_j nu_j / lambda_j.  Needs keep_intensities=True
        and the whole spectrum.  On demand: a synthesizer that never asks allocates and launches nothing new."""
        d, _ = self._disk_buffers(v_rot)
        c, n = self.ctx, self.n_nu
        d_u = self._device_vector("u", u, n, "column of the spectrum")
        W = c.empty((self.n_theta, n))
        c.call("sdx_disk_integrate_adjoint_dev", n, d["lambdas"].ptr, self.n_theta, d["scale"].ptr, self.d_w.ptr, d["rot"].ptr, ptr_of(d_u), None,
               self.d_nus.ptr, W.ptr, n, None)
        return W

    def ray_response(self, cotangent, want_opacity=True, want_source=True):
        """-> (R_alpha, R_source), DeviceArrays (N_d, count) (None for one not wanted): the derivatives of sum_theta cotangent[theta, i]
        emergent_intensities[theta, i] with respect to ln alpha[k, i] and to the source function S[k, i], from the last step's
        total_alphas and its source (the Planck function) — sdx_response_angles_dev: one launch that costs what the step's own
        k_response costs, in place of N_theta launches with one-hot weights.  cotangent (N_theta, count): host array, DeviceArray or
        CUDA tensor — disk_weights_to_rays(u, v_rot), say.  The step's total_alphas are kept with keep_intensities=True."""
        self.emergent_intensities
        if not (want_opacity or want_source):
            raise ValueError("ray_response: no output requested")
        c, cnt = self.ctx, self.count
        d_cot = self._device_vector("cotangent", cotangent, (self.n_theta, cnt))
        d_Ra = c.empty((self.n_depth, cnt)) if want_opacity else None
        d_Rs = c.empty((self.n_depth, cnt)) if want_source else None
        c.call("sdx_response_angles_dev", self.n_depth, cnt, self.n_theta, self.d_nus.ptr + 8 * self.begin, self.d_t.ptr, self.d_ray.ptr,
               ptr_of(d_cot), cnt, self.d_total.ptr, cnt, None, 0, ptr_of(d_Ra), cnt, ptr_of(d_Rs), cnt)
        return d_Ra, d_Rs

    def disk_line_sensitivities(self, u, v_rot, per_depth=False, wrt="strength"):
        """-> DeviceArray (n_lines,), or (n_lines, N_d) with per_depth=True: d(sum_i u_i disk_integrated(v_rot)_i) / d ln gf_l for every
        line of the list, at fixed windows, from the last step: disk_weights_to_rays(u, v_rot) -> ray_response -> the weight plane and
        the line adjoints of line_sensitivities, which this is with the disk integration in the flux sum's place (v_rot = 0:
        line_sensitivities(weights=u nu / lambda) up to the rounding of the theta sum).  wrt: as for line_sensitivities.  Needs
        keep_intensities=True and keep_response=True; plane-parallel, no scattering, the whole spectrum."""
        names, single = self._wrt_names(wrt)
        self._require_response()
        d_R, _ = self.ray_response(self.disk_weights_to_rays(u, v_rot), want_source=False)
        return self._sensitivities_of_response(d_R, None, names, single, per_depth)

    def _require_disk_instrument(self):
        self._require_instrument()
        if self.instrument.rotates:
            raise ValueError("the instrument already carries a v_rot: the disk integration is the rotation (rotation twice)")

    def observed_disk_line_sensitivities(self, c, v_rot, per_depth=False, wrt="strength"):
        """-> as disk_line_sensitivities: d(sum_j c_j observed_disk_integrated(v_rot)_j) / d ln gf_l — the pixel weights c taken back
        through the instrument's pixel and macroturbulence stages (Instrument.adjoint without nus: weights over the disk-integrated
        F_lambda), then disk_line_sensitivities.  An instrument with a v_rot of its own raises, as observed_disk_integrated does."""
        self._wrt_names(wrt)
        self._require_disk_instrument()
        self._require_response()
        self.emergent_intensities
        u = self.instrument.adjoint(self.d_lambdas, self.n_nu, self._pixel_vector("c", c))
        return self.disk_line_sensitivities(u, v_rot, per_depth, wrt)

    def chi2_disk_gradient(self, data, inverse_variance, v_rot, wrt="strength", per_depth=False):
        """-> (chi2, d chi2 / dV, line gradient): chi2 = sum_j ivar_j (data_j - observed_disk_integrated(v_rot)_j)^2 of the last step,
        its derivative to v sin i per km/s, and its gradient to ln gf of every line ((n_lines,), or (n_lines, N_d); wrt as for
        line_sensitivities) — one fit step of the rotation and the line list together with the model's own centre-to-limb variation.
        d chi2 / dV = sum_j c_j t_j, c_j = -2 ivar_j (data_j - observed_j), t = Instrument.tangent of d disk_integrated / dV (the sum on
        the host, math.fsum); the line gradient is observed_disk_line_sensitivities(c, v_rot).  Left out of all three: NaN pixels,
        pixels with inverse_variance 0 and the pixels edge-affected at the reach (v_rot + 6 v_mac) / c (Instrument.edge_affected(...,
        v_rot=v_rot)), as chi2_line_gradient leaves them out.  v_rot > 0; an instrument with a v_rot of its own raises.  A diagnostic
        call: it waits for the stream."""
        self._wrt_names(wrt)
        self._require_disk_instrument()
        self._require_response()
        self.emergent_intensities
        V = self._positive_rotation(v_rot)
        inst, n = self.instrument, self.n_nu
        # one launch gives disk_integrated(V), bit for bit, and its derivative; then the instrument as observed_disk_integrated applies it
        d_dlnv = self._disk_dlnv(V, self.ctx.empty((n,)))
        flux = self._disk["out"]
        broadened = inst.macroturbulence(self.d_lambdas, flux, n) if inst.macroturbulent else flux
        observed = inst.observe(self.d_lambdas, broadened, n, out=self.ctx.empty((inst.n_pix,)), broadened=True).numpy()
        chi2, c, use, _ = self._chi2_pixel_weights(data, inverse_variance, False, observed=observed, v_rot=V)
        t = inst.tangent(self.d_lambdas, n, flux, d_dlnv).numpy()
        dchi2_dv = math.fsum(c * np.where(use, t, 0.0)) / V
        return chi2, dchi2_dv, self.observed_disk_line_sensitivities(c, V, per_depth, wrt)

    def observed_disk_integrated(self, v_rot):
        """-> DeviceArray (n_pix,): disk_integrated(v_rot) through the instrument — its macroturbulence (if any), then the radial
        velocity, line-spread function and pixels (observe(..., broadened=True)).  An instrument that carries a v_rot of its own
        raises ValueError: the star would be rotated twice."""
        inst = self.instrument
        if inst is None:
            raise RuntimeError("no instrument: construct the synthesizer with instrument=")
        if inst.rotates:
            raise ValueError("the instrument already carries a v_rot: the disk integration is the rotation (rotation twice)")
        flux = self.disk_integrated(v_rot)
        if inst.macroturbulent:
            flux = inst.macroturbulence(self.d_lambdas, flux, self.n_nu)
        return inst.observe(self.d_lambdas, flux, self.n_nu, out=self.ctx.empty((inst.n_pix,)), broadened=True)

    def _require_response(self):
        if not self.keep_response:
            raise RuntimeError("the response functions were not kept: construct the synthesizer with keep_response=True")

    @property
    def response_opacity(self):
        """-> DeviceArray (N_d, count): dF_nu[-1] / d ln alpha[k] of the last step (`.numpy()` for a host array)."""
        self._require_response()
        return self.d_Ra

    @property
    def response_source(self):
        """-> DeviceArray (N_d, count): dF_nu[-1] / dS[k] of the last step."""
        self._require_response()
        return self.d_Rs

    def _require_scattering(self):
        if self.scattering is None:
            raise RuntimeError("no scattering solution was formed: construct the synthesizer with scattering=True")

    @property
    def scattering_source(self):
        """-> DeviceArray (N_d, count): S = (1 - albedo) B + albedo J[S] of the last step's columns (`.numpy()` for a host array)."""
        self._require_scattering()
        return self.d_Ssc

    @property
    def scattering_mean_intensity(self):
        """-> DeviceArray (N_d, count): the mean intensity J of scattering_source."""
        self._require_scattering()
        return self.d_Jsc

    @property
    def scattering_flux(self):
        """-> DeviceArray (count,): the emergent flux of the last step traced with scattering_source in place of Planck (F_nu stays LTE)."""
        self._require_scattering()
        return _DeviceRow(self.d_Fsc, self.n_depth - 1)

    @property
    def scattering_iterations(self):
        """-> (count,) int32 numpy array: the iterations every column of the last step took."""
        self._require_scattering()
        return self.d_sc_iterations.numpy()

    @property
    def scattering_status(self):
        """-> (count,) int32 numpy array: 0 converged, 1 max_iter reached, 2 the change was not finite (include/stardis_hip.h)."""
        self._require_scattering()
        return self.d_sc_status.numpy()

    @property
    def scattering_accelerations(self):
        """-> (count,) int32 numpy array: the Ng extrapolations every column of the last step took (scattering=dict(acceleration="ng"))."""
        self._require_scattering()
        if self.scattering.get("acceleration") is None:
            raise RuntimeError('the scattering solve is not accelerated: construct the synthesizer with scattering=dict(acceleration="ng")')
        return self.d_sc_accelerations.numpy()

    def _require_scattering_response(self):
        if self.scattering is None or not self.keep_response:
            raise RuntimeError("no scattering responses were formed: construct the synthesizer with scattering=True and keep_response=True")

    @property
    def scattering_response_opacity(self):
        """-> DeviceArray (N_d, count): d scattering_flux / d ln alpha[k] for added TRUE ABSORPTION at fixed Thomson opacity and Planck
        function (R_absorption of sdx_scatter_response_dev): what response_opacity is to F_nu."""
        self._require_scattering_response()
        return self.d_sc_Ra

    @property
    def scattering_response_thermal(self):
        """-> DeviceArray (N_d, count): d scattering_flux / dB[k]."""
        self._require_scattering_response()
        return self.d_sc_Rt

    @property
    def scattering_response_scatter(self):
        """-> DeviceArray (N_d, count): d scattering_flux / d ln alpha_scatter[k] at fixed absorption."""
        self._require_scattering_response()
        return self.d_sc_Rs

    @property
    def scattering_response_iterations(self):
        """-> (count,) int32 numpy array: the iterations the adjoint solve of every column of the last step took."""
        self._require_scattering_response()
        return self.d_scr_iterations.numpy()

    @property
    def scattering_response_status(self):
        """-> (count,) int32 numpy array: as scattering_status, of the adjoint solve."""
        self._require_scattering_response()
        return self.d_scr_status.numpy()

    def flux_derivative(self, alpha_part, scattering=False):
        """-> DeviceArray (count,): sum_k response_opacity[k] alpha_part[k] / total_alphas[k] (sdx_response_project_dev), the derivative
        of the emergent flux with respect to the logarithm of a scale factor on the part alpha_part (N_d, count; host array,
        DeviceArray or CUDA tensor) of the last step's opacity — the line opacity of one species: dF/d ln(abundance) at fixed ionisation
        and continuum.  scattering=True: of scattering_flux, with scattering_response_opacity in response_opacity's place (the part is
        true absorption)."""
        c = self.ctx
        d_R = self.scattering_response_opacity if scattering else self.response_opacity
        d_part = self._device_vector("alpha_part", alpha_part, (self.n_depth, self.count))
        out = c.empty((self.count,))
        c.call("sdx_response_project_dev", self.n_depth, self.count, d_R.ptr, self.count, ptr_of(d_part), self.count, self.d_total.ptr,
               self.count, out.ptr)
        return out

    def _tables_in_caller_order(self):
        """The four line tables as sdx_line_adjoint_dev reads them, row k = line k of the caller's list: the uploaded dense tables
        themselves (a sorted list: nothing is copied, values overwritten in place are seen), or — built on first use and kept, a
        SNAPSHOT of the values at that moment, as large as the tables — those of a line list of scalars, materialised by
        sdx_line_params_dev (the values its pre-pass generates), or the rows of an unsorted dense list, which the constructor sorted,
        put back in the caller's order.  `forget_line_tables()` drops the snapshot; the next call builds it again."""
        if self.linelist is None and self._line_order is None:
            return self.d_ln.ptr, self.d_dw, self.d_g, self.d_a
        if self._line_tables is None:
            c = self.ctx
            if self.linelist is not None:
                ll = self.linelist
                d_a, d_g, d_dw = c.empty((self.n_lines, self.n_depth)), c.empty((self.n_lines, self.gamma_cols)), c.empty((self.n_lines, self.n_depth))
                c.call("sdx_line_params_dev", self.n_depth, ll.byref(), d_a.ptr, d_g.ptr, d_dw.ptr)
                self._line_tables = (ll.nu_ptr, d_dw, d_g, d_a)
            else:
                back = np.argsort(self._line_order, kind="stable")
                d_ln, d_dw, d_g, d_a = (c.upload(a.numpy()[back]) for a in (self.d_ln, self.d_dw, self.d_g, self.d_a))
                self._line_tables = (d_ln.ptr, d_dw, d_g, d_a, d_ln)  # (the last entry keeps the frequencies alive)
        return self._line_tables[:4]

    def forget_line_tables(self):
        """Drop the snapshot of the line tables that line_sensitivities keeps for a line list of scalars or an unsorted dense list
        (after the uploaded tables or the list's device arrays were overwritten in place)."""
        self._line_tables = None

    @staticmethod
    def _wrt_names(wrt):
        """wrt= of the sensitivities -> (names, single): one name or a tuple of names out of LINE_WRT"""
        single = isinstance(wrt, str)
        names = (wrt,) if single else tuple(wrt)
        if not names or any(k not in LINE_WRT for k in names) or len(set(names)) != len(names):
            raise ValueError(f"wrt must be one of {LINE_WRT} or a tuple of different ones, got {wrt!r}")
        return names, single

    def _line_nus_in_caller_order(self):
        """the lines' rest frequencies as a host array, row k = line k of the tables of _tables_in_caller_order"""
        if self.linelist is not None:
            return self.linelist._keep["nu"].numpy()
        if self._line_order is None:
            return self.d_ln.numpy()
        self._tables_in_caller_order()
        return self._line_tables[4].numpy()

    def microturbulence_sensitivity(self, xi, weights=None):
        """-> float: d(sum_i weights[i] F_nu_i[-1]) / d xi of the microturbulent velocity xi (cm/s) that the lines' Doppler widths were
        built with, at fixed windows and regions, from the last step.  doppler_width = nu / c sqrt(2 k T / m + xi^2)
        (sdx_broadening.h), so d ln doppler_ld / d xi = xi (nu_l / c)^2 / doppler_ld^2 whatever the mass, and the value is
        sum_{l, d} line_sensitivities(weights, per_depth=True, wrt="doppler")[l, d] xi (nu_l / c)^2 / doppler_ld^2, summed on the host
        (a diagnostic call: it waits for the stream).  The damping constants are taken not to depend on xi.  xi = 0 gives exactly 0."""
        self._require_response()
        xi = float(xi)
        if xi == 0.0:
            return 0.0
        per = self.line_sensitivities(weights, per_depth=True, wrt="doppler").numpy()
        return float(np.sum(per * self._microturbulence_direction(xi)))

    def line_sensitivities(self, weights=None, per_depth=False, wrt="strength", scattering=False):
        """-> DeviceArray (n_lines,), or (n_lines, N_d) with per_depth=True: for every line l of the list, in the order the caller passed
        the lines, the derivative of  sum_i weights[i] F_nu_i[-1]  over this synthesizer's columns with respect to ln(strength of line
        l) — ln gf, or the abundance of a species that has this line alone — at FIXED WINDOWS, from the last step: the weight plane
        weights[i] response_opacity[k, i] / total_alphas[k, i] (sdx_response_weight_dev) gathered against every line's own terms
        (sdx_line_adjoint_dev: one pass with the Voigt evaluations of one direct-sum line opacity, whatever the number of lines).
        per_depth=True keeps the depth points apart: the response to the line's strength at depth point d alone.
        weights: None (1 for every column) or one value per column of this synthesizer (host array, DeviceArray or CUDA tensor).  The
        equivalent width W = sum_i (1 - F_i / F_c) dlambda_i of a feature on a flat continuum F_c has weights[i] = -dlambda_i / F_c on
        its columns and 0 elsewhere:  dW / d ln gf_l = line_sensitivities(weights)[l].  For a functional of the OBSERVED pixels (a
        chi-square against data, a width measured on the detector, the true continuum as reference) no weights need forming by hand:
        observed_line_sensitivities(c) and chi2_line_gradient(data, ivar) pull pixel weights back through the instrument
        (pixel_weights_to_grid) and call this.
        Fixed windows: the reference's window half-width is int(max(10, (gamma + doppler) alpha / d_nu * 20)), the flux is a step
        function of a line's strength wherever that integer moves, and this is the derivative between the steps.
        The line tables: a sorted dense list is read where the step reads it; a line list of scalars and an unsorted dense list are
        read from a snapshot taken at the first call (forget_line_tables() after changing the uploaded values in place).
        A frequency shard returns the partial sum over its own columns: shards add.  Needs keep_response=True; on demand, like
        flux_derivative — a synthesizer that never asks runs the launches it always ran.
        wrt: "strength" (the above), or the derivative of the same sum with respect to a number that sets the line's SHAPE, at fixed
        windows and fixed Humlicek regions (sdx_line_param_adjoint_dev): "damping" — ln gamma_l (an enhancement factor on the damping
        constant, the same at every depth), "doppler" — ln doppler_width_l, "centre" — the rest frequency nu_l, per Hz.  A tuple of
        them returns a dict of arrays, the shape parameters from ONE pass over the terms.
        scattering=True: the derivatives of the same sum over scattering_flux — the weight plane is formed from
        scattering_response_opacity, everything behind it is the same (needs scattering=True at construction as well)."""
        names, single = self._wrt_names(wrt)
        self._require_response()
        if scattering:
            self._require_scattering_response()
        d_w = None if weights is None else self._device_vector("weights", weights, self.count, "column of the synthesizer")
        return self._sensitivities_of_response(self.d_sc_Ra if scattering else self.d_Ra, d_w, names, single, per_depth)

    def _sensitivities_of_response(self, d_R, d_w, names, single, per_depth):
        """line_sensitivities behind its response plane: the weight plane d_w[i] d_R[k, i] / total_alphas[k, i] (d_w None: 1), then the
        line adjoints for `names`.  d_R: response_opacity, scattering_response_opacity, or the plane of a per-ray cotangent
        (disk_line_sensitivities)."""
        c = self.ctx
        cnt = self.count
        d_W = c.empty((self.n_depth, cnt))
        c.call("sdx_response_weight_dev", self.n_depth, cnt, d_R.ptr, cnt, self.d_total.ptr, cnt, ptr_of(d_w), d_W.ptr, cnt)
        ln_ptr, d_dw, d_g, d_a = self._tables_in_caller_order()
        shape = (self.n_lines, self.n_depth) if per_depth else (self.n_lines,)
        res = {}
        if "strength" in names:
            out = res["strength"] = c.empty(shape)
            c.call("sdx_line_adjoint_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, cnt, self.n_lines, ln_ptr, d_dw.ptr, d_g.ptr,
                   self.gamma_cols, d_a.ptr, d_W.ptr, cnt, None if per_depth else out.ptr, out.ptr if per_depth else None)
        params = [k for k in LINE_WRT[1:] if k in names]
        if params:
            for k in params:
                res[k] = c.empty(shape)
            ptrs = [ptr_of(res.get(k)) for k in LINE_WRT[1:]]
            none = [None] * 3
            c.call("sdx_line_param_adjoint_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, cnt, self.n_lines, ln_ptr, d_dw.ptr,
                   d_g.ptr, self.gamma_cols, d_a.ptr, d_W.ptr, cnt, *(none + ptrs if per_depth else ptrs + none))
        return res[names[0]] if single else {k: res[k] for k in names}

    # -- one line alone over a background: equivalent widths and curves of growth ----------------------------------------------------------
    def equivalent_widths(self, lines=None, ln_strength=None, background=None):
        """-> (W, depth), DeviceArrays (n_sel, K): the isolated-line equivalent width in Angstrom and the line depth of every selected
        line at every strength factor exp(ln_strength), over `background` — the line alone, not its blend (sdx_line_equivalent_widths_dev;
        ops.equivalent_widths states the definition).  lines: None (all) or indices into the list in the order the caller passed it
        (repeats allowed; ValueError for one outside it); ln_strength: None, a scalar, (K,) or (n_sel, K).  background: an opacity plane
        (N_d, count) of this synthesizer's columns (host array, DeviceArray or CUDA tensor), or None: the continuum plane, formed at
        every such call by sdx_total_alphas_dev with no line plane into a buffer allocated at the first — that needs continuum=.
        The synthesizer's own shard and angles: W of frequency shards adds, depth combines by max.  The line tables as
        line_sensitivities reads them (forget_line_tables()).  On demand: a synthesizer that never asks allocates nothing and launches
        what it launched; the step's outputs are not touched."""
        c = self.ctx
        index, scale = ops.line_selection(self.n_lines, lines, ln_strength)
        if background is None and not self._has_continuum:
            raise ValueError("equivalent_widths: background=None means the continuum plane, which needs continuum= at construction")
        if self._ew is None:
            self._ew = [c.upload(K.nu_to_angstrom(self.nus_host)), None]
        d_x = self._ew[0]
        if background is None:
            if self._ew[1] is None:
                self._ew[1] = c.empty((self.n_depth, self.count))
            d_b = self._ew[1]
            c.call("sdx_total_alphas_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, self.count, C.byref(self.cont), None, 0, d_b.ptr,
                   self.count)
        else:
            d_b = self._device_vector("background", background, (self.n_depth, self.count))
        ln_ptr, d_dw, d_g, d_a = self._tables_in_caller_order()
        n_sel, k = scale.shape
        d_index = None if index is None else c.upload(index, np.int64)
        d_scale = c.upload(scale)
        out_w, out_d = c.empty((n_sel, k)), c.empty((n_sel, k))
        c.call("sdx_line_equivalent_widths_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, self.count, d_x.ptr, self.n_lines, ln_ptr,
               d_dw.ptr, d_g.ptr, self.gamma_cols, d_a.ptr, n_sel, ptr_of(d_index), k, d_scale.ptr, ptr_of(d_b), self.count, self.n_theta,
               self.d_t.ptr, self.d_ray.ptr, self.d_w.ptr, out_w.ptr, out_d.ptr)
        return out_w, out_d

    def fit_equivalent_widths(self, W_obs, lines=None, **solve_args):
        """curve_of_growth.solve over equivalent_widths: for every selected line the offset delta log gf (dex) at which its isolated-line
        equivalent width over the continuum plane equals W_obs (n_sel,) in Angstrom -> curve_of_growth.Solution."""
        from . import curve_of_growth

        return curve_of_growth.solve(lambda ln_s: self.equivalent_widths(lines=lines, ln_strength=ln_s)[0].numpy(), W_obs, **solve_args)

    # -- forward mode through the lines: one direction over the lines, every column ----------------------------------------------------
    def line_tangent(self, strength=None, damping=None, doppler=None, centre=None):
        """-> DeviceArray (N_d, count): the plane by which the line opacity of this synthesizer's columns moves, at fixed windows and
        fixed Humlicek regions, when every line moves along the given directions (sdx_line_tangent_dev, the transpose of what
        line_sensitivities gathers): strength = d ln(strength), damping = d ln gamma, doppler = d ln doppler_width, centre = d nu_l in
        Hz; each None (zero), a scalar, (n_lines,) or (n_lines, N_d), in the order the caller passed the lines.  A 0 / 1 mask over the
        lines of a species as strength gives that species' line opacity — d alpha_line / d ln(abundance) — and costs what the species
        costs.  The line tables: a dense list is read where the step reads it (sorted; the directions are permuted with it), a line
        list of scalars from the snapshot line_sensitivities keeps (forget_line_tables()).  On demand: a synthesizer that never asks
        allocates and launches nothing new.  A frequency shard returns its own columns, bit for bit those of the whole grid."""
        dirs, cols = ops.line_directions(self.n_lines, self.n_depth, strength, damping, doppler, centre)
        c = self.ctx
        if self.linelist is not None:
            ln_ptr, d_dw, d_g, d_a = self._tables_in_caller_order()  # (a line list of scalars is sorted: check_sorted)
        else:
            ln_ptr, d_dw, d_g, d_a = self.d_ln.ptr, self.d_dw, self.d_g, self.d_a
            if self._line_order is not None:
                dirs = [None if v is None else np.ascontiguousarray(v[self._line_order]) for v in dirs]
        d_dirs = [None if v is None else c.upload(v) for v in dirs]
        out = c.empty((self.n_depth, self.count))
        c.call("sdx_line_tangent_dev", self.n_depth, self.n_nu, self.d_nus.ptr, self.begin, self.count, self.n_lines, ln_ptr, d_dw.ptr,
               d_g.ptr, self.gamma_cols, d_a.ptr, *(ptr_of(v) for v in d_dirs), cols, out.ptr, self.count)
        return out

    def flux_tangent(self, strength=None, damping=None, doppler=None, centre=None):
        """-> DeviceArray (count,): the derivative of F_nu[-1] along the given line directions, from the last step:
        flux_derivative(line_tangent(...)).  Needs keep_response=True."""
        self._require_response()
        return self.flux_derivative(self.line_tangent(strength, damping, doppler, centre))

    def _microturbulence_direction(self, xi):
        """d ln doppler_ld / d xi = xi (nu_l / c)^2 / doppler_ld^2 (microturbulence_sensitivity's factor), rows in the caller's order"""
        dw = self._tables_in_caller_order()[1].numpy()
        nu_over_c = self._line_nus_in_caller_order() / K.C_CGS
        return float(xi) * (nu_over_c * nu_over_c)[:, None] / (dw * dw)

    def microturbulence_tangent(self, xi):
        """-> DeviceArray (count,): d F_nu[-1] / d xi per column, of the microturbulent velocity xi (cm/s) the lines' Doppler widths
        were built with — the forward twin of microturbulence_sensitivity: flux_tangent(doppler=xi (nu_l / c)^2 / doppler_ld^2).  The
        damping constants are taken not to depend on xi.  xi = 0 gives zeros.  Needs keep_response=True."""
        self._require_response()
        if float(xi) == 0.0:
            return self.ctx.zeros((self.count,))
        return self.flux_tangent(doppler=self._microturbulence_direction(xi))

    def observed_line_jacobian(self, directions, normalized=False):
        """-> {name: DeviceArray (n_pix,)}: for every entry name -> dict of line directions (flux_tangent's keywords; or
        {"microturbulence": xi}) the column d observed_j / d p of the global parameter p that moves the lines along them, at the last
        step's spectrum: observed_tangent(flux_tangent(...)).  normalized=True: of observed_normalized; the continuum does not move.
        Needs instrument= and keep_response=True."""
        self._require_instrument()
        self._require_response()
        if normalized:
            self._require_continuum()
        out = {}
        for name, dirs in dict(directions).items():
            dirs = dict(dirs)
            if set(dirs) == {"microturbulence"}:
                d_f = self.microturbulence_tangent(dirs["microturbulence"])
            else:
                d_f = self.flux_tangent(**dirs)
            out[name] = self.observed_tangent(d_f, None, normalized)
        return out

    def _require_instrument(self):
        if self.instrument is None:
            raise RuntimeError("no instrument: construct the synthesizer with instrument=Instrument(...)")

    def _require_macroturbulence(self):
        self._require_instrument()
        if not self.instrument.macroturbulent:
            raise RuntimeError("no macroturbulence: construct the Instrument with v_mac=")
        if not self.instrument.v_mac > 0.0:
            raise ValueError("the derivative to zeta needs zeta > 0 (at zeta = 0 the stage is a copy)")

    def _pixel_vector(self, name, c):
        """a vector over the instrument's pixels (host array, DeviceArray or CUDA tensor) -> a device buffer; ValueError naming it"""
        return self._device_vector(name, c, self.instrument.n_pix, "pixel of the instrument")

    def pixel_weights_to_grid(self, c, normalized=False, with_continuum=False):
        """-> DeviceArray (n_nu,): the weights w over the columns of F_nu[-1] with  sum_j c_j observed_j = sum_i w_i F_nu_i[-1]  over the
        pixels the grid covers (c of a NaN pixel is never read) — the instrument transposed (sdx_observe_adjoint_dev, the factor nu /
        lambda of F_lambda applied), at the instrument's present radial velocity.  c: one value per pixel (host array, DeviceArray or
        CUDA tensor).  normalized=True: the weights of observed_normalized instead, its derivative to F_nu[-1] at the last step's
        F_lambda and continuum (needs keep_continuum_flux=True).  with_continuum=True -> (w, w_continuum), the second over the
        columns of F_nu_continuum[-1] (zeros unless normalized: the plain observed spectrum does not depend on the continuum).  On demand, after a step: what feeds line_sensitivities(weights=...)."""
        self._require_instrument()
        if normalized:
            self._require_continuum()
        d_c = self._pixel_vector("c", c)
        inst, n = self.instrument, self.n_nu
        if not normalized:  # (the plain observed spectrum does not depend on the continuum: its weights there are zeros)
            w = inst.adjoint(self.d_lambdas, n, d_c, nus=self.d_nus)
            return (w, self.ctx.zeros((n,))) if with_continuum else w
        return inst.adjoint(self.d_lambdas, n, d_c, flux=self.d_Flam, reference=self.d_Fclam, nus=self.d_nus, out_reference=bool(with_continuum))

    def observed_line_sensitivities(self, c, normalized=False, per_depth=False, wrt="strength"):
        """-> DeviceArray (n_lines,), or (n_lines, N_d) with per_depth=True: d(sum_j c_j observed_j) / d ln gf_l for every line of the
        list, at fixed windows, from the last step — line_sensitivities(weights=pixel_weights_to_grid(c, normalized), per_depth): the
        chain response functions -> line adjoint -> instrument, from the detector's pixels to every line.  normalized=True: of
        observed_normalized; the zero-line continuum does not depend on the lines, so its cotangent does not enter.  Needs
        instrument= and keep_response=True (normalized: keep_continuum_flux=True).  wrt: as for line_sensitivities."""
        self._wrt_names(wrt)
        self._require_instrument()
        self._require_response()
        return self.line_sensitivities(weights=self.pixel_weights_to_grid(c, normalized), per_depth=per_depth, wrt=wrt)

    def chi2_line_gradient(self, data, inverse_variance, normalized=False, per_depth=False, wrt="strength"):
        """-> (chi2, DeviceArray): chi2 = sum_j ivar_j (data_j - observed_j)^2 of the last step's observed (normalized=True:
        observed_normalized) spectrum against data, and its gradient to ln gf of every line, (n_lines,) or (n_lines, N_d):
        observed_line_sensitivities with c_j = -2 ivar_j (data_j - observed_j).  A pixel whose observed value is NaN (the grid does not
        cover its window) or whose ivar is 0 is left out of both; leaving every pixel out is a ValueError.  data, inverse_variance:
        host arrays, one value per pixel.  With rotation or macroturbulence (Instrument(v_rot=..., v_mac=...)) the pixels it reports
        as edge_affected — those that may see a point whose broadening window is truncated at an end of the grid — are left out in
        the same way.  A
        diagnostic call, not part of the step: it waits for the stream and forms the n_pix residuals on the host.  wrt: as for
        line_sensitivities (a tuple: the gradient is a dict)."""
        self._wrt_names(wrt)
        self._require_instrument()
        self._require_response()
        chi2, c, _, _ = self._chi2_pixel_weights(data, inverse_variance, normalized)
        return chi2, self.observed_line_sensitivities(c, normalized, per_depth, wrt)

    def _chi2_pixel_weights(self, data, inverse_variance, normalized, observed=None, v_rot=None):
        """-> (chi2, c, use, w): chi-square over the pixels chi2_line_gradient uses, c_j = d chi2 / d observed_j = -2 ivar_j (data_j -
        observed_j), 0 at the pixels left out, the mask of the pixels used and the inverse variance, 0 at the others.  The one
        download of the observed spectrum of a chi-square call.  observed, v_rot: a host spectrum in the step's place and the
        rotation whose reach decides the edge-affected pixels (chi2_disk_gradient: the disk integration is no stage of the instrument)."""
        if normalized:
            self._require_continuum()
        n_pix = self.instrument.n_pix
        d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        ivar = np.ascontiguousarray(inverse_variance, dtype=np.float64).reshape(-1)
        for name, v in (("data", d), ("inverse_variance", ivar)):
            if v.size != n_pix:
                raise ValueError(f"{name} must hold one value per pixel of the instrument ({n_pix}), got {v.size}")
        obs = (self.d_observed_normalized if normalized else self.d_observed).numpy() if observed is None else observed
        use = ~np.isnan(obs) & (ivar != 0)
        if v_rot is not None:
            use &= ~self.instrument.edge_affected(self.lambdas, v_rot=v_rot)
        elif self.instrument.broadens:
            use &= ~self.instrument.edge_affected(self.lambdas)
        if not np.any(use):
            raise ValueError("no pixel left: every pixel is NaN (not covered by the grid), edge-affected or has inverse_variance 0")
        r = np.where(use, d, 0.0) - np.where(use, obs, 0.0)
        w = np.where(use, ivar, 0.0)
        return float(np.sum(w * r * r)), -2.0 * w * r, use, w

    @staticmethod
    def _chi2_normal_equations(chi2, c, use, w, names, columns, curvature):
        """-> (chi2, gradient) or (chi2, gradient, H) of the parameters `names` from their columns d observed / d p (device arrays, by
        name): the sums over the pixels used, taken on the host (math.fsum of the fp64 products)"""
        J = {k: np.where(use, columns[k].numpy(), 0.0) for k in names}
        grad = {k: math.fsum(c * J[k]) for k in names}
        if not curvature:
            return chi2, grad
        H = np.empty((len(names), len(names)))
        for ia, a in enumerate(names):  # (the upper triangle, mirrored: symmetric bit for bit)
            for ib in range(ia, len(names)):
                H[ia, ib] = H[ib, ia] = 2.0 * math.fsum(w * J[a] * J[names[ib]])
        return chi2, grad, H

    def observed_macroturbulence_derivative(self, c, normalized=False):
        """-> float: d(sum_j c_j observed_j) / d zeta per km/s (normalized=True: of observed_normalized) at the last step's spectrum
        and the instrument's present zeta, at fixed windows — the first instrument-PARAMETER derivative.  On demand, a diagnostic
        call like chi2_line_gradient: the stages in front of the macroturbulence run again, then one k_macroturbulence with its
        derivative outputs (d / d ln zeta of the broadened flux and continuum, from the terms the profile is made of) and one
        k_observe_adjoint for the weights w over the BROADENED points; the result is sum_i (w_flux_i dout_i + w_reference_i
        dout_reference_i) / zeta, summed ON THE HOST after one download (math.fsum of the fp64 products: exactly rounded, so the
        same bits everywhere).  c: one value per pixel; c of a NaN pixel is never read.  Needs Instrument(v_mac=...) with zeta > 0."""
        self._require_macroturbulence()
        inst, n = self.instrument, self.n_nu
        if normalized:
            self._require_continuum()
        d_c = self._pixel_vector("c", c)
        ref = self.d_Fclam if normalized else None
        flux = self.d_Flam
        if inst.rotates:
            res = inst.rotate(self.d_lambdas, flux, n, reference=ref)
            flux, ref = res if normalized else (res, None)
        d_dout, d_w = self.ctx.empty((n,)), self.ctx.empty((n,))
        d_dref, d_wref = (self.ctx.empty((n,)), self.ctx.empty((n,))) if normalized else (None, None)
        res = inst.macroturbulence(self.d_lambdas, flux, n, reference=ref, dout=d_dout, dout_reference=d_dref)
        flux, ref = res if normalized else (res, None)
        self.ctx.call("sdx_observe_adjoint_dev", n, self.d_lambdas.ptr, flux.ptr if normalized else None, _lib.ptr_of(ref), inst.n_pix,
                      inst.d_edges.ptr, inst.d_sigma.ptr, inst.d_doppler.ptr, _lib.ptr_of(d_c), None, d_w.ptr, _lib.ptr_of(d_wref))
        terms = d_w.numpy() * d_dout.numpy()
        if normalized:
            terms = np.concatenate([terms, d_wref.numpy() * d_dref.numpy()])
        return math.fsum(terms) / inst.v_mac

    def chi2_macroturbulence_gradient(self, data, inverse_variance, normalized=False):
        """-> (chi2, d chi2 / d zeta): chi-square of the last step's observed (normalized=True: observed_normalized) spectrum against
        data over the pixels chi2_line_gradient uses (NaN, inverse_variance 0 and edge_affected pixels left out), and its derivative
        to the macroturbulence zeta per km/s: observed_macroturbulence_derivative with c_j = -2 ivar_j (data_j - observed_j).  No
        v_mac, or zeta = 0, raises."""
        self._require_macroturbulence()
        chi2, c, _, _ = self._chi2_pixel_weights(data, inverse_variance, normalized)
        return chi2, self.observed_macroturbulence_derivative(c, normalized)

    # -- forward mode: one direction, every pixel ---------------------------------------------------------------------------------
    def _column_tangent(self, name, v):
        """a tangent over the columns of F_nu[-1] (host array, DeviceArray or CUDA tensor) -> F_lambda's tangent on the device:
        the factor nu / lambda of sdx_flux_nu_to_lambda_dev applied"""
        n = self.n_nu
        d_v = self._device_vector(name, v, n, "column of the spectrum", at_least=True)  # (a longer device buffer passes, as it always did)
        out = self.ctx.empty((n,))
        self.ctx.call("sdx_flux_nu_to_lambda_dev", n, ptr_of(d_v), self.d_nus.ptr, self.d_lambdas.ptr, out.ptr)
        return out

    def observed_tangent(self, dF_nu, dF_nu_continuum=None, normalized=False):
        """-> DeviceArray (n_pix,): a tangent dF_nu over the columns of F_nu[-1] — flux_derivative(...)'s dF/d ln(abundance), say —
        pushed to the detector's pixels at the last step's spectrum: the factor nu / lambda, then Instrument.tangent (rotation,
        macroturbulence, sdx_observe_tangent_dev).  normalized=True: the tangent of observed_normalized (needs
        keep_continuum_flux=True), with dF_nu_continuum the tangent of F_nu_continuum[-1] (None: the continuum does not move).
        NaN where the observed spectrum is NaN.  On demand, after a step."""
        self._require_instrument()
        if dF_nu_continuum is not None and not normalized:
            raise ValueError("dF_nu_continuum enters the normalised spectrum only: pass normalized=True")
        if normalized:
            self._require_continuum()
        d_f = self._column_tangent("dF_nu", dF_nu)
        d_g = None if dF_nu_continuum is None else self._column_tangent("dF_nu_continuum", dF_nu_continuum)
        return self.instrument.tangent(self.d_lambdas, self.n_nu, self.d_Flam, d_f, reference=self.d_Fclam if normalized else None,
                                       dreference=d_g)

    def observed_jacobian(self, wrt, normalized=False):
        """-> {name: DeviceArray (n_pix,)}: the columns d observed_j / d p (normalized=True: of observed_normalized) of the
        instrument's parameters at the last step's spectrum — Instrument.parameter_tangents: "v_rad" per km/s, "lsf" per ln of a
        common factor on sigma (-d / d ln R), "v_mac" per km/s, "limb_darkening" per unit; a single name gives a one-entry dict.  v sin i
        has no column (see Instrument.parameter_tangents).  On demand, after a step."""
        self._require_instrument()
        if normalized:
            self._require_continuum()
        return self.instrument.parameter_tangents(self.d_lambdas, self.n_nu, self.d_Flam, reference=self.d_Fclam if normalized else None,
                                                  wrt=wrt)

    def chi2_instrument_gradient(self, data, inverse_variance, wrt, normalized=False, curvature=False):
        """-> (chi2, {p: d chi2 / d p}), with curvature=True -> (chi2, gradient, H): chi-square of the last step's observed
        (normalized=True: observed_normalized) spectrum against data over the pixels chi2_line_gradient uses (NaN, inverse_variance 0
        and edge_affected pixels left out), its derivative to the instrument parameters named by wrt (observed_jacobian's names and
        units) and the Gauss-Newton matrix H = 2 J^T W J, H[a][b] = 2 sum_j ivar_j J_ja J_jb in the order of wrt.  The tangent route:
        the columns J are downloaded and the sums are taken ON THE HOST (math.fsum of the fp64 products: exactly rounded, the same
        bits everywhere), as observed_macroturbulence_derivative takes its own."""
        self._require_instrument()
        names = self.instrument._wrt(wrt)
        chi2, c, use, w = self._chi2_pixel_weights(data, inverse_variance, normalized)
        return self._chi2_normal_equations(chi2, c, use, w, names, self.observed_jacobian(names, normalized), curvature)

    def chi2_joint_gradient(self, data, inverse_variance, instrument_wrt=(), line_directions=None, normalized=False, curvature=False):
        """-> (chi2, {p: d chi2 / d p}), with curvature=True -> (chi2, gradient, H): chi2_instrument_gradient over the instrument
        parameters named by instrument_wrt AND the global line parameters of line_directions (observed_line_jacobian's argument)
        together — the gradient and the Gauss-Newton matrix H = 2 J^T W J of one fit of both, rows and columns in the order
        instrument_wrt, then line_directions.  The same pixels and the same host sums (math.fsum) as chi2_instrument_gradient; with
        no line direction it IS chi2_instrument_gradient."""
        line_directions = dict(line_directions or {})
        if not line_directions:
            return self.chi2_instrument_gradient(data, inverse_variance, instrument_wrt, normalized, curvature)
        self._require_instrument()
        self._require_response()
        none_asked = instrument_wrt is not None and not isinstance(instrument_wrt, str) and len(tuple(instrument_wrt)) == 0
        inst_names = () if none_asked else self.instrument._wrt(instrument_wrt)
        clash = [k for k in line_directions if k in inst_names]
        if clash:
            raise ValueError(f"line_directions reuses the instrument's parameter names {clash}")
        chi2, c, use, w = self._chi2_pixel_weights(data, inverse_variance, normalized)
        columns = dict(self.observed_jacobian(inst_names, normalized)) if inst_names else {}
        columns.update(self.observed_line_jacobian(line_directions, normalized))
        return self._chi2_normal_equations(chi2, c, use, w, tuple(inst_names) + tuple(line_directions), columns, curvature)

    @property
    def observed(self):
        """-> DeviceArray (n_pix,): the last step's spectrum as the instrument records it (`.numpy()` for a host array)."""
        self._require_instrument()
        return self.d_observed

    @property
    def observed_normalized(self):
        """-> DeviceArray (n_pix,): the continuum-normalised observed spectrum of the last step."""
        self._require_instrument()
        self._require_continuum()
        return self.d_observed_normalized

    def formation_mean(self, x):
        """-> DeviceArray (count,): the formation mean of a per-depth quantity x (N_d values; host array, DeviceArray or CUDA tensor)
        under the last step's contribution function (sdx_formation_mean_dev)."""
        c = self.ctx
        d_C = self.contribution
        d_x = self._device_vector("x", x, self.n_depth, "depth point", at_least=True)  # (a longer device buffer passes, as it always did)
        out = c.empty((self.count,))
        c.call("sdx_formation_mean_dev", self.n_depth, self.count, d_C.ptr, self.count, ptr_of(d_x), out.ptr)
        return out

    def total_alphas(self):
        if not self.keep_total:
            raise RuntimeError("total_alphas was not kept: construct the synthesizer with keep_total=True")
        return self.d_total.numpy()

    def alpha_line(self):
        if not self.keep_line:
            raise RuntimeError("alpha_line was not kept: construct the synthesizer with keep_line=True")
        return self.d_line.numpy()

    def evaluations(self):
        return int(self.d_evals.numpy()[0]) if self.d_evals is not None else None

    def algorithmic_bytes(self):
        """line list, grid read once; total_alphas and F_nu written once (this shard's columns)."""
        if self.linelist is not None:
            lines = self.n_lines * self.linelist.host.bytes_per_line() + 8 * self.linelist.host.pop.size
        else:
            lines = 8 * self.n_lines * (1 + 2 * self.n_depth + self.gamma_cols)
        return lines + 8 * self.n_nu + 16 * self.n_depth * self.count

    def close(self):
        """Destroy the recorded graphs and the grid plan (a step after close() runs without one)."""
        self._destroy_graphs()
        plan, self.plan = getattr(self, "plan", None), None
        if plan is not None and self.ctx.handle:
            self.ctx.lib.sdx_grid_plan_destroy(plan)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _destroy_graphs(self):
        for which in ("graph", "graph_classify", "graph_batch"):
            if getattr(self, which) is not None:
                self.ctx.call("sdx_graph_destroy", getattr(self, which))
                setattr(self, which, None)
        self.batch = 1


class SynthesisPool:
    """Several independent syntheses in flight on one GPU — a grid of stars, abundances or line lists.  Members are
    dealt round-robin onto `n_streams` contexts (each its own HIP stream and scratch), so kernels of different members
    overlap on the device: the formal solution of one fills the issue slots the line kernel of another leaves idle
    (S-c2: about 4.7e9 spectral points/s with two in flight against 3.8e9 one after the other).  Every member computes exactly
    what it would alone."""

    def __init__(self, device=None, n_streams=2):
        import os

        dev = int(os.environ.get("STARDIS_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0"))) if device is None else int(device)
        self.contexts = [_lib.Context(dev) for _ in range(max(1, int(n_streams)))]
        self.members = []

    def add(self, *args, capture=True, **kwargs):
        """SpectralSynthesizer(*args, **kwargs) on the next context; captured into a hipGraph unless capture=False."""
        kwargs["ctx"] = self.contexts[len(self.members) % len(self.contexts)]
        syn = SpectralSynthesizer(*args, **kwargs)
        if capture:
            syn.count_evaluations = False
            syn.capture()
        self.members.append(syn)
        return syn

    def step(self):
        """Enqueue one step of every member (returns at once; members on different contexts run concurrently)."""
        for syn in self.members:
            syn.step()

    def synchronize(self):
        for c in self.contexts:
            c.synchronize()

    def fluxes(self):
        self.synchronize()
        return [syn.F_nu() for syn in self.members]

    def close(self):
        for syn in self.members:
            syn.close()
        self.members = []
