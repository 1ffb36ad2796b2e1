/*
 * stardis_hip.h — C ABI of libstardis_hip.so: the STARDIS radiation-field hot path on MI355X (gfx950).
 *
 * The reference (tardis-sn/stardis) has no FFI or plugin registry: its hot path sits behind plain
 * Python callables whose numeric seam is "contiguous float64 ndarrays in, ndarray out" into numba
 * kernels.  Each entry point below replaces one of those numba kernels / array functions; the
 * citation on each is the reference interface it stands in for (paths relative to stardis/).
 * INTEGRATION.md shows the ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - All arithmetic is IEEE fp64.  Arrays are C-order.  int64_t sizes for the frequency / line axes.
 *   - Functions ending in _dev take DEVICE pointers and enqueue work on the context's stream
 *     (asynchronous; call sdx_synchronize or use stream order).  Functions ending in _f64 take HOST
 *     pointers, copy in, run, copy out and return after the result is on the host (what a numpy
 *     caller binds).
 *   - Return value: 0 = ok, <0 = error (SDX_ERR_*); text via sdx_last_error_string() (thread-local).
 *   - The library never keeps a caller pointer past the call.  Device scratch is owned by the context.
 *   - A context is bound to one device and one stream; use one context per host thread.
 *
 * Environment
 *   The library's results do not depend on the environment.  Two variables are read unconditionally, neither changes a
 *   computed number: SDX_RCCL_LIB (path of the RCCL library opened by sdx_group_create) and SDX_EXPERIMENT.  Everything
 *   else is an experiment / analysis knob that is honoured ONLY when SDX_EXPERIMENT=1 is set as well (tests/test_gpu_round4.py
 *   runs a synthesis under a hostile environment without the switch and compares bits):
 *     changes kernel choice or summation order (last bits of a result; shards of one spectrum must agree on them):
 *       SDX_WIDE_BLOCKS   target number of wide-role workgroups -> line subsets per (depth, tile)
 *       SDX_RT_SEG        0 / 1 / 2: never / always the segmented formal-solution kernel, 2 preferring its step-shaped form (the option
 *                         "segmented_raytrace" wins; same values)
 *     scheduling only (same bits): SDX_NO_PINNED_STAGING,
 *       SDX_SPLIT_LAUNCHES (the line kernel as two launches, for profiling: the far and the wide role, then the narrow role)
 *     test hook: SDX_GROUP_LOOPBACK (see sdx_group_create).
 */
#ifndef STARDIS_HIP_H
#define STARDIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDX_OK 0
#define SDX_ERR_ARG (-1)  /* bad argument: null pointer, non-monotone grid, zero Doppler width ... */
#define SDX_ERR_HIP (-2)  /* HIP runtime error (no device, launch failure, ...) */
#define SDX_ERR_COMM (-3) /* RCCL error: library not loadable, communicator set-up or the collective itself (sdx_group_*) */
#define SDX_ERR_OOM (-4)  /* device or host allocation failed */
#define SDX_ERR_STALE (-5) /* sdx_graph_launch: the context's scratch was reallocated after the graph was captured; capture again */

/* broadening flags (broadening.py:688-691: which terms the config lists) */
#define SDX_LINEAR_STARK 1
#define SDX_QUADRATIC_STARK 2
#define SDX_VAN_DER_WAALS 4
#define SDX_RADIATION 8

typedef struct sdx_ctx sdx_ctx;

/* ---- runtime -------------------------------------------------------------------------------- */
const char* sdx_version(void);
const char* sdx_last_error_string(void);
int sdx_last_error_code(void); /* the SDX_ERR_* behind the last message (for entry points that return a pointer) */
int sdx_device_count(void); /* number of visible HIP devices, 0 when none (never an error) */
/* hipSetDevice for the calling thread: for callers that allocate device memory of their own next to a context (every sdx_* entry
 * point that takes a context selects the context's device itself where it matters) */
int sdx_set_device(int device);

/* One context per device.  stream = NULL: the context creates its own non-blocking stream;
 * otherwise an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
sdx_ctx* sdx_create(int device, void* stream);
void sdx_destroy(sdx_ctx* ctx);
int sdx_set_stream(sdx_ctx* ctx, void* stream);
void* sdx_get_stream(sdx_ctx* ctx);
int sdx_synchronize(sdx_ctx* ctx);
/* options:
 *   "indexed_min_lines" (default 8192): line lists at least this long are not scanned completely by every tile of the wide
 *       role: lines whose widest window exceeds 4096 grid points are listed once and visited by every tile, all others are
 *       found by centre range (the list is sorted); frequency shards of such lists also run a culled pre-pass.
 *   "prepass_ticket_min_blocks" (default 16384): frequency shards of long lists — from this many 32-line blocks on (5e5 lines) the
 *       culled pre-pass runs as many workgroups as the chip holds, drawing the blocks that have work from a counter, instead of one
 *       workgroup per candidate block (most of which return at once).  Scheduling only: the same bits.
 *   "mixed_precision" (default 0): 1 selects the fp32-mixed TOLERANCE path (BASELINE config 5).  Wide windows: far-wing
 *       evaluations — grid tiles wholly inside a line's window and wholly in Faddeeva region I, and window edges — compute
 *       the rational y (q + y^2 + 1/2) / ((q - y^2 - 1/2)^2 + 4 q y^2) in packed fp32, two grid points per instruction:
 *       x = (nu_i - nu_l) / doppler from hi + lo fp32 splits of both frequencies (relative error ~1e-7 whatever their
 *       distance), fp32 constants per (line, depth) written by the pre-pass, v_rcp_f32, fp32 running sums flushed into the
 *       fp64 sums every >= 48 terms.  Narrow windows (half-width <= 64 grid points) and the line cores delegated to them:
 *       all four Humlicek regions in fp32 with packed complex arithmetic and the hardware exp / cos
 *       (sdx_voigt_term_f32_dev exposes that routine).  Line cores kept by the wide windows, the continuum and the formal
 *       solution stay fp64.  Stated tolerance: 1e-4 relative on the emergent flux (measured: 7e-6 on the line opacity, 7e-6
 *       of Re w per evaluation; tests/test_gpu_configs.py, tests/test_gpu_hot_faddeeva.py).  fp64 remains the default and
 *       the parity path.  Where the reference divides by zero — an opaque gap with a TRANSPARENT gap ahead of it on the ray
 *       (radiation_field_solvers/base.py:208-249 with tau[gap + 1] = 0) — the fp64 kernels reproduce its NaN; the fp32 formal
 *       solution of this mode takes that step to first order and stays finite.
 *   "segmented_raytrace" (default -1): which formal-solution kernel runs.  -1: decided from the size of the GLOBAL grid against
 *       a fixed constant (grids under 3 x 4 x 256 k_raytrace waves take the segmented kernel) — never from the shard's own
 *       width or the device's CU count, so that a frequency shard and the unsharded grid run the same arithmetic and stay
 *       bit-identical; 0: never the segmented kernel; 1: whenever it supports the shape, always the general kernel
 *       k_raytrace_seg<8,7>; 2: whenever it supports the shape, and k_raytrace_seg_step<8,7> for the launches that have the shape
 *       of the fused synthesis step (a fused total of 0, 2 or 3 line planes, the Planck source, no extra line plane, no
 *       alpha_line_out, no I_nus, F_nu requested; the continuum launch of F_nu_continuum too) — the same arithmetic in the same
 *       order as the general kernel, so the same bits, with less fixed cost per wave.  -1 takes the step kernel under the same
 *       rule wherever it chooses the segmented one.  The fp32-mixed twins (*_f32mix) that
 *       SURVEY §8b proposed exist for the host-buffer entry points (below) and are this library's "mixed_precision" option for the rest.
 *   "far_field" (default -1): the far field of the line opacity.  A (line, depth) item whose window (base.py:561-575) contains a whole
 *       256-point tile of the GLOBAL grid, clear of the line's core range (every point of the tile in Faddeeva region I) and with the
 *       line's centre at least three tile widths (6 half-widths, measured in frequency) from the tile's centre, is not evaluated at
 *       the tile's 256 grid points but at its 16 Chebyshev nodes — the same region-I rational, fp64 — and the summed node values are
 *       carried to the grid points by the degree-15 interpolant (the far role of the line kernel's launch; a third partial plane).  Nine tenths of the window
 *       evaluations of the 3000 - 10000 A workloads are such triples.  Interpolation error <= 11.9^-16 = 6e-18 of an item's value;
 *       measured against the direct sum: <= 7e-15 relative on the line opacity, 7e-13 on the flux (tolerances 1e-12 / 1e-10).
 *       Which triples are far is a property of the grid and the list, not of the shard: shards stay bit-identical to the unsharded
 *       run.  -1: grids of at least 32768 frequencies (decided from the GLOBAL grid); 0: never — every window point is evaluated
 *       where it lies, as the reference does; 1: whenever the line kernel runs 256-point tiles (always, unless an experiment knob
 *       says otherwise).  With "mixed_precision" = 1 the far field and what it leaves to the wide windows (a line's near zone, window
 *       edges) are evaluated in fp64 as in the fp64 mode — the far wings that mode computed in fp32 are the far field's now —; narrow
 *       windows, delegated cores and the formal solution stay fp32. 
 *   "narrow_records" (default -1): where the narrow role of the line kernel (windows of at most 64 points, delegated line cores) finds 1 / dw, y
 *       and the amplitude of a (line, depth) item.  1: in records the pre-pass writes (24 bytes per narrow item); 0: it forms them itself from
 *       the caller's doppler widths, gammas and alphas — the same three operations, so the results are bit-identical — and the pre-pass
 *       writes one byte per item (long dense fp64 lists only: lists of at least "indexed_min_lines" lines, no line-list scalars, no
 *       "mixed_precision"); -1: 0 for lists of at least four lines per grid point (1e6 lines: 1.35 GB less traffic and scratch per
 *       synthesis, the step 0.5 % faster), 1 otherwise (1.5e5 lines: the step is 0.4 % slower without the records).
 *   "adjoint_partials" (default 2^22, at least 1): how many doubles sdx_line_adjoint_dev may spend on the partial sums of its tiled role
 *       (windows of more than 4096 points; at least one per (line, depth) item is always there).  It bounds the number of supertiles — runs
 *       of consecutive 1024-column tiles whose sums one wave adds — per item: min(tiles of the shard, partials / tiled items).  Scheduling
 *       and scratch only, but not bit-neutral: another number of supertiles adds an item's tiles in another grouping (the results stay
 *       deterministic and within the rounding of the sum).  32 MB at the default; tests lower it to run several tiles per supertile.
 *       sdx_line_param_adjoint_dev keeps four sums per item: there the option bounds groups of four doubles per (tiled item, supertile),
 *       min(tiles of the shard, (partials / 4) / tiled items) supertiles per item, and at least one group per item is always there.
 *   "wide_list" (default -1): how the wide role of the line kernel finds its candidates in a SHORT list (fewer than "indexed_min_lines"
 *       lines; long lists have the list launches).  0: every tile tests every line of its line subset, 64 per round trip.  1: the last
 *       line block of the pre-pass launch to finish lists the lines that have a wide window (half-width > 64 grid points) at any depth,
 *       one ascending list per line subset, and a tile tests those alone — the lines it would have met as possible hits, in the same
 *       order: the same hits, the same sums, bit-identical results (tests/test_gpu_wide_list.py).  No further launch; the list is built
 *       for dense tables and line-list inputs, whole grids and frequency shards.  The fp32-mixed mode keeps the full scan whatever the
 *       option says (its fp32 partial sums are flushed at chunk boundaries, which a compacted list would move).  -1: 1 for lists of at
 *       least 16 chunks of 64 lines per line subset (2000 lines on 7634 points, two subsets: the line kernel 1.2 us faster, the list
 *       built in the shadow of the launch's continuum tiles), 0 below (2000 lines on 1000 points, eight subsets: nothing gained and 3 us
 *       more at the end of the pre-pass launch).
 *   "grid_plan" (default -1): -1: a step that is given an sdx_grid_plan (sdx_synthesis_options.grid_plan) uses it; 0: the plan is
 *       checked and then ignored — the step runs the kernels it runs without one (A/B runs inside one library).  The same bits
 *       either way. */
int sdx_set_int_option(sdx_ctx* ctx, const char* name, int64_t value);
/* The far-field rule as the library applies it — for planners that weigh shards (stardis_amd.parallel.column_cost) and must not
 * carry constants of their own.  sdx_far_field_active: 1 when a synthesis of a GLOBAL grid of n_nu_global points on this context runs
 * with the far field (the "far_field" option, else the automatic rule: grids of at least *min_points), 0 when not, negative on a null
 * context.  sdx_far_field_rule: the rule's constants — the automatic threshold, the tile the far field lives on (grid points) and how
 * close to its centre, in grid points, a window is still evaluated point by point (half a tile + the pole-distance ratio in tile
 * half-widths).  Replaces nothing in the reference (its sum is always the direct one, opacities_solvers/base.py:577-592). */
int sdx_far_field_active(const sdx_ctx* ctx, int64_t n_nu_global);
int sdx_far_field_rule(int64_t* min_points, int* tile_points, int* near_points);
/* Which way the continuum plane of the last fused step on this context was computed, as the site that enqueued its launch decided
 * it (tests assert the route they mean to exercise; nothing here changes a launch).  Fills out[0 .. min(n_out, 10)):
 * [0] kernel: 0 no fused continuum launch yet, 1 the pre-pass launch (k_prepass_continuum), 2 the classification launch of a culled
 * shard or of the two-collective mode (k_classify_continuum); [1] 1: depth-group tiles, 0: one block per (tile, depth) that evaluates
 * every point from scratch (more bound-free levels than the tiles' per-depth factors fit in 48 KiB of LDS); [2] depths per block (1..8;
 * 1 when untiled); [3] 1: the 1-D cross-section table is searched from LDS (at most 1024 nodes), 0: from global memory, or there is
 * none, or the launch is planned; [4] 1: the launch honoured an sdx_grid_plan; [5] threads per block; [6] frequency tiles;
 * [7] block rows (depth groups); [8] dynamic LDS of the launch in bytes; [9] the device's compute units, which the choice of [2]
 * depends on.  A step of the two-collective mode reports the launch of its phase 1. */
int sdx_continuum_route(const sdx_ctx* ctx, int64_t* out, int n_out);

/* device memory for callers that do not bring their own (numpy-only users) */
/* (freed blocks are kept by the context — up to 4 GiB — and handed out again: all uses are ordered on the context's stream, so the
 * Python mirror's ~30 small uploads per drop-in call cost no hipMalloc / hipFree after the first call) */
void* sdx_malloc(sdx_ctx* ctx, size_t bytes);
int sdx_free(sdx_ctx* ctx, void* ptr);
int sdx_memcpy_h2d(sdx_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes); /* async on ctx stream */
int sdx_memcpy_d2h(sdx_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* synchronises */
int sdx_memset(sdx_ctx* ctx, void* dst_dev, int value, size_t bytes);
/* Page-locked host memory (hipHostMalloc) for callers that keep staging / result buffers of their own, and copies that move it
 * by DMA directly — sdx_memcpy_h2d / _d2h above take pageable pointers and go through a bounce buffer of the context.
 * sdx_memcpy_h2d_pinned is asynchronous on the context's stream: the source must stay untouched until a synchronising call
 * (sdx_memcpy_d2h[_pinned], sdx_synchronize) has returned.  sdx_host_alloc returns NULL on failure (-4 in sdx_last_error_code). */
void* sdx_host_alloc(sdx_ctx* ctx, size_t bytes);
int sdx_host_free(void* ptr);
int sdx_memcpy_h2d_pinned(sdx_ctx* ctx, void* dst_dev, const void* src_pinned, size_t bytes);
int sdx_memcpy_d2h_pinned(sdx_ctx* ctx, void* dst_pinned, const void* src_dev, size_t bytes); /* synchronises */

/* Scratch the line-opacity call needs for n_lines x n_depth; call once before stream capture. */
int sdx_reserve_line_workspace(sdx_ctx* ctx, int n_depth, int64_t n_lines);

/* stream capture -> hipGraph, so a launch-bound sequence of *_dev calls replays as one submit.  A graph bakes in the
 * context's scratch pointers: if a later, larger call on the same context makes the library reallocate scratch, launching
 * the old graph returns SDX_ERR_STALE instead of touching freed memory (reserve the largest workspace first, or re-capture). */
int sdx_graph_begin(sdx_ctx* ctx);
int sdx_graph_end(sdx_ctx* ctx, void** graph_exec_out);
int sdx_graph_launch(sdx_ctx* ctx, void* graph_exec);
int sdx_graph_destroy(sdx_ctx* ctx, void* graph_exec);

/* HIP-event timing on the context's stream (bench.py: whole region and per-kernel durations) */
int sdx_timer_start(sdx_ctx* ctx);
int sdx_timer_stop(sdx_ctx* ctx, double* elapsed_ms);
int sdx_profile_enable(sdx_ctx* ctx, int on); /* bracket every kernel launch with events */
int sdx_profile_reset(sdx_ctx* ctx);
int sdx_profile_get(sdx_ctx* ctx, const char* kernel, int64_t* launches, double* total_ms);
/* which device kernel last ran under the stage name `kernel` while profiling was on ("k_raytrace" -> "k_raytrace_seg<8,7>", "k_raytrace_seg_step<8,7>",
 * "k_raytrace<1>", "k_raytrace_f32", ...); "" when the stage has one kernel only or did not run */
int sdx_profile_variant(sdx_ctx* ctx, const char* kernel, char* out, int out_len);

/* ---- line opacity ---------------------------------------------------------------------------
 * Replaces calc_alan_entries (radiation_field/opacities/opacities_solvers/base.py:487-592):
 *   out[d, i] (+)= sum_l [lo_ld <= i < hi_ld] alpha_ld * voigt(nu_i - nu_l; doppler_ld, gamma_ld)
 * with the reference's window rule (:556-575) evaluated on the GLOBAL grid `nus` (n_nu, descending).
 * Only columns nu_begin .. nu_begin+nu_count-1 are produced (frequency sharding); out is
 * [n_depth][out_ld] with column 0 = global index nu_begin.  line_nus ascending; doppler/alphas are
 * [n_lines][n_depth]; gammas is [n_lines][gamma_cols], gamma_cols = n_depth or 1 (:547-551).
 * accumulate = 0 overwrites out, 1 adds to it.  n_evaluations_dev (optional, device int64)
 * receives sum(hi - lo) over all (line, depth), i.e. the number of Voigt evaluations of the full grid (0 for an empty list; a call
 * with nu_count = 0 returns at once and leaves it untouched — sdx_synthesize_sharded_f64 asks its first NON-empty rank). */
int sdx_line_opacity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin,
                         int64_t nu_count, int64_t n_lines, const double* line_nus, const double* doppler_widths,
                         const double* gammas, int gamma_cols, const double* alphas, double* out, int64_t out_ld,
                         int accumulate, int64_t* n_evaluations_dev);
/* host-buffer twin: the whole grid, out [n_depth][n_nu] overwritten.  n_nu = 0 returns after the argument checks, copies nothing and
 * stores 0 in *n_evaluations (optional). */
int sdx_line_opacity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines,
                         const double* line_nus, const double* doppler_widths, const double* gammas, int gamma_cols,
                         const double* alphas, double* out, int64_t* n_evaluations);
/* window rule only (:556-575): lower/upper are [n_lines][n_depth] int32, on device */
int sdx_line_windows_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines,
                         const double* line_nus, const double* doppler_widths, const double* gammas, int gamma_cols,
                         const double* alphas, int32_t* lower, int32_t* upper);

/* voigt.py:89-91 faddeeva (z, w interleaved re/im) and voigt.py:153-155 voigt_profile, element-wise */
int sdx_faddeeva_dev(sdx_ctx* ctx, int64_t n, const double* z, double* w);
int sdx_voigt_profile_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* doppler_width,
                          const double* gamma, double* phi);
/* The hot-path variant of the same function, element-wise: what the line kernels evaluate per (line, depth, frequency)
 * from the pre-pass constants — out = amp * Re w(delta_nu * inv_doppler_width + i y), real part only, FMA arithmetic
 * (voigt.py:17-86 regions and predicates; base.py:627 amplitude).  A test hook: it lets the kernel's own routine be
 * compared point by point with the reference's Faddeeva / Voigt vectors. */
int sdx_voigt_term_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y,
                       const double* amp, double* out);
/* The fp32 routine the narrow windows are evaluated with when the option mixed_precision is on (all four regions in packed
 * fp32, hardware exp / cos); same arguments, rounded to fp32 inside.  Test hook for the stated 1e-4 tolerance of that mode. */
int sdx_voigt_term_f32_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y,
                           const double* amp, double* out);
/* The term and its two partial derivatives, element-wise — the routine sdx_line_param_adjoint_dev evaluates per (line, depth,
 * frequency): with x = delta_nu * inv_doppler_width and K = Re w(x + i y)
 *     out_k = amp K,   out_kx = amp dK/dx,   out_ky = amp dK/dy.
 * What is differentiated is the reference's formula in the Humlicek region it picks (voigt.py:39-84; y and amp as voigt.py:148-149
 * form them), chosen by sdx_voigt_term_dev's own predicates on the same rounded x and y, the region boundaries held fixed: dK/dx =
 * Re w'(z), dK/dy = -Im w'(z) of that region's rational (region IV: of exp(-z^2) minus its rational), not of the true Faddeeva
 * function.  A test hook, like sdx_voigt_term_dev: it lets the routine be judged point by point. */
int sdx_voigt_grad_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y,
                       const double* amp, double* out_k, double* out_kx, double* out_ky);

/* ---- broadening (opacities_solvers/broadening.py) -------------------------------------------
 * calc_gamma :550-656 with calculate_broadening's argument preparation :706-721 (ion_number is the
 * reference's ion_number + 1); per-line inputs [n_lines], per-depth inputs [n_depth], out [n_lines][n_depth]. */
int sdx_calc_gamma_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const int32_t* atomic_number,
                       const int32_t* ion_number, const double* ionization_energy, const double* upper_level_energy,
                       const double* lower_level_energy, const double* A_ul, const double* electron_density,
                       const double* temperature, const double* h_density, int flags, double* gammas);
/* calc_doppler_width :32-71 broadcast as at :723-730 / :814-819 */
int sdx_doppler_widths_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const double* line_nus, const double* mass,
                           const double* temperature, double microturbulence, double* doppler_widths);
/* calc_vald_gamma :1009-1085 (stark :880-890, van der Waals :893-1006).  flags: 1 linear Stark (hydrogen lines), 2 VALD Stark,
 * 4 van der Waals, 8 radiation; + 16 = the sum is NOT halved: the VALD branch of calculate_molecule_broadening (:771-799), which adds
 * A_ul, calc_vald_stark_gamma when linear OR quadratic Stark is configured (pass 2, never 1) and calc_vald_vdW and skips :1084. */
int sdx_calc_vald_gamma_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const int32_t* atomic_number,
                            const int32_t* ion_number, const double* ionization_energy,
                            const double* upper_level_energy, const double* lower_level_energy, const double* A_ul,
                            const double* stark, const double* waals, const double* mass,
                            const double* electron_density, const double* temperature, const double* h_density,
                            int flags, double* gammas);

/* The reference's element-wise ufuncs, all operands already broadcast to length n (integers passed as doubles):
 *   op 0 calc_doppler_width(nu_line, temperature, atomic_mass, microturbulence)                    :69-71
 *   op 1 calc_n_effective(ion_number, ionization_energy, level_energy)                            :140-146
 *   op 2 calc_gamma_linear_stark(n_eff_upper, n_eff_lower, electron_density)                      :232-234
 *   op 3 calc_gamma_quadratic_stark(ion_number, n_eff_upper, n_eff_lower, electron_density, T)    :346-360
 *   op 4 calc_gamma_van_der_waals(ion_number, n_eff_upper, n_eff_lower, T, h_density)             :476-490 */
int sdx_broadening_scalar_dev(sdx_ctx* ctx, int op, int64_t n, const double* a, const double* b, const double* c,
                              const double* d, const double* e, double* out);

/* ---- continuum (opacities_solvers/base.py:40-317); every out is [n_depth][ld], columns nu_begin.. -- */
/* calc_alpha_file :40-70 with a 1-D table (util.py:94-103, np.interp): out = sigma(lambda_i) * density[d] */
int sdx_alpha_file_1d_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* lambdas, int n_table,
                          const double* table_wavelength, const double* table_sigma, const double* density,
                          double* out, int64_t ld);
/* calc_alpha_file :70 with sigma already tabulated per (depth, nu) (util.py:35-91 host interpolation) */
int sdx_alpha_file_2d_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* sigma, int64_t sigma_ld,
                          const double* density, double* out, int64_t ld);
/* sigma_file for the two 2-D tables (opacities_solvers/util.py:35-91): scipy's
 * LinearNDInterpolator(points, values, fill_value=0) on the Delaunay triangulation of the rectilinear table, evaluated at
 * the mesh (lambdas[k], second[d]) with second = T (H2+ bf) or 5040/T (H- ff).  The caller passes the triangulation its
 * scipy/Qhull built, indexed by grid cell: cell_simplices[(i*(n_y-1)+j)*2 + {0,1}] are the two triangles of cell (i, j),
 * transform[s] is Qhull's 3x2 barycentric transform of triangle s (scipy.spatial.Delaunay.transform),
 * simplex_values[s][v] the table value at its v-th vertex.  scale_kind 0: raw; 1: x 1e-18 (util.py:58);
 * 2: x 1e-26 x k_B x T[d] (util.py:83-88).  zero_rows (optional, [n_depth]) is set to 1 for rows that contain an exact
 * zero — the rows the reference names in its "outside of interpolation range" warning.  sigma is [n_depth][ld]. */
int sdx_sigma_table_2d_dev(sdx_ctx* ctx, int n_x, const double* x_axis, int n_y, const double* y_axis,
                           const int32_t* cell_simplices, const double* transform, const double* simplex_values,
                           int n_depth, int64_t n_nu, const double* lambdas, const double* second, int scale_kind,
                           const double* temperature, double* sigma, int64_t ld, int32_t* zero_rows);
/* calc_alpha_bf :178-271: levels grouped by species; cutoff[L] = (E_ion - E_exc)/h; level_density [n_levels][n_depth] */
int sdx_alpha_bf_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int n_species,
                     const int32_t* species_offsets, const int32_t* species_ion_number, const double* cutoff,
                     const double* level_density, double* out, int64_t ld);
/* calc_alpha_ff :274-317: number_density [n_species][n_depth] = n_ion * n_e, ion_number as get_number_density returns */
int sdx_alpha_ff_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, const double* temperature,
                     int n_species, const int32_t* species_ion_number, const double* number_density, double* out,
                     int64_t ld);
/* calc_alpha_rayleigh :74-135; NULL density = species not requested.  `nus` is modified in place
 * (nu > 2.3e15 -> 0) exactly as the reference does at :99. */
int sdx_alpha_rayleigh_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* nus, const double* n_h,
                           const double* n_he, const double* n_h2, double* out, int64_t ld);
/* calc_alpha_electron :139-174 */
int sdx_alpha_electron_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* electron_density, double* out,
                           int64_t ld);
/* Opacities.calc_total_alphas (radiation_field/opacities/base.py:24-28): total += src */
int sdx_accumulate_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* total, int64_t total_ld, const double* src,
                       int64_t src_ld);

/* ---- formal solution (radiation_field/radiation_field_solvers/base.py) ---------------------- */
/* blackbody_flux_at_nu (source_functions/blackbody.py:10-35) */
int sdx_blackbody_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, const double* temperature,
                      double* out, int64_t ld);
/* calc_weights_parallel :6-47 */
int sdx_calc_weights_dev(sdx_ctx* ctx, int64_t n, const double* delta_tau, double* w0, double* w1, double* w2);
/* raytrace :271-346, plane-parallel branch.  ray_dist is [n_depth-1][n_theta] = dist[:,None]/cos(thetas)
 * (:302-305).  nus/total_alphas/F_nu hold the n_nu columns being traced (a shard passes its own
 * slice).  accumulate = 1: F_nu is ACCUMULATED into, the reference's behaviour (:336); 0: F_nu is overwritten
 * (row 0 becomes 0).  I_nus [n_depth][n_nu][n_theta] optional (:333-334). */
int sdx_raytrace_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                     const double* temperature, const double* ray_dist, const double* theta_weights,
                     const double* total_alphas, int64_t alpha_ld, double* F_nu, int64_t F_ld, double* I_nus,
                     int accumulate);
/* raytrace :271-346, spherical branch: ray_dist from calculate_spherical_ray (:349-381, zeros where a ray misses a
 * shell), the inward sweep of single_theta_trace_parallel (:141-198) before the outward one, and finally
 * F_nu *= photospheric_correction = (r[-1] / reference_r)**2 (:340-344). */
int sdx_raytrace_spherical_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                               const double* temperature, const double* ray_dist, const double* theta_weights,
                               const double* total_alphas, int64_t alpha_ld, double* F_nu, int64_t F_ld, double* I_nus,
                               int accumulate, double photospheric_correction);
/* raytrace with the source function handed over as a plane [n_depth][source_ld] instead of the Planck function the other
 * entry points evaluate in the kernel: RadiationField.source_function is any callable (nu, T[:, None]) -> (N_d, N_nu)
 * (radiation_field/base.py:12-68, used at radiation_field_solvers/base.py:133); the host evaluates a foreign one and uploads
 * the result.  source = NULL: Planck.  inward != 0: spherical geometry (as sdx_raytrace_spherical_dev, with the correction). */
int sdx_raytrace_source_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                            const double* temperature, const double* ray_dist, const double* theta_weights,
                            const double* total_alphas, int64_t alpha_ld, const double* source, int64_t source_ld,
                            double* F_nu, int64_t F_ld, double* I_nus, int accumulate, int inward,
                            double photospheric_correction);
int sdx_raytrace_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                     const double* temperature, const double* ray_dist, const double* theta_weights,
                     const double* total_alphas, double* F_nu, double* I_nus);

/* ---- flux contribution function and formation depth ------------------------------------------
 * WHERE the emergent flux is formed.  The reference has no such output; it follows from its formal solution without a new
 * model: per ray and gap the step of single_theta_trace_parallel (radiation_field_solvers/base.py:200-266) is the affine map
 * I[g+1] = c[g] I[g] + e[g], every ray starts at I[0] = 0 (:134), so the emergent intensity is exactly sum_g T[g+1] e[g] with
 * T[N_d-1] = 1, T[k] = T[k+1] c[k] the transmission from row k to the surface.  With tau[g] = mean_alpha[g] ray_dist[g] (:121-129),
 * (c, e) the step of the formal-solution kernels themselves (the tau == 0 -> (1, 0) rule of :203-206 and :253-254 included; the
 * last gap by :253-266) and the flux weights of :324-338:
 *     C[0][nu] = 0,   C[k][nu] = sum_theta w_theta (T[k] e[k-1])       what the layer below row k adds to F_nu[N_d-1][nu]
 * (theta in two ascending halves, the lower added to the upper, as F_nu is summed), hence sum_k C[k] = F_nu[N_d-1] up to rounding.
 * C may be negative in a layer where the second-order scheme overshoots; it is reported as it is.
 * nus / total_alphas / C hold the n_nu columns being traced (a shard passes its own slice), as for sdx_raytrace_dev; ray_dist
 * [n_depth-1][n_theta]; source = NULL: Planck, else a plane [n_depth][source_ld] as for sdx_raytrace_source_dev; C [n_depth][C_ld].
 * Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0, so a caller can ask at set-up time): a context with
 * mixed_precision = 1, n_theta > 64, a model whose columns do not fit 64 KB of LDS at one frequency per wave.  Plane-parallel
 * geometry only: the inward sweep of the spherical branch (:141-198) makes I[0] != 0, and there is no argument to ask for it. */
int sdx_contribution_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                         const double* temperature, const double* ray_dist, const double* theta_weights,
                         const double* total_alphas, int64_t alpha_ld, const double* source, int64_t source_ld,
                         double* C, int64_t C_ld);
/* Formation mean of a per-depth quantity x[n_depth] the caller chooses (geometric depth, temperature, a reference log tau), weighted
 * by the contribution function above (a decomposition of the flux sum of :324-338):
 *     out[nu] = (sum_{k>=1} C[k][nu] m_k) / (sum_{k>=1} C[k][nu]),   m_k = (x[k-1] + x[k]) 0.5
 * both sums over ascending k, every operation one correctly rounded fp64 operation; a zero denominator gives what IEEE gives (NaN). */
int sdx_formation_mean_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* C, int64_t C_ld, const double* x,
                           double* out);
/* host-buffer twin of sdx_contribution_dev (decomposes raytrace :271-346 as above): contiguous arrays, total_alphas / source / C
 * [n_depth][n_nu]; source = NULL: Planck. */
int sdx_contribution_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                         const double* temperature, const double* ray_dist, const double* theta_weights,
                         const double* total_alphas, const double* source, double* C);

/* ---- emergent intensity of every ray: the surface row alone ------------------------------------
 * I(theta, nu) at the surface, without the [n_depth][n_nu][n_theta] volume that I_nus costs: the walk of the plain formal-solution kernel
 * (k_raytrace: columns of (S, sqrt(alpha)) staged per wave from a FINISHED total_alphas plane, the inward sweep of :141-198 first where
 * inward != 0, the step of :200-266 per gap through the same device functions on the same operands in the same order) that keeps what a
 * ray holds after the last gap.  I_out[theta][nu] is therefore row n_depth-1 of I_nus as sdx_raytrace_source_dev returns it from that
 * kernel on the same inputs, bit for bit.  These are INTENSITIES: no theta weights and no photospheric correction are applied (the flux
 * is sum_theta w_theta I_out[theta], in two ascending halves, times the correction of a spherical model).
 * I_out is theta-major, [n_theta][I_ld] with I_ld >= n_nu: one angle's spectrum is contiguous, which is what sdx_disk_integrate_dev
 * reads.  nus / total_alphas / source hold the n_nu columns being traced, as for sdx_contribution_dev; ray_dist [n_depth-1][n_theta];
 * source = NULL: Planck, else a plane [n_depth][source_ld].
 * Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0, so a caller can ask at set-up time): a context with
 * mixed_precision = 1, n_theta > 64, a model whose columns do not fit 64 KB of LDS at one frequency per wave, I_out that is one of the
 * inputs.  Device pointers, asynchronous, no allocation, capturable.  Stage name: "k_emergent_intensity". */
int sdx_emergent_intensity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                               const double* temperature, const double* ray_dist, const double* total_alphas, int64_t alpha_ld,
                               const double* source, int64_t source_ld, int inward, double* I_out, int64_t I_ld);
/* host-buffer twin: contiguous arrays, total_alphas / source [n_depth][n_nu], I_out [n_theta][n_nu]; source = NULL: Planck. */
int sdx_emergent_intensity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                               const double* temperature, const double* ray_dist, const double* total_alphas,
                               const double* source, int inward, double* I_out);

/* ---- response functions: flux derivatives to opacity and source per depth ------------------------
 * HOW the emergent flux changes: the exact derivative of the formal solution above, the companion of the contribution function.
 * It is the derivative of the reference's formulas as written, branch by branch (radiation_field_solvers/base.py:22-45, :200-266).
 * Per ray t[g] = sqrt(alpha[g]) sqrt(alpha[g+1]) ray_dist[g], I[g+1] = c[g] I[g] + e[g], I[0] = 0, T[N_d-1] = 1, T[k] = T[k+1] c[k].
 * Derivatives of the weights, (p0, p1, p2) = d(w0, w1, w2)/dt:  t < 5e-4: (1 - t, t - t^2, t^2 - t^3);  t < 50: (E, t E, t^2 E),
 * E = exp(-t);  otherwise 0.
 * Inner gap g < N_d-2, t0 = t[g], t1 = t[g+1], s = t0 + t1, d10 = S[g] - S[g+1], d21 = S[g+2] - S[g+1],
 * A = d10 t1/t0 - d21 t0/t1, B = d10/t0 + d21/t1:
 *     e      = w0 S[g+1] + (w1 A + w2 B)/s
 *     de/dt0 = p0 S[g+1] + (p1 A + p2 B)/s + w1 [(-d21/t1 - d10 t1/t0^2)/s - A/s^2] + w2 [(-d10/t0^2)/s - B/s^2]
 *     de/dt1 = w1 [(d10/t0 + d21 t0/t1^2)/s - A/s^2] + w2 [(-d21/t1^2)/s - B/s^2]
 *     e = a S[g] + q S[g+1] + r S[g+2]:   a = (w1 t1/t0 + w2/t0)/s,   r = (-w1 t0/t1 + w2/t1)/s,   q = w0 - a - r
 * Last gap:  e = w0 S1 + w2 d10/t0^2,   de/dt0 = p0 S1 + p2 d10/t0^2 - 2 w2 d10/t0^3,   a = w2/t0^2,  q = w0 - a,  r = 0.
 * A gap with t0 == 0 is the (1, 0) step (:203-206, :253-254): its derivatives and its three coefficients are 0 — so a row with
 * alpha = 0 contributes 0 through t = 0.
 * With G[j] = dI_emergent/dt[j] = T[j+1] (-p0[j] I[j] + de[j]/dt0) + T[j] de[j-1]/dt1 (the last term absent for j = 0):
 *     R_alpha[k][nu]  = sum_theta w_theta (t[k-1] G[k-1] + t[k] G[k]) / 2                    = dF_nu[N_d-1] / d ln alpha[k]
 *     R_source[k][nu] = sum_theta w_theta (T[k+1] a[k] + T[k] q[k-1] + T[k-1] r[k-2])        = dF_nu[N_d-1] / dS[k]
 * (terms that do not exist are dropped; theta in two ascending halves, the lower added to the upper, as F_nu is summed).
 * sum_k R_source[k] S[k] = F_nu[N_d-1] up to rounding, since I is linear in S.  T[j+1] I[j] is formed from a forward and a backward
 * walk, not from differences of the emergent intensity: deep layers keep their (tiny) response instead of a cancelled one.
 * Range: the derivative divides by t0^3 and s^2 and so leaves the normal numbers earlier than the flux does — optical depths at the
 * ends of the double range (about 1e-100 and 1e100) are outside the contract; where the reference's own formulas divide by zero
 * (a transparent row above an opaque one) the rows concerned are inf / NaN as the formulas give them.
 * Arguments as for sdx_contribution_dev; R_alpha [n_depth][R_alpha_ld], R_source [n_depth][R_source_ld]; either may be NULL (not
 * formed), not both.  Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0, so a caller can ask at set-up time):
 * mixed_precision = 1, n_theta > 64, a model whose columns and stashed intensities — ((n_theta + 2) n_depth + 7 n_theta) doubles at
 * one frequency per wave — do not fit 64 KB of LDS (117 depth points at 64 angles, 366 at 20).  Plane-parallel geometry only. */
int sdx_response_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                     const double* temperature, const double* ray_dist, const double* theta_weights,
                     const double* total_alphas, int64_t alpha_ld, const double* source, int64_t source_ld,
                     double* R_alpha, int64_t R_alpha_ld, double* R_source, int64_t R_source_ld);
/* host-buffer twin of sdx_response_dev: contiguous arrays, total_alphas / source / R_alpha / R_source [n_depth][n_nu]; source = NULL:
 * Planck; R_alpha or R_source may be NULL. */
int sdx_response_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                     const double* temperature, const double* ray_dist, const double* theta_weights,
                     const double* total_alphas, const double* source, double* R_alpha, double* R_source);
/* The response for a cotangent per (angle, frequency): what carries a weight on sdx_emergent_intensity_dev's rows — the transpose of
 * sdx_disk_integrate_dev, say — back to the opacity and the source function.  The arguments are sdx_response_dev's with the plane
 * cotangent[n_theta][cot_ld] (cot_ld >= n_nu) in place of theta_weights:
 *     R_alpha[k][nu]  = sum_theta cot[theta][nu] (t[k-1] G[k-1] + t[k] G[k]) / 2  = d(sum_theta cot[theta][nu] I_theta(nu)) / d ln alpha[k][nu]
 *     R_source[k][nu] = sum_theta cot[theta][nu] (T[k+1] a[k] + T[k] q[k-1] + T[k-1] r[k-2])
 * The kernel is k_response with a compile-time flag: the same device functions, two walks, LDS layout and theta sum (the flux's order),
 * a ray's terms times cot[theta][nu] where the flux weight w_theta stands otherwise.  cot[theta][nu] = w_theta for every nu therefore
 * reproduces sdx_response_dev bit for bit, and n_theta calls of sdx_response_dev with one-hot weights hold the same products.
 * Plane-parallel geometry only; sdx_response_dev's refusals, and cot_ld < n_nu or an output that is the cotangent.  Device pointers,
 * asynchronous, no allocation, capturable.  Stage name: "k_response_angles". */
int sdx_response_angles_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                            const double* temperature, const double* ray_dist, const double* cotangent, int64_t cot_ld,
                            const double* total_alphas, int64_t alpha_ld, const double* source, int64_t source_ld,
                            double* R_alpha, int64_t R_alpha_ld, double* R_source, int64_t R_source_ld);
/* host-buffer twin: contiguous arrays, cotangent [n_theta][n_nu], the planes [n_depth][n_nu]. */
int sdx_response_angles_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                            const double* temperature, const double* ray_dist, const double* cotangent,
                            const double* total_alphas, const double* source, double* R_alpha, double* R_source);
/* The response to a scale factor on one part of the opacity (the line opacity of one species, say: dF/d ln epsilon at fixed
 * ionisation and continuum):
 *     out[nu] = sum_k R_alpha[k][nu] (part[k][nu] / total[k][nu])
 * over ascending k, every operation one correctly rounded fp64 operation; a zero in total gives what IEEE gives. */
int sdx_response_project_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* R_alpha, int64_t R_ld, const double* part,
                             int64_t part_ld, const double* total, int64_t total_ld, double* out);

/* ---- continuum scattering: mean intensity and the scattering source function -----------------------
 * Every formal solution above takes the LTE source function S = B and treats Thomson and Rayleigh opacity — part of total_alphas,
 * ((((file + bf) + ff) + rayleigh) + electron) + line — as true absorption, as the reference does.  These two entry points produce
 * what the source-plane arguments of sdx_raytrace_source_dev, sdx_contribution_dev and sdx_response_dev consume instead: the mean
 * intensity J of the project's own formal solution at every depth point, over both hemispheres, and the solution of
 *     S = (1 - albedo) B + albedo J[S],   albedo = alpha_scatter / alpha_total
 * for coherent, isotropic scattering (every frequency its own linear problem).  The reference has no counterpart.
 * Plane-parallel, fp64, n_theta <= 64.  Per frequency and angle k the optical depth of gap g is the kernels' own,
 * tau_k[g] = (sqrt(alpha[g]) sqrt(alpha[g+1])) ray_dist[g][k].  For a source column S of N_d values (row 0 deepest):
 *   upward sweep    exactly the outward recurrence of the flux kernels: U_k[g+1] = c U_k[g] + e with (c, e) of the inner gaps from
 *                   (tau[g], tau[g+1], S[g] - S[g+1], S[g+2] - S[g+1], S[g+1]) and of the last gap from its own form (:253-266), the
 *                   tau == 0 -> (1, 0) rule and the rare-lane fallback included — but started from U_k[0] = S[0], a THERMALISED lower
 *                   boundary (the reference's I[0] = 0, which stays what the flux kernels use, would halve J at the bottom);
 *   downward sweep  the same recurrence on the depth-reversed column, started from D_k[N_d-1] = 0: arrival at point g >= 1 takes the
 *                   inner form with (tau[g], tau[g-1], S[g+1] - S[g], S[g-1] - S[g], S[g]), arrival at point 0 the last-gap form with
 *                   (tau[0], 0, S[1] - S[0], 0, S[0]); no negative-index wrap as in the spherical inward sweep;
 *   mean intensity  J[d] = (sum_k m_k U_k[d]) + (sum_k m_k D_k[d]), each sum over k as the flux is summed (two ascending halves, the
 *                   lower added to the upper); the downward sum of row N_d-1 is a sum of zeros;
 *   diagonal        L[d] = (sum_k m_k qU_k[d]) + (sum_k m_k qD_k[d]), q the coefficient of the arrival point's source value in the
 *                   step's e (q of sdx_response_dev above; 0 for a gap with tau == 0), qU_k[0] = 1, qD_k[N_d-1] = 0.  It depends on
 *                   the optical depths alone;
 *   mean weights    m [n_theta] is an argument, with sum_k 2 m_k = 1 so that an isotropic field gives J = I (otherwise the iteration
 *                   creates or destroys photons).  For Gauss-Legendre nodes in theta with the field's weights w:
 *                   m_k = w_k sin(theta_k) / (2 sum_j w_j sin(theta_j)).
 * sdx_mean_intensity_dev is one application: J and / or lambda_diag [n_depth][ld] (either may be NULL, not both) of the source plane
 * (NULL: Planck, as the flux kernels stage it).
 * sdx_scatter_source_dev iterates.  albedo[d] = alpha_scatter[d] / total_alphas[d] clamped to [0, 1] (NaN -> 0), 0 where
 * total_alphas == 0; alpha_scatter [n_depth][scatter_ld], or with scatter_ld == 0 one value per depth point [n_depth] (Thomson).
 * The thermal term is (1 - albedo) B, B the plane `thermal` or (NULL) Planck.  Jacobi iteration with a local operator:
 *     S^0 = B,   S^(n+1) = S^n + ((1 - albedo) B + albedo J[S^n] - S^n) / (1 - albedo Lc),   Lc = clamp(L, 0, 1) (NaN -> 0)
 * (the clamp changes the rate, never the fixed point; L is formed once).  Every point of a column is updated from the J of the
 * finished sweeps: no point sees a neighbour's new value within an iteration.  A column stops
 *   status 0   when max_d |S^(n+1)[d] - S^n[d]| <= tol max_d |S^(n+1)[d]|;
 *   status 1   after max_iter iterations;
 *   status 2   when the change is not finite; the update is then not applied — S is the last finite iterate — and `change` is +inf.
 * `iterations` counts the updates evaluated (the refused one of status 2 included), `change` is the last max_d |S^(n+1) - S^n|.
 * A column that has stopped is never written again while the others of its launch finish: its bits do not depend on the grid, the
 * shard or the other columns.  max_iter bounds the kernel's loop.  J, when asked for, is the mean intensity OF THE RETURNED S (one more
 * application).  No atomics anywhere: the same bits from run to run.
 * The step is second order and NOT a positive operator.  On grids as fine as stellar model atmospheres (57 points over 7 decades of
 * tau) L lies in (0, 1) and the iteration converges (albedo 0.5 / 0.9 / 0.99 / 0.999: 23 / 77 / 242 / 516 iterations at tol = 1e-12);
 * on coarse grids L leaves [0, 1] (seen: -0.59 and 1.71 at 3 points over 7 decades), and for albedo >= 0.9 the discrete problem
 * itself has no positive solution: the iteration diverges, which is what status 1 and 2 report.  DESIGN.md, "Scattering in the source function".
 * Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0): mixed_precision = 1, n_theta > 64, tol < 0 or NaN,
 * max_iter < 1, a model whose columns — (6 n_depth + 4 n_theta) doubles at one frequency per wave — do not fit 64 KB of LDS (1352
 * depth points at 20 angles).  Out of scope: spherical geometry, line scattering.  Derivatives of the scattering solution:
 * sdx_scatter_response_dev below. */
int sdx_mean_intensity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                           const double* temperature, const double* ray_dist, const double* mean_weights,
                           const double* total_alphas, int64_t alpha_ld, const double* source, int64_t source_ld,
                           double* J, int64_t J_ld, double* lambda_diag, int64_t L_ld);
int sdx_scatter_source_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                           const double* temperature, const double* ray_dist, const double* mean_weights,
                           const double* total_alphas, int64_t alpha_ld, const double* alpha_scatter, int64_t scatter_ld,
                           const double* thermal, int64_t thermal_ld, double tol, int max_iter, double* S, int64_t S_ld,
                           double* J, int64_t J_ld, int* iterations, int* status, double* change);
/* host-buffer twins: contiguous arrays, planes [n_depth][n_nu]; source / thermal = NULL: Planck; outputs that may be NULL as above.
 * scatter_per_frequency != 0: alpha_scatter [n_depth][n_nu], else [n_depth]. */
int sdx_mean_intensity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                           const double* temperature, const double* ray_dist, const double* mean_weights,
                           const double* total_alphas, const double* source, double* J, double* lambda_diag);
int sdx_scatter_source_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                           const double* temperature, const double* ray_dist, const double* mean_weights,
                           const double* total_alphas, const double* alpha_scatter, int scatter_per_frequency,
                           const double* thermal, double tol, int max_iter, double* S, double* J, int* iterations,
                           int* status, double* change);

/* ---- continuum scattering: Ng acceleration of the source iteration ----------------------------------
 * sdx_scatter_source_ng_dev is sdx_scatter_source_dev's iteration with the unweighted second-order Ng extrapolation (Olson, Auer &
 * Buchler 1986) and a safeguard, per column.  Arguments, outputs and refusals are the sibling's; `accelerations` [n_nu] (may be
 * NULL) receives the extrapolations applied.  The bits differ from the plain solve's: it is a different sequence to the same fixed
 * point, stopped by the same rule.
 *   update          exactly the plain one: same residual, same local operator 1 / (1 - albedo Lc), same order of operations.  The
 *                   stopping rule is evaluated on updates only, never on an extrapolation's jump, and is otherwise unchanged: statuses
 *                   0 / 1 / 2, the refused non-finite update, the frozen column, `iterations` (updates evaluated) and `change` keep
 *                   their meaning, and status 0 always follows a plain update.
 *   history         the last four iterates SINCE THE LAST EXTRAPOLATION, x0 the newest .. x3; S^0 and an extrapolated iterate count.
 *   extrapolation   after update n, where the column is live and still accelerated, ng_start <= n < max_iter (what is returned has
 *                   always been through an update), at least ng_period updates have passed since the last extrapolation and the
 *                   history holds four iterates:
 *                       q1 = (x0 - 2 x1) + x2,   q2 = ((x0 - x1) - x2) + x3,   q3 = x0 - x1
 *                       A1 = sum_d q1 q1, B1 = sum_d q1 q2, C1 = sum_d q1 q3, B2 = sum_d q2 q2, C2 = sum_d q2 q3
 *                       det = A1 B2 - B1 B1,   a = (C1 B2 - C2 B1) / det,   b = (C2 A1 - C1 B1) / det
 *                       S <- (((1 - a) - b) x0 + a x1) + b x2
 *                   every operation one rounded fp64 operation.  The sums are unweighted: lane g of the column's n_theta lanes adds
 *                   its depths g, g + n_theta, ... in ascending order from 0, then the n_theta partials are added in ascending lane
 *                   order from 0 — the order is fixed by (n_depth, n_theta) alone.
 *   skipped         if any component of the extrapolated column is not finite (det == 0 included) the extrapolation is skipped: the
 *                   iterate stays x0, nothing is counted, the history continues.
 *   safeguard       an extrapolation remembers `reference`, the change of the update before it, and keeps a copy of the iterate it
 *                   replaced.  ng_period updates later — at the update before the next extrapolation would be due — the change is
 *                   compared with the reference.  Smaller: a gain; the next extrapolation takes a new reference and a new copy.
 *                   Not smaller: a strike; the next extrapolation goes ahead but keeps reference and copy.  Two strikes in a row:
 *                   the column takes the copy back (the iterate before the first of the two extrapolations), continues plain for
 *                   good, and `accelerations` stops counting.  It costs no operator application and reads the column's own
 *                   numbers alone, so a column's bits depend on nothing that shares its wave, launch or shard.
 * Defaults of the Python layers: ng_start = 4, ng_period = 4.  One strike alone is too quick for this iteration (after a good
 * extrapolation the max-norm change often rises by a few percent for one period while the error has halved), none at all is the
 * bare method.  DESIGN.md, "Scattering in the source function", has the rule's evidence and the variants that failed.
 * The adjoint solve (sdx_scatter_response_dev) has NO accelerated sibling: no safeguard tried keeps it within the plain iteration's
 * cost on every column ("The scattering adjoint").
 * Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0): what sdx_scatter_source_dev refuses, ng_start < 4,
 * ng_period < 1, and a model whose columns — (10 n_depth + 5 n_theta) doubles at one frequency per wave: the iteration's and four
 * columns of history — do not fit 64 KB of LDS (809 depth points at 20 angles; sdx_scatter_source_dev, the plain iteration, serves
 * 1352). */
int sdx_scatter_source_ng_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                              const double* temperature, const double* ray_dist, const double* mean_weights,
                              const double* total_alphas, int64_t alpha_ld, const double* alpha_scatter, int64_t scatter_ld,
                              const double* thermal, int64_t thermal_ld, double tol, int max_iter, double* S, int64_t S_ld,
                              double* J, int64_t J_ld, int* iterations, int* status, double* change, int ng_start,
                              int ng_period, int* accelerations);
int sdx_scatter_source_ng_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                              const double* temperature, const double* ray_dist, const double* mean_weights,
                              const double* total_alphas, const double* alpha_scatter, int scatter_per_frequency,
                              const double* thermal, double tol, int max_iter, double* S, double* J, int* iterations,
                              int* status, double* change, int ng_start, int ng_period, int* accelerations);

/* ---- continuum scattering: the adjoint solve and the flux responses --------------------------------
 * The derivative of a functional of the scattering solution is the adjoint of a fixed point: one transposed solve per column with
 * the operator of sdx_mean_intensity_dev, not a derivative through the iterations.  Notation as there: Lambda is the linear map
 * S -> J of one column (upward sweep from U[0] = S[0], downward sweep from 0, mean weights m), W = diag(albedo).  Both sweeps are
 * chains of the kernels' own step, val[s+1] = c[s] val[s] + e[s], e[s] = a[s] S[behind] + q[s] S[arrival] + r[s] S[ahead] — behind,
 * arrival, ahead are the rows (s, s+1, s+2) of the upward sweep and (N_d-1-s, N_d-2-s, N_d-3-s) of the downward one; the last step of
 * a sweep has r = 0 and the last-gap a and q.  (c, a, q, r, p0 = -dc/dt0, de/dt0, de/dt1) are those of sdx_response_dev above, with
 * t0 the optical depth of the step's own gap and t1 that of the sweep's next gap.
 * Transposed application.  Given a plane z, for each sweep and angle theta walk against the sweep with
 *     vbar[last] = m_theta z[p_last],   vbar[s] = m_theta z[p_s] + c[s] vbar[s+1]        (p_s: the row the sweep reaches after s steps)
 * and accumulate
 *     (Lambda^T z)[behind_s] += a[s] vbar[s+1],  (Lambda^T z)[arrival_s] += q[s] vbar[s+1],  (Lambda^T z)[ahead_s] += r[s] vbar[s+1],
 * and in the upward sweep (Lambda^T z)[0] += vbar[0].  A gap with tau == 0 is the (1, 0) step: c = 1, a = q = r = 0.  Per ray a row
 * collects (a[j] vbar[j+1] + q[j-1] vbar[j]) + r[j-2] vbar[j-1]; the sum over theta runs in the flux's order (two ascending halves,
 * the lower added to the upper), the downward sweep's sum is added to the upward one's.  The kernel takes (c, a, q, r) of this walk
 * from the forward step itself (the step is linear in the three source values): sum z J[x] = sum (Lambda^T z) x holds between the
 * two entry points to rounding, also where the step's own rounding near tau = 5e-4 is far above that.
 * Opacity derivative of one application, at fixed S.  With val[s] of the forward sweep, the gap of step s collects
 *     tbar[gap t0_s] += vbar[s+1] (de/dt0[s] - p0[s] val[s]),     tbar[gap t1_s] += vbar[s+1] de/dt1[s]
 * and  G[k] = d(z^T J[S]) / d ln alpha[k] = sum_theta (t[k-1] tbar[k-1] + t[k] tbar[k]) / 2  (terms that do not exist are dropped: the
 * shape of R_alpha), per sweep, the downward sweep's sum added to the upward one's.
 * sdx_mean_intensity_adjoint_dev is one application: Lt = Lambda^T z and / or G [n_depth][ld] (either may be NULL, not both) for the
 * planes z [n_depth][z_ld] and source (NULL: Planck; it enters G only).  Either output alone has the bits it has beside the other.
 * Adjoint solve.  For a functional Phi(S, alpha) with cotangent c = dPhi/dS and direct part d = dPhi/d ln alpha at fixed S — for the
 * emergent flux R_source and R_alpha of sdx_response_dev(source = S) — sdx_scatter_response_dev solves y = c + Lambda^T (W y):
 *     y^0 = c,   y^(n+1) = y^n + (c + Lambda^T (W y^n) - y^n) / (1 - albedo Lc),   Lc = clamp(L, 0, 1) (NaN -> 0)
 * with L, the clamp, the stopping rule max |dy| <= tol max |y^(n+1)|, status 0 / 1 / 2, the refused non-finite update, the frozen
 * column, `iterations` and `change` exactly those of sdx_scatter_source_dev.  (1 - D M^T) is the transpose of (1 - M D), and M D is
 * similar to D M: the spectral radius is the forward iteration's.  albedo is formed as there (clamped to [0, 1], NaN -> 0, 0 where
 * total_alphas == 0); thermal = NULL: Planck; direct = NULL: 0.
 * Outputs, with z = W y, G of that z, J = Lambda S of the S passed in, A[k] = d[k] + G[k] (the total derivative to ln alpha at fixed
 * albedo) and H[k] = y[k] (J[k] - B[k]) = dPhi/d albedo[k]:
 *     y                                                             (optional)
 *     R_thermal[k]    = (1 - albedo[k]) y[k]                            = dPhi/dB[k]
 *     R_absorption[k] = A[k] - albedo[k] H[k]                           = dPhi/d ln alpha[k] when the added opacity is true absorption
 *                                                                        (alpha_scatter and B fixed): what takes R_alpha's place
 *     R_scatter[k]    = albedo[k] A[k] + albedo[k] (1 - albedo[k]) H[k]  = dPhi/d ln alpha_scatter[k] at fixed absorption
 * each [n_depth][ld], each may be NULL, not all.  The derivatives are exact for the discrete problem AT THE S THAT IS PASSED IN: at an
 * unconverged S (status 1 of sdx_scatter_source_dev) they are the derivatives of the fixed-point equations, not of the truncated
 * iteration.  No atomics and no grid-wide synchronisation: the same bits from run to run, a column's bits do not depend on the grid,
 * the shard or the other columns.
 * Refused with SDX_ERR_ARG before anything is enqueued (also for n_nu = 0): mixed_precision = 1, n_theta > 64, tol < 0 or NaN,
 * max_iter < 1, a model whose columns and stashed sweep — ((n_theta + 10) n_depth + 3 n_theta) doubles at one frequency per wave — do
 * not fit 64 KB of LDS (271 depth points at 20 angles).  Out of scope: spherical geometry, line scattering, second derivatives. */
int sdx_mean_intensity_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                                   const double* temperature, const double* ray_dist, const double* mean_weights,
                                   const double* total_alphas, int64_t alpha_ld, const double* z, int64_t z_ld,
                                   const double* source, int64_t source_ld, double* Lt, int64_t Lt_ld, double* G,
                                   int64_t G_ld);
int sdx_scatter_response_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                             const double* temperature, const double* ray_dist, const double* mean_weights,
                             const double* total_alphas, int64_t alpha_ld, const double* alpha_scatter, int64_t scatter_ld,
                             const double* thermal, int64_t thermal_ld, const double* S, int64_t S_ld,
                             const double* cotangent, int64_t cotangent_ld, const double* direct, int64_t direct_ld,
                             double tol, int max_iter, double* y, int64_t y_ld, double* R_thermal, int64_t R_thermal_ld,
                             double* R_absorption, int64_t R_absorption_ld, double* R_scatter, int64_t R_scatter_ld,
                             int* iterations, int* status, double* change);
/* host-buffer twins: contiguous arrays, planes [n_depth][n_nu]; NULL as above. */
int sdx_mean_intensity_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                                   const double* temperature, const double* ray_dist, const double* mean_weights,
                                   const double* total_alphas, const double* z, const double* source, double* Lt,
                                   double* G);
int sdx_scatter_response_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                             const double* temperature, const double* ray_dist, const double* mean_weights,
                             const double* total_alphas, const double* alpha_scatter, int scatter_per_frequency,
                             const double* thermal, const double* S, const double* cotangent, const double* direct,
                             double tol, int max_iter, double* y, double* R_thermal, double* R_absorption,
                             double* R_scatter, int* iterations, int* status, double* change);

/* ---- per-line flux sensitivities: the adjoint of the line-opacity sum -----------------------------
 * WHICH lines matter: the line opacity scatters, for every line l and depth point d,
 *     alpha_line[d][i] += alpha_ld voigt(nu_i - nu_l; doppler_ld, gamma_ld)     for i in the reference's window [lo_ld, hi_ld)
 * (window opacities_solvers/base.py:556-575, profile voigt.py:17-86,153-155, amplitude base.py:627), and this gathers the same terms per
 * line against a weight plane W:
 *     out_line_depth[l][d] = sum over i in [lo_ld, hi_ld) within the shard of  W[d][i] alpha_ld voigt(nu_i - nu_l; doppler_ld, gamma_ld)
 *     out_line[l]          = sum_d out_line_depth[l][d]
 * the vector-Jacobian product of the line opacity with respect to the logarithm of a per-line (per-line, per-depth) strength.  With
 * W[d][i] = w_i R_alpha[d][i] / total_alphas[d][i] (sdx_response_weight_dev) out_line[l] is d(sum_i w_i F_nu_i[N_d-1]) / d ln(strength of
 * line l) AT FIXED WINDOWS: the derivative of a band flux, an equivalent width or any linear functional of the spectrum with respect to
 * ln gf of every line, in one pass with the Voigt evaluations of one direct-sum line opacity.  The reference has no counterpart.
 * Fixed windows: the reference's window has the half-width int(max(10, (gamma + doppler) alpha / d_nu * 20)), so the flux is a step
 * function of a line's strength wherever that integer moves; this is the derivative between the steps.
 * The windows are formed on the GLOBAL grid and are bit for bit those of sdx_line_windows_dev, clipped to the columns [nu_begin,
 * nu_begin + nu_count); each term is what the fp64 line kernels evaluate, always by the direct sum (no far field, no fp32 path).  The list
 * may be in any order; row k of an output belongs to line k.  Deterministic: no floating-point atomics, every sum in an order that follows
 * from the shapes, the windows and the shard.  Shards add: the sum of the shards' outputs is the whole grid's up to rounding, and an item
 * whose window misses the shard is exactly 0.
 * line arrays as for sdx_line_windows_dev; weight [n_depth][weight_ld], column 0 at global index nu_begin; out_line [n_lines],
 * out_line_depth [n_lines][n_depth]; either may be NULL, not both.  Refused with SDX_ERR_ARG before anything is enqueued (also for
 * n_nu = 0, so a caller can ask at set-up time): a null context, mixed_precision = 1, both outputs NULL, gamma_cols neither 1 nor n_depth,
 * a shard outside the grid.  n_lines = 0 or nu_count = 0: nothing is launched.  Only enqueues on the context's stream; its scratch is the
 * context's and grows outside a capture only (one eager call of the same size first). */
int sdx_line_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                         int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                         int gamma_cols, const double* alphas, const double* weight, int64_t weight_ld,
                         double* out_line, double* out_line_depth);
/* host-buffer twin of sdx_line_adjoint_dev: the whole grid, contiguous arrays, weight [n_depth][n_nu]; out_line or out_line_depth may
 * be NULL. */
int sdx_line_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                         const double* doppler_widths, const double* gammas, int gamma_cols, const double* alphas,
                         const double* weight, double* out_line, double* out_line_depth);
/* ---- line-profile sensitivities: damping, Doppler width and line centre ----------------------------
 * The same gather for the three numbers that set the SHAPE of a line.  The term of line l at depth d and grid point i is T = amp K(x, y)
 * with x = (nu_i - nu_l) / doppler_ld, y = (gamma_ld / (sqrt(pi) pi)) / doppler_ld, amp = alpha_ld / (sqrt(pi) doppler_ld), K = Re w(x + i y)
 * (voigt.py:39-84 for w, :148-149 for x, y and amp).  With the sums over the item's window clipped to the shard
 *     S0 = sum W T,   Sx = sum W amp K_x,   Sxx = sum W amp x K_x,   Sy = sum W amp K_y          (K_x, K_y: sdx_voigt_grad_dev)
 * the outputs are, per (line, depth) in the _depth arrays and summed over depth per line,
 *     out_damping :  d/d ln gamma_ld   =  y Sy
 *     out_doppler :  d/d ln doppler_ld = -(S0 + Sxx + y Sy)           (x, y and amp all carry 1 / doppler)
 *     out_centre  :  d/d nu_l          = -Sx / doppler_ld             (per Hz)
 * of  sum_d sum_i W[d][i] alpha_line[d][i]  AT FIXED WINDOWS AND FIXED REGIONS: the windows as for sdx_line_adjoint_dev (for the centre:
 * the window's centre index held fixed too), the Humlicek region of every term held fixed — the derivative between the steps of the
 * reference's forward model, which is what difference quotients of it give wherever no integer moves.  out_damping[l] is the response
 * to scaling gamma of line l at every depth by one factor, out_doppler[l] likewise; the per-depth arrays keep the depths apart.
 * Arguments, windows, classes, determinism, sharding and refusals as for sdx_line_adjoint_dev (a null context, mixed_precision = 1, all
 * six outputs NULL, gamma_cols neither 1 nor n_depth, a shard outside the grid, the int32 limits: SDX_ERR_ARG before anything is
 * enqueued, also for n_nu = 0); any of the six outputs may be NULL; n_lines = 0 or nu_count = 0 launches nothing.  Only enqueues on the
 * context's stream; scratch as sdx_line_adjoint_dev's, four sums per item: "adjoint_partials" bounds groups of FOUR doubles per (tiled
 * item, supertile) here, i.e. at most min(tiles of the shard, (partials / 4) / tiled items) supertiles per item.  Stage name of the
 * profile hooks: k_line_param_adjoint. */
int sdx_line_param_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                               int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                               int gamma_cols, const double* alphas, const double* weight, int64_t weight_ld,
                               double* out_damping, double* out_doppler, double* out_centre,
                               double* out_damping_depth, double* out_doppler_depth, double* out_centre_depth);
/* host-buffer twin of sdx_line_param_adjoint_dev (x, y, amp: voigt.py:148-149; w: voigt.py:39-84): the whole grid, contiguous arrays,
 * weight [n_depth][n_nu]; any of the six outputs may be NULL, not all. */
int sdx_line_param_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                               const double* doppler_widths, const double* gammas, int gamma_cols, const double* alphas,
                               const double* weight, double* out_damping, double* out_doppler, double* out_centre,
                               double* out_damping_depth, double* out_doppler_depth, double* out_centre_depth);
/* ---- the tangent of the line-opacity sum: forward mode through the lines ----------------------------
 * The Jacobian-vector product the two gathers above are the transposes of.  With T, x, y and amp as above and per line, or per (line,
 * depth), the directions  a = d ln alpha,  g = d ln gamma,  b = d ln doppler,  n = d nu_l (Hz):
 *     out[d][i] = sum over the items (l, d) with i in [lo_ld, hi_ld) of
 *                     a T  +  g (amp y K_y)  -  b (T + amp x K_x + amp y K_y)  -  n (amp K_x / doppler_ld)
 * AT FIXED WINDOWS AND FIXED REGIONS, the window's centre index held too — so that, for every weight plane W,
 *     sum_d sum_i W[d][i] out[d][i] = sum_l sum_d (a S0 + g out_damping + b out_doppler + n out_centre)[l][d]
 * with S0 = sdx_line_adjoint_dev's out_line_depth and the three outputs of sdx_line_param_adjoint_dev.  It is the column of the line
 * opacity for ONE global parameter that acts on many lines: an abundance (a = 1 on the lines of the species), the microturbulence
 * (b = xi (nu_l / c)^2 / doppler_ld^2), a damping enhancement (g), a velocity shift (n); sdx_response_project_dev takes it to the flux.
 * Windows bit for bit those of sdx_line_windows_dev on the GLOBAL grid; T is what the fp64 line kernels evaluate, K_x and K_y are
 * sdx_voigt_grad_dev's; always the direct sum, always fp64, no far field.
 * PRECONDITION, as for sdx_line_opacity_dev: line_nus ascending (the kernel finds a tile's lines as a range of the list); a list in
 * another order gives wrong sums, not an error.  line arrays as for sdx_line_windows_dev; each direction NULL (zero) or
 * [n_lines][dir_cols] with dir_cols 1 or n_depth, one dir_cols for all four; out [n_depth][out_ld], column 0 at global index nu_begin:
 * EVERY element of the columns [0, nu_count) is written, exactly 0.0 where no window covers it.  An item all of whose directions are
 * exactly zero is skipped before any evaluation: a 0 / 1 mask over a species costs what the species costs.
 * Deterministic: no floating-point atomics; a column's sum stays in one lane and runs over the items that cover it in an order the tables
 * alone fix — first those whose half-width exceeds 256 grid points, then the others, each in ascending line order.  The bits are
 * therefore the same from run to run, under graph replay, through the host twin and WHATEVER THE SHARD: a shard's columns are bit for
 * bit the whole-grid call's.
 * Refused with SDX_ERR_ARG before anything is enqueued, also for n_nu = 0: a null context, mixed_precision = 1, all four directions
 * NULL, dir_cols or gamma_cols neither 1 nor n_depth, a shard outside the grid, the int32 limits (n_nu, n_lines * n_depth).  n_lines = 0
 * still writes the zeros; nu_count = 0 launches nothing.  Only enqueues on the context's stream; its scratch is the context's (shared
 * with the two gathers) and grows outside a capture only.  Stage name of the profile hooks: k_line_tangent. */
int sdx_line_tangent_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                         int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                         int gamma_cols, const double* alphas, const double* d_strength, const double* d_damping,
                         const double* d_doppler, const double* d_centre, int dir_cols, double* out, int64_t out_ld);
/* host-buffer twin of sdx_line_tangent_dev: the whole grid, contiguous arrays, out [n_depth][n_nu]; the same bits. */
int sdx_line_tangent_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                         const double* doppler_widths, const double* gammas, int gamma_cols, const double* alphas,
                         const double* d_strength, const double* d_damping, const double* d_doppler, const double* d_centre,
                         int dir_cols, double* out);
/* The weight plane of the flux sensitivities from the response functions (sdx_response_dev):
 *     weight[k][j] = nu_weight[j] (R_alpha[k][j] / total[k][j])          (nu_weight = NULL: 1)
 * every operation one correctly rounded fp64 operation; a zero in total gives what IEEE gives (as sdx_response_project_dev). */
int sdx_response_weight_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* R_alpha, int64_t R_ld,
                            const double* total, int64_t total_ld, const double* nu_weight, double* weight, int64_t weight_ld);

/* ---- isolated-line equivalent widths and line depths: one line alone over a background ----------------
 * HOW STRONG is this one line, on its own: what a one-line synthesis over the background gives, integrated by the trapezoid rule over
 * the points the line reaches — per selected line and per trial strength, without a step per line.  The reference has no counterpart.
 * For a selected line l and a strength factor s (row j, column k of the outputs):
 *   alpha'[d] = mul_rn(alphas[l][d], s).
 *   The window at depth d is the window rule (opacities_solvers/base.py:556-575) on the GLOBAL grid with alpha'[d]: bit for bit the window
 *     sdx_line_windows_dev gives for a table holding alpha'.
 *   A[d][i] = add_rn(B[d][i], term), B the caller's background opacity plane; inside the depth's window term is the line's term as the
 *     fp64 line kernels and the adjoints evaluate it (1 / doppler, y and the amplitude from doppler, gamma and alpha'), outside it is +0.
 *   F(i) and F_B(i) are the emergent fluxes (row n_depth - 1) of the plane-parallel formal solution of A and of B: the Planck source, the
 *     step's coefficients with the tau = 0 -> (1, 0) rule, the angles summed in sdx_raytrace_dev's order.  Both are formed in the same
 *     launch by the same operations from the same staged source values and ray lengths, so where the line adds exactly zero at every
 *     depth F and F_B have the same bits.
 *   r(i) = (F_B(i) - F(i)) / F_B(i): one subtraction and one IEEE division (not 1 - F / F_B).
 *   U is the union over depth of the windows (an interval).
 *   Node weights on the caller's abscissa x[n_nu] (global, strictly monotone; lambda in Angstrom gives W in Angstrom):
 *     h(i) = 1/2 (|x[i+1] - x[i]| [i+1 in U] + |x[i] - x[i-1]| [i-1 in U]),  U the UNCLIPPED union, so frequency shards add.
 *   W = sum over i in U within the shard of h(i) r(i);  depth = max over the same i of r(i);  both 0.0 where no such i exists.
 *   Shards combine W by addition and depth by max; the max of the shards' depths is exact whenever some r >= 0 (a shard without
 *   points reports 0.0, which the max then ignores; where every r is negative it would win).
 * A zero-strength line gives W = depth = 0 exactly.  Row j depends on its own line and strength alone: not on what else is selected,
 * nor on n_scale.  Deterministic: no floating-point atomics, every sum in an order that the tables, the selection and the shard fix.
 * Always fp64, always the direct sum (no far field), the Planck source, plane-parallel geometry.
 * nus [n_nu]; the shard is the columns [nu_begin, nu_begin + nu_count); line arrays as for sdx_line_adjoint_dev (any order; gamma_cols 1
 * or n_depth); line_index [n_sel] (int64, device; repeats allowed), NULL: all lines, n_sel = n_lines; scale [n_sel][n_scale], NULL: 1.0,
 * n_scale >= 1; background [n_depth][background_ld], column 0 at global index nu_begin; temperatures [n_depth]; ray_dist
 * [n_depth - 1][n_theta]; theta_weights [n_theta]; out_W and out_depth [n_sel][n_scale], either may be NULL, not both.
 * Refused with SDX_ERR_ARG before anything is enqueued (also for an empty selection, so a caller can ask at set-up time): a null context,
 * mixed_precision = 1, n_depth < 2, n_theta outside 1..64, a model whose columns do not fit LDS at one frequency per wave, both outputs
 * NULL, gamma_cols neither 1 nor n_depth, a shard outside the grid, n_sel * n_scale * nu_count beyond 2^34.  The indices of line_index
 * live in device memory and are NOT checked here: the kernels clamp them into [0, n_lines) (no access out of bounds, the clamped line's
 * values); ops.equivalent_widths and SpectralSynthesizer.equivalent_widths check them on the host before upload and raise.
 * n_sel = 0 or nu_count = 0: SDX_OK, nothing is launched.  Only enqueues on the context's stream and reads nothing back, so it can be
 * captured; its scratch is the context's (shared with the line adjoints) and grows outside a capture only (one eager call of the same
 * size first).  Stage name of the profile hooks: k_line_ew (five launches). */
int sdx_line_equivalent_widths_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                                   const double* x, int64_t n_lines, const double* line_nus, const double* doppler_widths,
                                   const double* gammas, int gamma_cols, const double* alphas, int64_t n_sel,
                                   const int64_t* line_index, int n_scale, const double* scale, const double* background,
                                   int64_t background_ld, int n_theta, const double* temperatures, const double* ray_dist,
                                   const double* theta_weights, double* out_W, double* out_depth);

/* ---- fused synthesis for resident data (the benchmark path) ---------------------------------
 * total_alphas[d,i] = ((((file + bf) + ff) + rayleigh) + electron) + line   in calc_alphas order
 * (:655-738), then raytrace.  Any source pointer group may be NULL (skipped, contributes nothing).
 * All arrays are device-resident; outputs cover columns nu_begin .. nu_begin+nu_count-1. */
typedef struct sdx_continuum {
    /* alpha_file_Hminus_bf style 1-D table source */
    const double* lambdas;          /* [n_nu] Angstrom, global grid */
    int n_table;
    const double* table_wavelength; /* [n_table] */
    const double* table_sigma;      /* [n_table] */
    const double* table_density;    /* [n_depth] */
    /* bf */
    int bf_n_species;
    int bf_n_levels;                /* = bf_species_offsets[bf_n_species], known to the host */
    const int32_t* bf_species_offsets;
    const int32_t* bf_species_ion_number;
    const double* bf_cutoff;
    const double* bf_level_density;
    /* ff */
    int ff_n_species;
    const int32_t* ff_species_ion_number;
    const double* ff_number_density;
    /* rayleigh (all NULL: source returns zeros, as the reference does for an empty species list) */
    const double* ray_n_h;
    const double* ray_n_he;
    const double* ray_n_h2;
    int rayleigh_enabled;
    /* electron */
    const double* electron_density; /* NULL = disable_electron_scattering */
    const double* temperature;      /* [n_depth] */
    /* further alpha_file_<source> planes, already formed on the device (sdx_alpha_file_1d_dev / sdx_alpha_file_2d_dev: the
     * two-dimensional tables Hminus_ff and H2plus_bf, or several tabulated sources at once): [n_depth][file_plane_ld] each,
     * column 0 = grid index 0, added right after the 1-D table above in this order — with the table left out (table_sigma NULL)
     * the planes are calc_alphas' file loop (:666-677) in the configuration's own order.  Device pointers only: the host-buffer
     * entry points (*_f64) refuse a description that carries planes. */
    int n_file_planes;              /* 0 .. 4 */
    const double* file_plane[4];
    int64_t file_plane_ld;
} sdx_continuum;

/* calc_alpha_file / calc_alpha_bf / calc_alpha_ff / calc_alpha_rayleigh / calc_alpha_electron (opacities_solvers/base.py:40-317)
 * and their sum in calc_alphas' order (:655-700) for a caller that holds everything in HOST memory (numpy through ctypes, C):
 * `cont` carries host pointers here (array lengths follow from the sizes in the struct; no file planes), every output is an
 * optional host array [n_depth][n_nu]; one upload of the inputs, one download per requested plane, on the context's
 * persistent staging.  alpha_rayleigh != NULL also reproduces the reference's side effect (:99): frequencies above 2.3e15 Hz
 * are set to 0 in the caller's `nus`.  alpha_electron with electron_density == NULL is a plane of zeros (the reference
 * returns the scalar 0 there, :164-165).  total_alphas = ((((file + bf) + ff) + rayleigh) + electron), sources that are
 * absent contributing nothing. */
int sdx_continuum_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* nus, const sdx_continuum* cont, double* alpha_file,
                      double* alpha_bf, double* alpha_ff, double* alpha_rayleigh, double* alpha_electron, double* total_alphas);

int sdx_total_alphas_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin,
                         int64_t nu_count, const sdx_continuum* cont, const double* alpha_line, int64_t line_ld,
                         double* total_alphas, int64_t total_ld);

/* ---- post-processing ---------------------------------------------------------------------------
 * scipy.ndimage.convolve1d(in, weights) with mode='reflect', origin 0, odd kernel length: the operation
 * rotation_broadening applies to the spectrum (opacities_solvers/broadening.py:869-871).  symmetric != 0 selects
 * scipy's pairwise order for symmetric kernels (the caller applies scipy's DBL_EPSILON symmetry test). */
int sdx_convolve1d_reflect_dev(sdx_ctx* ctx, int64_t n, const double* in, int m, const double* weights, int symmetric,
                               double* out);
/* spectrum_lambda = F_nu * nu / lambda, element-wise (stardis/base.py:137-141) — keeps the emergent spectrum on the
 * device between the formal solution and the instrumental / rotational convolutions */
int sdx_flux_nu_to_lambda_dev(sdx_ctx* ctx, int64_t n, const double* f_nu, const double* nus, const double* lambdas, double* out);
/* out[i] = a[i] / b[i] (the continuum-normalised spectrum: flux over continuum). */
int sdx_divide_dev(sdx_ctx* ctx, int64_t n, const double* a, const double* b, double* out);

/* ---- instrument model: Doppler shift, line-spread function, pixel integration ---------------------
 * From a spectrum on the model's own grid to what a spectrograph records, in one launch (k_observe).  The reference has no
 * counterpart: its rotation-broadening walk-through smooths the spectrum with scipy.ndimage.gaussian_filter1d at ONE sigma in grid
 * points (mirrored by stardis_amd.postprocess.gaussian_filter1d), which is a line-spread function of constant resolving power only
 * on a log-uniform grid, shifts nothing and rebins nothing.  This generalises it: the width is given per pixel in Angstrom, on any
 * ascending grid.  fp64 whatever "mixed_precision" says; every operation below is one correctly rounded fp64 operation.
 *   lambdas[n]     strictly ascending wavelengths (Angstrom), flux[n] the spectrum on them, reference[n] optional (NULL: none);
 *   edges[n_pix+1] strictly ascending pixel edges (Angstrom), sigma[n_pix] > 0 the Gaussian width of the line-spread function at
 *                  each pixel (Angstrom; constant resolving power R: sigma = centre / (R 2 sqrt(2 ln 2)));
 *   D              the Doppler factor sqrt((1 + beta) / (1 - beta)), beta = v_rad / c: x_i = lambdas[i] D.  Only the wavelengths
 *                  move; the flux is not rescaled.
 * Trapezoid weights h_i = (x[i+1] - x[i-1]) / 2, at the ends h_0 = (x[1] - x[0]) / 2 and h_{n-1} = (x[n-1] - x[n-2]) / 2.  The Gaussian
 * around x_i integrated over pixel j, with a = (edges[j] - x_i) / (sigma[j] sqrt 2), b = (edges[j+1] - x_i) / (sigma[j] sqrt 2):
 *     r = 0.5 (erfc(a) - erfc(b))  where a > 0,   r = 0.5 (erfc(-b) - erfc(-a))  where b < 0,   r = 0.5 (erf(b) - erf(a))  otherwise
 * (the tails keep their relative accuracy).  The window of pixel j is the points with lo_j <= x_i <= hi_j, lo_j = edges[j] - 8 sigma[j],
 * hi_j = edges[j+1] + 8 sigma[j] (what lies outside is below 1e-15 of the sum), and over it
 *     out[j] = (sum_i r h_i flux[i]) / (sum_i r h_i g_i),   g_i = 1, or reference[i]:
 * with a reference the continuum-normalised observed spectrum, observe(flux) / observe(reference), from the same launch.  A pixel
 * whose window the grid does not cover, !(lo_j >= x_0 && hi_j <= x_{n-1}), is NaN.
 * Accuracy, measured against an extended-precision evaluation of this definition (profiles/observe_truth_classes.json): for pixels not
 * much narrower than sigma out[j] is the definition's to a few ulp of (sum_i |w_ij flux[i]| + |out[j]| sum_i |w_ij g_i|) / |den_j| (1e-16 to
 * 4e-16; 4e-15 where one far-tail weight carries the value), far-tail spikes, deep cores, points on the edges and 1e+-150 included.  For
 * width / sigma << 1 the loss is the conditioning of the erfc difference — an argument's rounding is amplified by 2 p^2 and one ulp of
 * erfc by sigma / width — and belongs to any fp64 evaluation: 2e-16, 3e-14, 2e-12 at width / sigma = 1e-2, 1e-4, 1e-6 on a smooth
 * spectrum, 2e-14, 2e-12, 2.5e-10 with a spike of 1e12 to 1e14 in a far tail.
 * out depends on the arrays alone: no floating-point atomics, and the order of the sums does not follow from the device or the
 * launch — two calls, and the replay of a captured graph, give the same bits.
 * sdx_observe_dev: device pointers, asynchronous on the context's stream, no allocation, no synchronisation (capturable).  The Doppler
 * factor is read from device memory when the kernel runs (doppler_dev; NULL: 1), so a captured graph follows a new velocity without
 * being recorded again.  n_pix = 0 returns at once; n < 2 or a null required pointer is SDX_ERR_ARG before anything is enqueued.  The
 * arrays' contents cannot be checked here: whatever they hold (NaN, unordered values, sigma <= 0), every access stays inside the
 * arrays and a pixel's loop runs at most n trips — the result is then meaningless, never an out-of-range access.
 * Stage name for sdx_profile_get: "k_observe". */
int sdx_observe_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                    const double* edges, const double* sigma, const double* doppler_dev, double* out);
/* host-buffer twin: host pointers, the Doppler factor by value.  The arrays ARE checked here, before any upload: lambdas and edges
 * finite and strictly ascending, sigma finite and > 0, doppler finite and > 0; anything else is SDX_ERR_ARG with a message that names
 * the argument. */
int sdx_observe_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                    const double* edges, const double* sigma, double doppler, double* out);

/* ---- the adjoint of the instrument model: from pixel weights to grid weights -----------------------
 * The vector-Jacobian product of sdx_observe_dev: a vector c over the pixels pulled back to a vector over the grid points, so that the
 * derivative of any functional of the OBSERVED pixels (a chi-square against data, an equivalent width measured on the detector) becomes
 * weights over the model's own columns — what sdx_line_adjoint_dev and the response functions take.  In the notation above, every
 * quantity formed with the same operations and roundings as k_observe:
 *     x_i = lambdas[i] D,  h_i its trapezoid weight,  lo_j = edges[j] - 8 sigma[j],  hi_j = edges[j+1] + 8 sigma[j],
 *     covered_j = (lo_j >= x_0 && hi_j <= x_{n-1}),  w_ij = r_ij h_i  (bit for bit the weight of k_observe's loop),
 *     den_j = sum_i w_ij g_i  (g = 1, or reference),   out_j = (sum_i w_ij flux[i]) / den_j   over the window lo_j <= x_i <= hi_j,
 * and for the pixel vector pixel_weight = c[n_pix]
 *     a_j          = covered_j ? c_j / den_j : 0      (c_j of an uncovered pixel is never used, whatever it holds, NaN included)
 *     w_flux[i]    = sum over the j with covered_j and lo_j <= x_i <= hi_j of  w_ij a_j
 *     w_reference[i] = the same sum of  w_ij (-out_j a_j)     (with a reference only: the cotangent of `reference`)
 * so that  sum_j c_j out_j = sum_i w_flux[i] flux[i]  over the covered pixels and  sum_j c_j d out_j / d reference[i] = w_reference[i].
 * A grid point in no covered pixel's window is exactly 0.0.  The windows are fixed: no derivative to D or sigma.
 * nus[n] (optional) turns weights over F_lambda into weights over F_nu, the transpose of sdx_flux_nu_to_lambda_dev: both outputs
 * become (w nus[i]) / lambdas[i], and feed sdx_response_weight_dev (nu_weight) directly.
 * sigma is per pixel, so lo_j and hi_j need not ascend with j and the pixels that hold a point need not be consecutive: the
 * candidates of a point are bracketed by a prefix maximum of hi and a suffix minimum of lo (exact: max and min round nothing) and each is
 * tested with the predicate above — the set is exactly the transpose of the forward windows on an ascending grid.
 * fp64, every operation one rounded operation; no floating-point atomics; the order of every sum follows from the arrays alone
 * (ascending j dealt round-robin to the lanes of the point, then a butterfly): two calls, and the replay of a captured graph, give the
 * same bits.  The lanes per point (8 or 64) follow from an estimate of the pixels per point, 1 + 16 sigma / (the mean pixel width) with
 * sigma that of pixel floor((x_i - edges[0]) / mean width) clamped to the array, against 32, over groups of 8 consecutive points.
 * sdx_observe_adjoint_dev: device pointers, asynchronous on the context's stream, capturable; D is read from device memory when the
 * kernels run (doppler_dev; NULL: 1), so a captured call follows a new velocity.  Its scratch (a, -out a and the two scans: 4 n_pix
 * doubles and a little) is the context's and grows outside a capture only (one eager call of the same size first).  flux is read only with a
 * reference (NULL otherwise); nus and w_reference are optional.  n_pix = 0 writes zeros to the outputs and returns.  SDX_ERR_ARG
 * before anything is enqueued, the context usable afterwards: n < 2, a null required pointer (lambdas, w_flux; edges, sigma,
 * pixel_weight unless n_pix = 0), w_reference without reference, reference without flux.  The arrays' contents cannot be checked
 * here: whatever they hold (NaN, unordered values, sigma <= 0), every access stays inside the arrays and every loop has a bound that
 * follows from n and n_pix — the result is then meaningless, never an out-of-range access.
 * Stage name for sdx_profile_get: "k_observe_adjoint" (four launches: per-pixel factors, the scans in two, the gather per point). */
int sdx_observe_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, const double* doppler_dev, const double* pixel_weight,
                            const double* nus, double* w_flux, double* w_reference);
/* host-buffer twin: host pointers, the Doppler factor by value.  lambdas, edges, sigma and doppler are checked as by sdx_observe_f64
 * before any upload (SDX_ERR_ARG with a message that names the argument); pixel_weight may hold anything. */
int sdx_observe_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, double doppler, const double* pixel_weight, const double* nus,
                            double* w_flux, double* w_reference);

/* ---- rotational broadening (v sin i) in velocity space, and its adjoint ----------------------------
 * Gray's rotation profile on ANY ascending grid, applied on the rest-frame grid in front of sdx_observe_dev (the operator is
 * multiplicative in lambda, so it commutes with the Doppler shift and does not read the Doppler factor).  The reference's
 * rotation_broadening (mirrored by stardis_amd.postprocess.rotation_broadening) samples the kernel at integer pixel offsets for one
 * velocity per pixel, which is a rotation profile on a log-uniform grid only, and has no transpose.
 *   lambdas[n]  strictly ascending rest-frame wavelengths (Angstrom), flux[n], reference[n] optional (NULL: none);
 *   V = v sin i >= 0 in km/s, eps in [0, 1] the linear limb-darkening coefficient; beta = V / c, c = 299792.458 km/s.
 * For point i, every operation one correctly rounded fp64 operation, in this order (the device function rot_weight):
 *     reach_i = lambdas[i] beta,   lo_i = lambdas[i] - reach_i,   hi_i = lambdas[i] + reach_i,
 *     y_ij = (lambdas[j] - lambdas[i]) / reach_i,   q_ij = 1 - y_ij y_ij,
 *     INCLUDED(i, j) = (lo_i <= lambdas[j] && lambdas[j] <= hi_i && q_ij > 0) || j == i      (j = i: q = 1),
 *     K_ij = (2 (1 - eps)) sqrt(q_ij) + ((pi / 2) eps) q_ij      (Gray's profile, unnormalised),
 *     h_j = (lambdas[j+1] - lambdas[j-1]) / 2, the ends clamped as in sdx_observe_dev,      w_ij = K_ij h_j,
 *     den_i = sum_j w_ij,   out[i] = (sum_j w_ij flux[j]) / den_i,   out_reference[i] = (sum_j w_ij reference[j]) / den_i
 * over the included j — the discrete form of  integral flux(lambda_i (1 - v / c)) G_rot(v) dv.  den_i > 0 always (i includes itself),
 * so a constant stays constant to rounding and nothing is NaN.  A window that reaches past an end of the grid is TRUNCATED AND
 * RENORMALISED: it sums what exists, and the points within reach of either end are edge-affected (Instrument.edge_affected reports
 * the pixels they feed).  !(V > 0) — zero, negative, NaN — is a copy: out[i] = flux[i] bit for bit.
 * The sums: a point's 8 or 64 lanes take its window round-robin from the first point with lambdas >= lo_i, each adds in ascending j,
 * and a butterfly (offsets W/2 ... 1) closes them; 8 lanes where no point of the group of 8 expects more than 32 points,
 * 2 beta lambdas[i] (n - 1) / (lambdas[n-1] - lambdas[0]).  No floating-point atomics: two calls, and the replay of a captured graph,
 * give the same bits.
 * sdx_rotate_dev: device pointers, asynchronous on the context's stream, no allocation, capturable.  rot_dev: two doubles in device
 * memory, {V, eps}, read when the kernel runs — a captured graph follows new values.  SDX_ERR_ARG before anything is enqueued: n < 2,
 * a null required pointer, reference without out_reference or the reverse, an output that is one of the inputs.  The arrays'
 * contents cannot be checked here: whatever they hold (NaN, unordered values, any V and eps), every access stays inside the arrays and
 * every loop is bounded by its bracket within [0, n) — the result is then meaningless, never an out-of-range access.
 * Stage name for sdx_profile_get: "k_rotate". */
int sdx_rotate_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* rot_dev,
                   double* out, double* out_reference);
/* The transpose: for weights u (and u_reference) over the BROADENED points,
 *     a_i = u[i] / den_i,     w[j] = sum over the i with INCLUDED(i, j) of  w_ij a_i       (w_reference: the same with u_reference),
 * w_ij bit for bit the forward's, so that  sum_i u[i] out[i] = sum_j w[j] flux[j].  With nus, both outputs become (w nus[j]) /
 * lambdas[j], as sdx_observe_adjoint_dev ends.  The candidates i of a point j have lambdas[i] in [lambdas[j] / (1 + beta), lambdas[j] /
 * (1 - beta)]; that range is searched a few 1e-15 wide and every candidate is tested with INCLUDED.  Ascending i round-robin over the
 * point's lanes, then the butterfly; no floating-point atomics.  Its scratch (a: two rows of n) is the context's and grows outside a
 * capture only.  !(V > 0): w = u.  Refusals and bounds as above.  Stage name: "k_rotate_adjoint" (two launches: a, the gather).
 * The broadening stages (this one, sdx_rotate_integrated_dev, sdx_macroturbulence_dev) share this adjoint and their host-buffer twins.
 * A stage provides its profile from its device scalar(s) with "the stage is on", its window's width over lambdas[i], den_i from its own
 * sums, per node j the candidate range and what j's weights share, and the weight of point i for node j; one kernel pair, one launch
 * routine with one scratch of the context's (an adjoint consumes it between its own two launches) and one twin each way serve all. */
int sdx_rotate_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* rot_dev, const double* u, const double* u_reference,
                           const double* nus, double* w, double* w_reference);
/* host-buffer twins: host pointers, V and eps by value.  Checked before any copy: lambdas finite and strictly ascending, v_rot finite
 * with 0 <= v_rot < 3000, 0 <= limb_darkening <= 1; anything else is SDX_ERR_ARG with a message that names the argument. */
int sdx_rotate_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                   double limb_darkening, double* out, double* out_reference);
int sdx_rotate_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double v_rot, double limb_darkening, const double* u,
                           const double* u_reference, const double* nus, double* w, double* w_reference);

/* ---- radial-tangential macroturbulence in velocity space, its adjoint and its derivative to zeta ----
 * Gray's radial-tangential profile with equal areas and zeta_R = zeta_T = zeta, integrated over the disk without limb darkening, has
 * the closed form  M(u) ~ K(u) = exp(-u^2) - sqrt(pi) u erfc(u),  u = |dv| / zeta:  K(0) = 1, K > 0, K ~ exp(-u^2) / (2 u^2) for large u,
 * integral of K du = sqrt(pi) / 4 per side, and dK/du = -sqrt(pi) erfc(u), so that  dK / d ln zeta = s(u) = sqrt(pi) u erfc(u), the term K
 * is made of.  K(6) = 3.1e-18 and the mass beyond u = 6 is 5.6e-19 of the total: the window is |u| <= 6.
 * ORDER IN THE CHAIN: rotation (sdx_rotate_dev), then macroturbulence, then sdx_observe_dev; the adjoint runs the stages in reverse.
 * Both broadenings are convolutions in velocity and commute on a log-uniform grid; on other grids, and at the ends, this order is the
 * definition.  Applied on the rest-frame grid, like the rotation.
 *   lambdas[n]  strictly ascending rest-frame wavelengths (Angstrom), flux[n], reference[n] optional (NULL: none);
 *   zeta >= 0 in km/s; beta = zeta / c, c = 299792.458 km/s.
 * For point i, every operation one rounded fp64 operation (exp and erfc: the device library's), in this order (the device function
 * mac_weight):
 *     reach_i = lambdas[i] (6 beta),   lo_i = lambdas[i] - reach_i,   hi_i = lambdas[i] + reach_i,
 *     INCLUDED(i, j) = (lo_i <= lambdas[j] && lambdas[j] <= hi_i) || j == i,
 *     u_ij = |lambdas[j] - lambdas[i]| / (lambdas[i] beta),
 *     j == i: K = 1, s = 0;   else e = exp(-(u u)),   s = (sqrt(pi) u) erfc(u),   K = max(e - s, 0),
 *     h_j = (lambdas[j+1] - lambdas[j-1]) / 2, the ends clamped as in sdx_observe_dev,      w_ij = K h_j,   v_ij = s h_j,
 *     den_i = sum_j w_ij,   out[i] = (sum_j w_ij flux[j]) / den_i,   out_reference[i] = (sum_j w_ij reference[j]) / den_i,
 *     dout[i] = (sum_j v_ij flux[j] - out[i] sum_j v_ij) / den_i,   dout_reference[i] likewise with reference and out_reference
 * over the included j.  dout = d out / d ln zeta AT FIXED WINDOWS (a point entering a window brings 3e-18 of the peak); d out / d zeta
 * = dout / zeta.  den_i > 0 always (i includes itself).  A window that reaches past an end of the grid is TRUNCATED AND RENORMALISED, as
 * the rotation's is: it sums what exists (Instrument.edge_affected reports the pixels concerned).  !(zeta > 0) — zero, negative, NaN —
 * is a copy: out[i] = flux[i] bit for bit, dout[i] = 0.
 * The sums: as sdx_rotate_dev's — a point's 8 or 64 lanes take its window round-robin from the first point with lambdas >= lo_i, each
 * adds in ascending j, and a butterfly (offsets W/2 ... 1) closes them; 8 lanes where no point of the group of 8 expects more than 32
 * points, 2 (6 beta) lambdas[i] (n - 1) / (lambdas[n-1] - lambdas[0]).  No floating-point atomics: two calls, the replay of a captured
 * graph and the host-buffer twin give the same bits.
 * sdx_macroturbulence_dev: device pointers, asynchronous on the context's stream, no allocation, capturable.  mac_dev: one double in
 * device memory, zeta, read when the kernel runs — a captured graph follows a new value.  dout and dout_reference are optional (NULL:
 * not formed).  SDX_ERR_ARG before anything is enqueued: n < 2, a null required pointer (out is required: no dout without out),
 * reference without out_reference or the reverse, dout_reference without reference, an output that is one of the inputs or another
 * output.  The arrays' contents cannot be checked here: whatever they hold (NaN, unordered values, any zeta), every access stays inside
 * the arrays and every loop is bounded by its bracket within [0, n) — the result is then meaningless, never an out-of-range access.
 * Stage name for sdx_profile_get: "k_macroturbulence". */
int sdx_macroturbulence_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* mac_dev,
                            double* out, double* out_reference, double* dout, double* dout_reference);
/* The transpose: for weights u (and u_reference) over the BROADENED points,
 *     a_i = u[i] / den_i,     w[j] = sum over the i with INCLUDED(i, j) of  w_ij a_i       (w_reference: the same with u_reference),
 * w_ij bit for bit the forward's, so that  sum_i u[i] out[i] = sum_j w[j] flux[j].  With nus, both outputs become (w nus[j]) /
 * lambdas[j], as sdx_observe_adjoint_dev ends.  The candidates i of a point j have lambdas[i] in [lambdas[j] / (1 + 6 beta), lambdas[j] /
 * (1 - 6 beta)]; that range is searched a few 1e-15 wide and every candidate is tested with INCLUDED.  Ascending i round-robin over
 * the point's lanes, then the butterfly; no floating-point atomics.  Its scratch (a: two rows of n) is the context's and grows outside
 * a capture only.  !(zeta > 0): w = u.  Refusals (w and w_reference must be buffers of their own) and bounds as above.  Stage name:
 * "k_macroturbulence_adjoint" (two launches: a, the gather). */
int sdx_macroturbulence_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* mac_dev, const double* u,
                                    const double* u_reference, const double* nus, double* w, double* w_reference);
/* host-buffer twins: host pointers, zeta by value.  Checked before any copy: lambdas finite and strictly ascending, zeta finite with
 * 0 <= zeta < 500; anything else is SDX_ERR_ARG with a message that names the argument. */
int sdx_macroturbulence_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double zeta,
                            double* out, double* out_reference, double* dout, double* dout_reference);
int sdx_macroturbulence_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double zeta, const double* u, const double* u_reference,
                                    const double* nus, double* w, double* w_reference);

/* ---- the tangent of the instrument model: d observed / d (v_rad, LSF width, input spectrum), forward mode ----
 * The Jacobian-vector products of sdx_observe_dev, one pass over sdx_observe_dev's own windows (k_observe_tangent): where the adjoint
 * above takes one functional of the pixels back to every grid point, this takes one direction — a parameter, or a tangent of the
 * spectrum on the grid — forward to every pixel: the columns d out_j / d p that a Gauss-Newton or Levenberg-Marquardt fit of the few
 * global parameters needs.  In the notation of sdx_observe_dev (x_i = lambdas[i] D, h_i, lo_j, hi_j, covered_j, r_ij, w_ij = r_ij h_i,
 * den_j = sum_i w_ij g_i, out_j = sum_i w_ij flux[i] / den_j, every one of them formed by the same code as k_observe's), with
 * a' = (edges[j] - x_i) / sigma[j], b' = (edges[j+1] - x_i) / sigma[j] and phi the unit normal density:
 *     dr/dx = (phi(a') - phi(b')) / sigma[j],        dr/d ln sigma = a' phi(a') - b' phi(b')        (the device function obs_response_grad),
 *     d w_ij / d ln D = (x_i dr/dx + r_ij) h_i   (h_i scales with D),        d w_ij / d ln sigma[j] = (dr/d ln sigma) h_i,
 *     dout_p[j] = (sum_i d_p w_ij flux[i] - out_j sum_i d_p w_ij g_i) / den_j        for p = ln D and p = ln sigma,
 *     dout_velocity[j] = dout_lnD[j] (D^2 + 1)^2 / (4 D^2 c)      per km/s of v_rad (d ln D / dv for D = sqrt((1 + beta) / (1 - beta))),
 *     dout_lsf[j]      = dout_ln sigma[j]: the derivative to ln kappa of a common factor kappa on every sigma[j]; for a resolving power
 *                        R (sigma = centre / (R 2 sqrt(2 ln 2))) this is -d / d ln R,
 *     dout_flux[j]     = (sum_i w_ij dflux[i] - out_j sum_i w_ij dreference[i]) / den_j     (the tangent of the quotient for the direction
 *                        (dflux, dreference) of (flux, reference); without dreference the second term is absent).
 * THE WINDOWS AND covered ARE FIXED, as for the derivative to zeta: a point that enters a window when D or sigma moves carries 1e-15 of
 * the sum.  The difference phi(a') - phi(b') is formed as e^(-near^2 / 2) expm1(-(|a'^2 - b'^2|) / 2) from the nearer edge, a'^2 - b'^2 =
 * (a' - b')(a' + b') taken from the differences of the edges and of the point, so that it keeps its relative accuracy for a pixel much
 * narrower than sigma and where both edges lie in one tail; dr/d ln sigma = near (phi(a') - phi(b')) + (a' - b') phi(far), the product
 * rule over the same two differences.  An uncovered pixel is NaN in every output.  `out`, when asked for, is sdx_observe_dev's bit for
 * bit.  fp64, every operation one rounded operation (exp, expm1, erf, erfc: the device library's); no floating-point atomics, the order
 * of every sum follows from the arrays alone: two calls, the replay of a captured graph and the host-buffer twin give the same bits.
 * The derivative to v sin i is sdx_rotate_integrated_dev's dout_lnv below, for the cell-integrated rotation profile; the sampled sum of
 * sdx_rotate_dev has none (Gray's profile ends in a square root, and the trapezoid sum has a square-root kink in V wherever a point enters
 * a window).  Its derivative to eps is bounded and is sdx_rotate_tangent_dev below.
 * sdx_observe_tangent_dev: device pointers, asynchronous on the context's stream, no allocation, capturable; D is read from device
 * memory when the kernel runs (doppler_dev; NULL: 1) and the velocity factor is formed from it there, so a captured call follows a new
 * velocity.  reference, dflux, dreference and every output are optional (NULL: not read, not formed, not written; the parameter sums
 * are formed only with dout_velocity or dout_lsf).  SDX_ERR_ARG before anything is enqueued: n < 2 (n_pix = 0 returns at once), a null
 * required pointer (lambdas, flux, edges, sigma), dreference without reference, dflux without dout_flux or the reverse, an output that
 * is one of the inputs or another output.  The arrays' contents cannot be checked here: whatever they hold (NaN, unordered values,
 * sigma <= 0), the searches and loops are sdx_observe_dev's own — every access stays inside the arrays and a pixel's loop runs at most n
 * trips, reading lambdas at i - 1, i, i + 1 clamped and flux, reference, dflux, dreference at i — and a pixel writes only its own
 * element of each output: the result is then meaningless, never an out-of-range access.
 * Stage name for sdx_profile_get: "k_observe_tangent". */
int sdx_observe_tangent_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, const double* doppler_dev, const double* dflux,
                            const double* dreference, double* out, double* dout_velocity, double* dout_lsf, double* dout_flux);
/* host-buffer twin: host pointers, the Doppler factor by value; lambdas, edges, sigma and doppler are checked as by sdx_observe_f64
 * before any upload. */
int sdx_observe_tangent_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, double doppler, const double* dflux, const double* dreference,
                            double* out, double* dout_velocity, double* dout_lsf, double* dout_flux);
/* r, dr/dx and dr/d ln sigma of the pixel response point by point, as the tangent's loop evaluates them (obs_response and
 * obs_response_grad with sigma sqrt 2 rounded as there): n values of (e0, e1, x, sigma) -> three arrays of n.  For tests.
 * Stage name: "k_observe_response_grad". */
int sdx_observe_response_grad_dev(sdx_ctx* ctx, int64_t n, const double* e0, const double* e1, const double* x, const double* sigma,
                                  double* out_r, double* out_rx, double* out_rs);
int sdx_observe_response_grad_f64(sdx_ctx* ctx, int64_t n, const double* e0, const double* e1, const double* x, const double* sigma,
                                  double* out_r, double* out_rx, double* out_rs);
/* sdx_rotate_dev with its derivative to the limb-darkening coefficient from the same pass (k_rotate_tangent: k_rotate's body with a
 * compile-time flag; rot_weight stays the one place where a pair is included and K is rounded).  K is linear in eps, so with the
 * sqrt(q_ij) and q_ij of the forward weight
 *     dw_ij = (-2 sqrt(q_ij) + (pi / 2) q_ij) h_j,      dout_eps[i] = (sum_j dw_ij flux[j] - out[i] sum_j dw_ij) / den_i,
 * dout_eps_reference likewise with reference and out_reference: d out / d eps, exact (the windows do not depend on eps).  out and
 * out_reference are sdx_rotate_dev's bit for bit.  !(V > 0) copies and writes zeros to the derivative outputs.  out and dout_eps are
 * required, dout_eps_reference is optional and needs a reference; otherwise sdx_rotate_dev's refusals (every output a buffer of its
 * own) and bounds.  Stage name: "k_rotate_tangent".  The host-buffer twin checks its arguments as sdx_rotate_f64 does. */
int sdx_rotate_tangent_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* rot_dev,
                           double* out, double* out_reference, double* dout_eps, double* dout_eps_reference);
int sdx_rotate_tangent_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                           double limb_darkening, double* out, double* out_reference, double* dout_eps, double* dout_eps_reference);

/* ---- the cell-integrated rotation profile: a second rotation mode, with d / d (v sin i) ----
 * sdx_rotate_dev samples Gray's profile at the grid points.  Here the flux is taken as piecewise linear between the nodes (as
 * sdx_observe_dev's trapezoid assumes) and the profile K(y) = (2 (1 - eps)) sqrt(q) + ((pi / 2) eps) q, q = 1 - y^2, is integrated against
 * it exactly, cell by cell: the operator tends to the identity continuously as V -> 0, a node on the profile's edge contributes a cell of
 * zero length, a linear flux is reproduced at interior points of any grid, and out is differentiable in V.  sdx_rotate_dev is unchanged.
 * For point i, every operation one correctly rounded fp64 operation (atan2: the device library's), in this order (the device functions
 * rot_cell, rot_moments, rot_half), beta = V / c, reach_i = lambdas[i] beta, and every cell g = [j, j + 1]:
 *     y_j = (lambdas[j] - lambdas[i]) / reach_i  (y_i = 0),   c_j = min(max(y_j, -1), 1),   COUNTS(i, g) = c_{j+1} > c_j,
 *     Delta_g = (lambdas[j+1] - lambdas[j]) / reach_i,      d_g = Delta_g where neither end is clamped, else c_{j+1} - c_j,
 *     S0, Q0, S1, Q1 = the integrals of sqrt(q), q, y sqrt(q), y q over [c_j, c_{j+1}]: for 0 <= p < s <= 1 (the other half mirrored), with
 *       u = 1 - y, q = u (1 + y), R = sqrt(q_p) sqrt(q_s), D = d (s + p):
 *       sin = D / (s sqrt(q_p) + p sqrt(q_s)),   cos = p s + R,   dl = atan2(sin, cos),
 *       S0 = ((dl - sin dl) + sin (u_p + u_s p + R)) / 2,  dl - sin dl = dl^3 (1/3! - dl^2 (1/5! - ... 1/25!)),
 *       Q0 = d ((u_p + u_s) - (u_p^2 + u_p u_s + u_s^2) / 3),   S1 = D (q_p + R + q_s) / (3 (sqrt(q_p) + sqrt(q_s))),   Q1 = D (q_p + q_s) / 4
 *       (sums of non-negative terms: each keeps its relative accuracy for a cell of any width, also one that touches +-1),
 *     M0_g = c_sqrt S0 + c_q Q0,   M1_g = c_sqrt S1 + c_q Q1,   r_g = (M1_g - y_j M0_g) / Delta_g,   t_g = M1_g / Delta_g,
 *     den_i = sum_g M0_g,   out[i] = sum_g ((M0_g - r_g) flux[j] + r_g flux[j+1]) / den_i      (W_ij = r_{j-1} + (M0_j - r_j)),
 *     e_0 = y_0 K(y_0) if -1 < y_0 else 0,   e_1 = y_{n-1} K(y_{n-1}) if y_{n-1} < 1 else 0      (a truncated window's end terms; there
 *       1 - |y| = (reach_i - |lambdas[end] - lambdas[i]|) / reach_i, the difference first, and q = (1 - |y|)(1 + |y|)),
 *     dout_lnv[i] = (sum_g t_g (flux[j+1] - flux[j]) + e_0 flux[0] - e_1 flux[n-1] - out[i] (e_0 - e_1)) / den_i = d out[i] / d ln V,
 *     dout_eps[i] = (sum_g ((dM0_g - dr_g) flux[j] + dr_g flux[j+1]) - out[i] sum_g dM0_g) / den_i, dM0, dr: M0, r with c_sqrt = -2, c_q = pi / 2
 * over the cells that count; the *_reference outputs likewise with reference.  dout_lnv is EXACT, not "at fixed windows": written over
 * lambda the domain does not move with V, K(+-1) = 0 removes the boundary terms, and one integration by parts leaves the integral of
 * K y phi_j' with phi_j' piecewise constant; d / dV = dout_lnv / V.  The cells of point i are those of sdx_rotate_dev's window [i0, i1) and
 * the partial cell on each side; a window narrower than one spacing still has three weights.  A window that reaches past an end of the
 * grid is TRUNCATED AND RENORMALISED as sdx_rotate_dev's is.  !(V > 0) is a copy bit for bit, and zeros in the derivative outputs.
 * Mapping, window search, round-robin over the point's 8 or 64 lanes, ascending order and butterfly are sdx_rotate_dev's; no
 * floating-point atomics: two calls, the replay of a captured graph and the host-buffer twin give the same bits.
 * sdx_rotate_integrated_dev: device pointers, asynchronous, no allocation, capturable; rot_dev is sdx_rotate_dev's {V, eps} pair, read
 * when the kernel runs.  The four derivative outputs are optional (all NULL: not formed, the kernel without them runs).  SDX_ERR_ARG
 * before anything is enqueued: n < 2, a null required pointer, reference without out_reference or the reverse, a *_reference derivative
 * without a reference, an output that is one of the inputs or another output.  Contents unchecked as for sdx_rotate_dev: every access
 * stays inside the arrays (a cell index g has 0 <= g < n - 1) and every loop is bounded by its bracket.  Stage name: "k_rotate_integrated". */
int sdx_rotate_integrated_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference,
                              const double* rot_dev, double* out, double* out_reference, double* dout_lnv, double* dout_lnv_reference,
                              double* dout_eps, double* dout_eps_reference);
/* The transpose: a_i = u[i] / den_i, w[j] = sum_i W_ij a_i over the i with lambdas[i] in [lambdas[j-1] / (1 + beta), lambdas[j+1] / (1 -
 * beta)], searched a few 1e-15 wide; rot_cell decides, so the weights are the forward's bit for bit and  sum_i u[i] out[i] = sum_j w[j]
 * flux[j].  nus, scratch, refusals and bounds as sdx_rotate_adjoint_dev.  Stage name:
 * "k_rotate_integrated_adjoint" (two launches: a, the gather). */
int sdx_rotate_integrated_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* rot_dev, const double* u,
                                      const double* u_reference, const double* nus, double* w, double* w_reference);
/* host-buffer twins: lambdas, v_rot and limb_darkening checked as by sdx_rotate_f64 before any copy */
int sdx_rotate_integrated_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                              double limb_darkening, double* out, double* out_reference, double* dout_lnv, double* dout_lnv_reference,
                              double* dout_eps, double* dout_eps_reference);
int sdx_rotate_integrated_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double v_rot, double limb_darkening, const double* u,
                                      const double* u_reference, const double* nus, double* w, double* w_reference);
/* M0 = int K and M1 = int y K over [ya[i], yb[i]] clamped to [-1, 1] for the limb darkening eps[i], point by point, as rot_cell forms them
 * (d = yb - ya rounded once; an empty cell gives zeros; a cell that spans 0 is split there).  For tests.  Stage name: "k_rotate_moments". */
int sdx_rotate_moments_dev(sdx_ctx* ctx, int64_t n, const double* ya, const double* yb, const double* eps, double* out_m0, double* out_m1);
int sdx_rotate_moments_f64(sdx_ctx* ctx, int64_t n, const double* ya, const double* yb, const double* eps, double* out_m0, double* out_m1);

/* ---- disk integration with rigid rotation: per-ring spectra instead of a limb-darkening law ----
 * sdx_rotate_dev and sdx_rotate_integrated_dev apply Gray's profile, i.e. I(mu, lambda) = f(lambda) (1 - eps + eps mu) with one chosen
 * eps.  Here the disk is a set of rings of constant mu, ring r at the projected radius ring_scale[r] = sin theta_r in [0, 1] (b / R for a
 * spherical model) with its OWN spectrum I[r][.] (sdx_emergent_intensity_dev's rows, in any one unit) and the flux weight
 * ring_weights[r].  Along a ring the line-of-sight velocity of a rigid rotator is V ring_scale[r] cos phi with phi uniform, so the ring's
 * average is the convolution of its spectrum with the arcsine density 1 / (pi sqrt(1 - y^2)) of half-width V ring_scale[r] / c.  The
 * spectrum is piecewise linear between the nodes and the density is integrated against it exactly, cell by cell, as
 * sdx_rotate_integrated_dev does with Gray's profile.  lambdas[n] ascending; I [n_rings][I_ld], I_ld >= n.
 * For point i and ring r, every operation one correctly rounded fp64 operation (atan2: the device library's), in this order (the device
 * functions disk_cell, arc_moments, arc_half), beta_r = (V / c) ring_scale[r], reach = lambdas[i] beta_r:
 *     !(reach > 0):  A_r[i] = I[r][i], a copy;   otherwise over every cell g = [j, j + 1] of sdx_rotate_dev's window for that reach and
 *     the partial cell on each side:
 *     y_j = (lambdas[j] - lambdas[i]) / reach  (y_i = 0),   c_j = min(max(y_j, -1), 1),   COUNTS(g) = c_{j+1} > c_j,
 *     Delta_g = (lambdas[j+1] - lambdas[j]) / reach,      d_g = Delta_g where neither end is clamped, else c_{j+1} - c_j,
 *     M0_g, M1_g = the integrals of 1 / (pi sqrt(1 - y^2)) and y / (pi sqrt(1 - y^2)) over [c_j, c_{j+1}]: for 0 <= p < s <= 1 (the
 *       other half mirrored, a cell that spans 0 split there), with q = (1 - y)(1 + y), D = d (s + p):
 *       sin = D / (s sqrt(q_p) + p sqrt(q_s)),   cos = p s + sqrt(q_p) sqrt(q_s),   M0 = atan2(sin, cos) / pi,
 *       M1 = D / (pi (sqrt(q_p) + sqrt(q_s)))      (no difference of asin or of square roots: a cell of any width keeps its accuracy),
 *     r_g = (M1_g - y_j M0_g) / Delta_g,
 *     A_r[i] = sum_g ((M0_g - r_g) I[r][j] + r_g I[r][j+1]) / sum_g M0_g       (ascending g; the two products of a cell in this order),
 *     out[i] = sum_r ring_weights[r] A_r[i]      in the flux's order: two ascending halves over r, the lower added to the upper.
 * out_reference likewise from I_reference (both or neither).  A window truncated at an end of the grid is renormalised by its own sum
 * of M0, as sdx_rotate_dev's is.  Consequences: V = 0 gives the flux sum sum_r w_r I[r][i] in the flux's order bit for bit (fed
 * sdx_emergent_intensity_dev's rows and the field's weights: F_nu[n_depth-1] of the plain kernel, plane-parallel); the result is
 * continuous as V -> 0 (a window under one spacing still has three weights); a spectrum linear in lambda is reproduced at interior
 * points of any grid; a node on a ring's edge closes a cell of zero length.  With I[r] = f (1 - eps + eps mu_r) and rings that
 * resolve s = sin theta in [0, 1] with weight 2 s ds the result tends to sdx_rotate_integrated_dev's.
 * Mapping, window search, round-robin over the point's 8 or 64 lanes, ascending order and butterfly are sdx_rotate_dev's (the mapping
 * chosen by the widest possible ring, ring_scale = 1); a point's lanes take the rings one after the other.  No floating-point atomics:
 * two calls, the replay of a captured graph and the host-buffer twin give the same bits.
 * sdx_disk_integrate_dev: device pointers, asynchronous, no allocation, capturable; rot_dev is sdx_rotate_dev's {V, eps} pair in device
 * memory, of which only V is read, when the kernel runs (a captured call follows a rewritten pair).  SDX_ERR_ARG before anything is
 * enqueued: n < 2, n_rings outside 1 .. 64, a null required pointer, I_reference without out_reference or the reverse, I_ld < n, an
 * output that is one of the inputs or the other output.  Contents unchecked as for sdx_rotate_dev: every access stays inside the arrays
 * (a cell index g has 0 <= g < n - 1, a ring index 0 <= r < n_rings) and every loop is bounded by its bracket.
 * Stage name: "k_disk_integrate". */
int sdx_disk_integrate_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                           const double* ring_weights, const double* I, int64_t I_ld, const double* I_reference, const double* rot_dev,
                           double* out, double* out_reference);
/* host-buffer twin: I and I_reference [n_rings][n] contiguous; additionally refuses, before any copy, lambdas that are not finite and
 * strictly ascending, v_rot that is not finite with 0 <= v_rot < 3000 km/s, and ring_scale outside [0, 1]. */
int sdx_disk_integrate_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                           const double* ring_weights, const double* I, const double* I_reference, double v_rot, double* out,
                           double* out_reference);
/* The same with d out / d ln V from the same pass (the kernel's second instantiation; out and out_reference are sdx_disk_integrate_dev's
 * bit for bit).  The derivative is exact for the discrete operator — the spectrum is piecewise linear and the domain over lambda does
 * not move, so it needs no integration by parts.  With disk_cell's quantities, for ring r, point i, reach > 0:
 *     dnum = sum_g (M1_g / Delta_g) (I[r][j+1] - I[r][j])             (M1_g over the clamped cell; ascending g)
 *            - y_hi K(y_hi) I[r][n-1]   if the window is truncated above,  y_hi = (lambdas[n-1] - lambdas[i]) / reach < 1,
 *            + y_lo K(y_lo) I[r][0]     if it is truncated below,          y_lo = (lambdas[0] - lambdas[i]) / reach > -1,
 *     dden =   - y_hi K(y_hi) + y_lo K(y_lo)   (each under the same condition),     K(y) = 1 / (pi sqrt((1 - y)(1 + y))),
 *     dA_r[i] = (dnum - A_r[i] dden) / den,     dout_lnv[i] = sum_r ring_weights[r] dA_r[i]   in the flux's two-halves order;
 * 1 - |y_end| is formed as (reach - |lambdas[end] - lambdas[i]|) / reach, the difference first.  !(reach > 0) contributes 0, !(V > 0)
 * gives zeros.  Per km/s: dout_lnv / V.  K is singular at the ring's edge: a truncated window whose end node lies within 1e-5 of the
 * edge (1 - |y_end| < 1e-5) is OUTSIDE the derivative's contract — the term is finite but grows as the inverse square root of that
 * distance, and the operator itself has a square-root kink in V there.
 * dout_lnv is required, dout_lnv_reference optional and needs I_reference; otherwise sdx_disk_integrate_dev's refusals, the four outputs
 * distinct buffers.  Stage name: "k_disk_integrate". */
int sdx_disk_integrate_deriv_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                 const double* ring_weights, const double* I, int64_t I_ld, const double* I_reference,
                                 const double* rot_dev, double* out, double* out_reference, double* dout_lnv,
                                 double* dout_lnv_reference);
int sdx_disk_integrate_deriv_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                 const double* ring_weights, const double* I, const double* I_reference, double v_rot, double* out,
                                 double* out_reference, double* dout_lnv, double* dout_lnv_reference);
/* The transpose of sdx_disk_integrate_dev.  The cotangent of a disk-integrated spectrum is not a vector over the grid but a plane over
 * (ring, node), because each ring's spectrum is convolved with its own kernel: for weights u[n] over the broadened points,
 *     W[r][j] = ring_weights[r] sum_i (u_i / den_r(i)) (weight of node j in point i's row for ring r),
 * the node weight being (M0_g - r_g) of cell [j, j + 1] plus r_g' of cell [j - 1, j], with disk_cell deciding: the forward's weights bit
 * for bit, den_r(i) in the forward's order, so that sum_i u_i out_i = sum_r sum_j W[r][j] I[r][j] up to the rounding of the sums.  A
 * ring with !(reach > 0) passes ring_weights[r] u_j through (V = 0: W[r][j] = ring_weights[r] u_j exactly).  It is the broadening
 * stages' pair of launches (sdx_rotate_integrated_adjoint_dev), one ring per row of the launch: a_r[i] = u_i / den_r(i) into the context's
 * stage scratch (2 n_rings rows, sdx_rotate_adjoint_dev's convention: grown at the first call of a size, so warm a call before capturing
 * it), then per node the gather over the candidates lambdas[i] in [lambdas[j-1] / (1 + beta_r), lambdas[j+1] / (1 - beta_r)], round-robin
 * in ascending i and closed by the butterfly.  nus (optional): W[r][j] is further multiplied by nus[j] / lambdas[j], the transpose of
 * sdx_flux_nu_to_lambda_dev per ring — the rows then apply to I_nu instead of I_lambda, as sdx_rotate_integrated_adjoint_dev treats nus.
 * W [n_rings][W_ld]; W_reference likewise from u_reference (both or neither).  No floating-point atomics.  SDX_ERR_ARG before anything is
 * enqueued: as for sdx_disk_integrate_dev, and W_ld < n, a reference output without its input or the reverse, an output that is one of
 * the inputs or the other output.  Stage name: "k_disk_integrate_adjoint". */
int sdx_disk_integrate_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                   const double* ring_weights, const double* rot_dev, const double* u, const double* u_reference,
                                   const double* nus, double* W, int64_t W_ld, double* W_reference);
/* host-buffer twin: W and W_reference [n_rings][n] contiguous; the host checks of sdx_disk_integrate_f64. */
int sdx_disk_integrate_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                   const double* ring_weights, double v_rot, const double* u, const double* u_reference,
                                   const double* nus, double* W, double* W_reference);

/* Everything in one call for resident data: pre-pass + line opacity + total (above) + raytrace (F_nu
 * overwritten).  F_nu is [n_depth][ld].  alpha_line_out and total_alphas ([n_depth][ld]) are OPTIONAL outputs (NULL: the
 * plane is never written to HBM — the reference only reads them back through opacities_dict / Opacities.total_alphas;
 * the formal solution forms total = continuum + line while staging its columns).  This is the step bench.py times. */
int sdx_synthesize_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                       int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                       int gamma_cols, const double* alphas, const sdx_continuum* cont, int n_theta,
                       const double* temperature, const double* ray_dist, const double* theta_weights,
                       double* alpha_line_out, double* total_alphas, double* F_nu, int64_t ld,
                       int64_t* n_evaluations_dev);
/* The same step with the two optional extras of RadiationField (radiation_field/base.py:38-68).  source: the caller's source
 * function already evaluated, [n_depth][source_ld] with column 0 = column nu_begin (RadiationField.source_function is any callable
 * (nu, T) -> (N_d, N_nu), radiation_field_solvers/base.py:133; NULL: the Planck function, evaluated by the kernel).  I_nus:
 * track_individual_intensities (:64-68, filled at radiation_field_solvers/base.py:324-338), [n_depth][nu_count][n_theta] receives
 * the intensity of every ray at every depth point (row 0: zeros, the reference's initial condition :134); NULL: not kept. */
int sdx_synthesize_ex_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                          int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                          int gamma_cols, const double* alphas, const sdx_continuum* cont, int n_theta,
                          const double* temperatures, const double* ray_dist, const double* weights, double* alpha_line_out,
                          double* total_alphas, double* F_nu, int64_t ld, const double* source, int64_t source_ld, double* I_nus,
                          int64_t* n_evaluations_dev);

/* The same synthesis for a caller whose data lives in host memory (plain C, or numpy through ctypes): every pointer,
 * including those inside `cont`, is a HOST pointer; arrays are uploaded, sdx_synthesize_dev runs, results come back.
 * F_nu is [n_depth][n_nu] (overwritten); alpha_line_out, total_alphas ([n_depth][n_nu]) and n_evaluations are optional.
 * ray_dist is the (n_depth-1, n_theta) table dist[:, None] / cos(theta) (radiation_field_solvers/base.py:302-305). */
int sdx_synthesize_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                       const double* doppler_widths, const double* gammas, int gamma_cols, const double* alphas,
                       const sdx_continuum* cont, int n_theta, const double* temperature, const double* ray_dist,
                       const double* theta_weights, double* alpha_line_out, double* total_alphas, double* F_nu,
                       int64_t* n_evaluations);

/* ---- fp32-mixed twins of the host-buffer entry points (`*_f32mix`) ---------------------------
 * The same signatures and semantics as sdx_line_opacity_f64 / sdx_raytrace_f64 / sdx_synthesize_f64 with the context's
 * "mixed_precision" option on for the duration of the call (and restored afterwards, whatever it was): the tolerance path of BASELINE
 * configs[4] — far wings, window edges and narrow windows in packed fp32, the formal solution of plane-parallel grids in fp32; the
 * pre-pass, the continuum and kept line cores in fp64; stated tolerance 1e-4 on the flux against the fp64 path (measured 1e-6).  The
 * device-pointer entry points (*_dev) take the option instead: sdx_set_int_option(ctx, "mixed_precision", 1).  The reference has no
 * counterpart (its arithmetic is fp64 throughout, opacities_solvers/base.py:487-627, radiation_field_solvers/base.py:85-346). */
int sdx_line_opacity_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines,
                            const double* line_nus, const double* doppler_widths, const double* gammas, int gamma_cols,
                            const double* alphas, double* out, int64_t* n_evaluations);
int sdx_raytrace_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus,
                        const double* temperature, const double* ray_dist, const double* theta_weights,
                        const double* total_alphas, double* F_nu, double* I_nus);
int sdx_synthesize_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                          const double* doppler_widths, const double* gammas, int gamma_cols, const double* alphas,
                          const sdx_continuum* cont, int n_theta, const double* temperature, const double* ray_dist,
                          const double* theta_weights, double* alpha_line_out, double* total_alphas, double* F_nu,
                          int64_t* n_evaluations);

/* ---- one process, several GPUs ---------------------------------------------------
 * The frequency axis shards with no data-path exchange: every output column depends only on its own frequency
 * (radiation_field_solvers/base.py:200 is a prange over nu; calc_alan_entries :548-590 is a pure gather per (depth, nu)).
 * A group is one context + one stream per device and ONE RCCL communicator over them (ncclCommInitAll).
 * sdx_synthesize_sharded_f64 = sdx_synthesize_f64 with the columns split over the group's devices: the line list is
 * replicated, every device applies the window rule on the GLOBAL grid (global d_nu, centres, clamp — results equal the
 * single-GPU call bit for bit), and ONE ncclAllGather of the zero-padded F_nu[-1] shards (8 * max shard width bytes per
 * rank, over xGMI) leaves the emergent spectrum on every device; it is returned from device 0.
 *   devices      NULL = devices 0 .. n_gpus-1; each device at most once.
 *   shard_begin  NULL = equal blocks of ceil(n_nu / n_gpus) columns; else [n_gpus + 1] ascending column indices from 0 to n_nu
 *                (e.g. shards of equal estimated work).
 *   outputs      all host, all optional except that one of F_nu / emergent_flux must be given: alpha_line_out, total_alphas,
 *                F_nu are [n_depth][n_nu] (each device fills the columns it owns), emergent_flux [n_nu] = the gathered F_nu[-1].
 * RCCL is opened at run time (librccl.so.1; env SDX_RCCL_LIB overrides the path); any RCCL failure returns SDX_ERR_COMM.
 * Test hook: with SDX_EXPERIMENT=1 and SDX_GROUP_LOOPBACK=1 in the environment a group may list one device several times and the gather is done
 * with plain device copies instead of RCCL (RCCL refuses two ranks on one GPU) — for exercising the sharding logic on a
 * one-GPU box, never a product mode. */
typedef struct sdx_group sdx_group;
sdx_group* sdx_group_create(int n_gpus, const int* devices); /* NULL on error: sdx_last_error_code / _string */
void sdx_group_destroy(sdx_group* group);
int sdx_group_size(const sdx_group* group);
sdx_ctx* sdx_group_context(sdx_group* group, int rank); /* the rank's context (options, profiling); owned by the group */
/* what the last sharded call's collective was: ranks in the communicator, bytes each rank contributed, RCCL's version code
 * (0 in loop-back mode) */
int sdx_group_last_gather(const sdx_group* group, int* ranks, int64_t* bytes_per_rank, int* rccl_version);
/* n_evaluations (optional): the number of Voigt evaluations of the whole synthesis — a global figure, counted by the first rank
 * that owns columns.  Counting needs every window of every line, so that rank runs the full (unculled) pre-pass and becomes the
 * straggler of the group: a diagnostic, pass NULL in timed loops. */
int sdx_synthesize_sharded_f64(sdx_group* group, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines,
                               const double* line_nus, const double* doppler_widths, const double* gammas, int gamma_cols,
                               const double* alphas, const sdx_continuum* cont, int n_theta, const double* temperature,
                               const double* ray_dist, const double* theta_weights, const int64_t* shard_begin,
                               double* alpha_line_out, double* total_alphas, double* F_nu, double* emergent_flux,
                               int64_t* n_evaluations);

/* ---- line parameters generated on the device ---------------------------------------
 * Instead of the three dense (N_l, N_d) tables the reference builds on the host before calc_alan_entries —
 * alpha_line (plasma/base.py:178-321 AlphaLineVald, :324-455 AlphaLineShortlistVald; plasma/molecules.py:192-320,
 * :322-440 the molecular twins), gammas and doppler_widths (opacities_solvers/broadening.py:659-732
 * calculate_broadening, :735-821 calculate_molecule_broadening, :1009-1085 calc_vald_gamma) — the caller passes
 * ~80 B of per-line scalars plus per-depth state, and the pre-pass evaluates the three values per (line, depth) itself.
 * Lines are sorted by ascending nu and already restricted to the grid's range, exactly as
 * calc_alpha_line_at_nu prepares them (opacities_solvers/base.py:392-421).  All pointers are device pointers.
 *   alpha = ((alpha_coefficient * ((exp(-e_low/(k T)) * pop[pop_row]) [* g_lo])) * strength) * (1 - exp(-h nu/(k T)))
 * gamma_mode: 0 = calc_gamma (broadening.py:550-656), 1 = calc_vald_gamma (:1009-1085), 2 = A_ul only, one column
 * (molecules, :799-801), 3 = zero.  broadening_flags: 1 linear Stark | 2 quadratic Stark | 4 van der Waals | 8 radiation.
 * ion_number is the charge seen by the outer electron (`ion_number + 1`, broadening.py:708-709).
 * mass and temperature must be positive and finite at every line and depth: the arrays live on the device, so the library
 * cannot look at them, and the generated Doppler width forms 2 k T / m from the reciprocal of the mass without the
 * division's handling of a zero or infinite quotient.  The caller checks them (the Python LineList refuses mass <= 0). */
typedef struct sdx_linelist {
    int64_t n_lines;
    const double* nu;          /* [n_lines] Hz, ascending */
    const double* e_low_ev;    /* [n_lines] lower level energy, eV */
    const double* g_lo;        /* [n_lines] 2 j_lo + 1; NULL for short lists */
    const double* strength;    /* [n_lines] f_lu = 10**log_gf / g_lo, or 10**log_gf for short lists */
    const int32_t* pop_row;    /* [n_lines] row of pop for the line's ion or molecule */
    const double* pop;         /* [n_pop_rows][n_depth] number density / partition function */
    int n_pop_rows;
    double alpha_coefficient;  /* pi e^2 / (m_e c), cgs */
    const double* mass;        /* [n_lines] g */
    double microturbulence;    /* cm/s */
    int gamma_mode;
    int broadening_flags;
    const int32_t* atomic_number;
    const int32_t* ion_number;
    const double* ionization_energy; /* erg */
    const double* upper_energy;      /* erg */
    const double* lower_energy;      /* erg */
    const double* A_ul;
    const double* stark;       /* VALD log Stark parameter (gamma_mode 1) */
    const double* waals;       /* VALD van der Waals parameter (gamma_mode 1) */
    const double* temperature;       /* [n_depth] K */
    const double* electron_density;  /* [n_depth] cm^-3 */
    const double* h_density;         /* [n_depth] neutral hydrogen, cm^-3 */
} sdx_linelist;

/* The reference's dense tables from a line list (parity checks; any output may be NULL).  gammas is
 * [n_lines][n_depth], or [n_lines][1] for gamma_mode 2 and 3. */
int sdx_line_params_dev(sdx_ctx* ctx, int n_depth, const sdx_linelist* lines, double* alphas, double* gammas,
                        double* doppler_widths);

/* AlphaLine.calculate (plasma/base.py:146-175), lines from TARDIS atomic data: alphas[l][d] =
 * ((alpha_coefficient * level_density[lower_index[l]][d]) * stim[l][d]) * f_lu[l].  level_density is
 * [n_levels][n_depth]; stim (the stimulated-emission factor TARDIS supplies) and alphas are [n_lines][n_depth].
 * lower_index must lie in [0, n_levels) (numpy take(mode="raise") on the host side). */
int sdx_alpha_line_levels_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, int n_levels, const double* level_density,
                              const int32_t* lower_index, const double* stim, const double* f_lu,
                              double alpha_coefficient, double* alphas);

/* The fused step with everything optional a RadiationField configuration can ask for, in one description (the entry point the
 * drop-in create_stellar_radiation_field binds for the configurations sdx_synthesize_dev / _ex_dev do not cover):
 *   source / I_nus       as in sdx_synthesize_ex_dev;
 *   inward_rays          spherical models (radiation_field_solvers/base.py:141-198, :296-300, :340-344): ray_dist is the chord table
 *                        of calculate_spherical_ray (:349-381), the surface-to-centre sweep runs before the outward one and
 *                        F_nu is finally scaled by photospheric_correction = (r[-1] / reference_r)^2;
 *   line_plane[]         further line-opacity planes the caller has formed on the device ([n_depth][line_plane_ld], column 0 =
 *                        column nu_begin; sdx_line_opacity_dev / _linelist_dev): the molecular list of include_molecules
 *                        (opacities_solvers/base.py:444-484, :716-736), added AFTER the step's own line opacity in this order —
 *                        total = ((continuum + line) + plane 0) + plane 1, what Opacities.calc_total_alphas does with the
 *                        dictionary entries (opacities/base.py:24-28);
 *   linelist             when set, the step's own lines come as per-line scalars (f1, below) and the dense arrays
 *                        (line_nus ... alphas, n_lines) are ignored;
 *   F_nu_continuum       when set, the continuum flux [n_depth][continuum_ld] (column 0 = column nu_begin) is traced with F_nu
 *                        (beside it in k_raytrace_cont; on the small grids of the segmented kernel by a second launch of it on the
 *                        continuum plane): the formal solution of the continuum plane alone, with the same angles, source function
 *                        and geometry (inward_rays, photospheric_correction).  The step's lines, linelist and line_plane[] are
 *                        excluded; it is F_nu of the same step with no lines and no line planes, bit for bit, on every kernel the
 *                        option "segmented_raytrace" selects, and on frequency shards.  F_nu, total_alphas, alpha_line_out and I_nus
 *                        (still the total intensity) are unchanged by it.  Works with source, I_nus, inward_rays, line_plane[],
 *                        linelist and line_m_max (the synthesis after the classification in the two-collective mode, step 3 below).  SDX_ERR_ARG (-1) with "mixed_precision" = 1,
 *                        or where the step cannot fuse the total into the formal solution (n_theta > 64, models whose columns do
 *                        not fit LDS).
 *   grid_plan            when set, a plan built for this grid, line list and cross-section table (sdx_grid_plan_create, below): the
 *                        pre-pass launch reads what depends on them alone from the plan instead of forming it again.  Bit-identical
 *                        results.  A plan whose recorded pointers or sizes differ from this call's is SDX_ERR_ARG before anything is
 *                        enqueued.
 * A zero-initialised description is sdx_synthesize_dev, bit for bit; `options` itself must not be NULL (-1). */
typedef struct sdx_grid_plan sdx_grid_plan;
typedef struct sdx_synthesis_options {
    const double* source;
    int64_t source_ld;
    double* I_nus;
    int inward_rays;
    double photospheric_correction;
    int n_line_planes; /* 0 .. 2 */
    const double* line_plane[2];
    int64_t line_plane_ld;
    const sdx_linelist* linelist;
    const double* line_m_max; /* two-collective mode (below): the gathered per-line maxima [n_lines], or NULL */
    const sdx_grid_plan* grid_plan; /* or NULL */
    double* F_nu_continuum;   /* [n_depth][continuum_ld] continuum flux, or NULL (no continuum chain) */
    int64_t continuum_ld;
} sdx_synthesis_options;

/* ---- grid plan: the grid-only work of the fused step, once per grid instead of once per step -----------------------------------
 * The pre-pass launch of a step begins with work that reads nothing but the frequency grid, the line frequencies and the tabulated
 * cross-section: the grid spacing d_nu (opacities_solvers/base.py:524-526) and 1 / d_nu, every line's centre index (:556-558),
 * the number of lines centred at or beyond each grid index, and per frequency the interpolated cross-section (util.py:94-103),
 * nu^-3 and the Rayleigh powers (nu / (2 c R))^4,6,8.  A synthesis that is stepped many times on one grid and one list — a fit,
 * a model grid: line STRENGTHS, widths, dampings, temperatures and densities change from step to step, the grid and the list do
 * not — forms them once:
 *   sdx_grid_plan_create   allocates the plan's device arrays from the context's block pool and enqueues ONE launch
 *                          (k_grid_plan_build) on the context's stream that fills them with the step's own device functions and
 *                          operations: the values are the step's, bit for bit.  cont may be NULL (no table).  No host round trip;
 *                          the allocation makes it unfit for stream capture, the other two calls are capturable.
 *   sdx_grid_plan_refresh  the same launch again — after the caller has changed the VALUES of the arrays in place.
 *   sdx_grid_plan_destroy  returns the arrays to the pool (uses are ordered on the context's stream).
 * Contract: the plan records the pointers and sizes it was built from (nus, n_nu, line_nus, n_lines, cont->lambdas,
 * cont->table_wavelength, cont->table_sigma, cont->n_table).  While a plan is in use the VALUES of nus, line_nus, lambdas, the
 * table's axis and the table must not change, short of a refresh.  Everything per depth (temperatures, every density, ray
 * distances), the bound-free edges and the lines' doppler_widths, gammas and alphas may change freely: none of it is in the plan.
 * Honoured by sdx_synthesize_opt_dev on the un-culled pre-pass of a dense line list next to the tiled continuum (at most 4096
 * bound-free levels): whole grids and frequency shards of lists below "indexed_min_lines", whole grids of longer ones.  IGNORED
 * (after the check of its pointers and sizes) by culled shards and the two-collective mode (line_m_max) and where the context
 * option "grid_plan" is 0; ignored unchecked with a line list given as scalars (options->linelist: the generating pre-pass has no
 * planned form).  On grids of more than 16384 points the planned step also drops the grid-spacing launch unless the far field
 * needs its tile ranges.  A recorded hipGraph holds the plan's device pointers: destroy the graph before the plan. */
int sdx_grid_plan_create(sdx_ctx* ctx, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                         const sdx_continuum* cont_or_null, sdx_grid_plan** out);
int sdx_grid_plan_refresh(sdx_grid_plan* plan);
void sdx_grid_plan_destroy(sdx_grid_plan* plan);
int sdx_synthesize_opt_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                           int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                           int gamma_cols, const double* alphas, const sdx_continuum* cont, int n_theta,
                           const double* temperatures, const double* ray_dist, const double* weights, double* alpha_line_out,
                           double* total_alphas, double* F_nu, int64_t ld, const sdx_synthesis_options* options,
                           int64_t* n_evaluations_dev);

/* Frequency shards of long lists in TWO collectives (optional; SURVEY §8e plans one).  A shard's step begins by classifying EVERY
 * line of the replicated list — the largest (gamma + doppler_width) alpha over the depths, from which the window rule
 * (opacities_solvers/base.py:561-575) gives the line's widest window: which lines can reach the shard from anywhere — a stream of
 * 8 n_lines (2 n_depth + gamma_cols) bytes that every rank repeats and that does not shrink with the number of ranks.  Here each
 * rank classifies a SHARE of the lines and the ranks exchange the shares (an all-gather of 8 n_lines bytes):
 *   1. sdx_synthesize_classify_dev(...)       m_max[line_begin .. line_begin + line_count) = this rank's share; the same launch
 *                                             leaves the grid spacing, the shard's line ranges and the continuum plane of the step
 *                                             in the context's scratch;
 *   2. the caller gathers m_max [n_lines]      (RCCL / torch.distributed; stardis_amd.parallel.ClassificationGatherer);
 *   3. sdx_synthesize_opt_dev(..., options->line_m_max = m_max)   the rest of the step — same context, same grid, shard, lists.
 * Results are bit-identical to the one-call step (the classes of the lines follow from the same numbers).  Only for culled
 * shards: dense lists of >= `indexed_min_lines` lines, grids of more than 16384 points, nu_count < n_nu, no evaluation count;
 * anything else is SDX_ERR_ARG (-1), as is step 3 without step 1.  What step 1 leaves in the scratch belongs to ONE step 3: it is
 * consumed by it, and invalidated by any other call on the context that prepares lines or a continuum plane in between (a second
 * step 3, a synthesis of another problem, sdx_line_opacity_dev ...: SDX_ERR_ARG instead of another problem's data).  A recorded
 * hipGraph replays steps 1 and 3 without these host-side checks: replay them in pairs.  The "far_field" option may differ between
 * the steps (step 3 computes the tiles' far ranges itself when step 1 has not). */
int sdx_synthesize_classify_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                                int64_t n_lines, const double* line_nus, const double* doppler_widths, const double* gammas,
                                int gamma_cols, const double* alphas, const sdx_continuum* cont, int64_t line_begin,
                                int64_t line_count, double* m_max);

/* sdx_line_opacity_dev / sdx_synthesize_dev with the line parameters generated in the pre-pass. */
int sdx_line_opacity_linelist_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin,
                                  int64_t nu_count, const sdx_linelist* lines, double* out, int64_t out_ld, int accumulate,
                                  int64_t* n_evaluations_dev);
int sdx_synthesize_linelist_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin,
                                int64_t nu_count, const sdx_linelist* lines, const sdx_continuum* cont, int n_theta,
                                const double* temperature, const double* ray_dist, const double* theta_weights,
                                double* alpha_line_out, double* total_alphas, double* F_nu, int64_t ld,
                                int64_t* n_evaluations_dev);

#ifdef __cplusplus
}
#endif
#endif /* STARDIS_HIP_H */
