"""Every kernel of the formal solution against the 80-bit evaluation of the reference's formulas, on hostile columns
(tests/formal_solution_truth.py): waves that sit in one regime of the weights or straddle 5e-4 or 50, transparent layers under, inside
and on top of opaque ones (where the reference divides by zero: the same NaN pattern), and optical depths at both ends of the double
range, where the step's common denominator t0 t1 (t0 + t1) is subnormal, zero or infinite (the rare-lane path).

Criterion (fp64 kernels), per class of columns: the kernel is no further from the truth than 4 x the oracle's own distance
+ 4e-15 per gap, flux and tracked intensities alike; its NaN pattern is the oracle's; no infinity where the oracle has none;
transparent columns are exactly 0 and F[0] == 0.  `underflow` carries no bound (the double-precision reference is meaningless there:
w2 is subnormal) — pattern, finiteness and zeros only.  tests/test_formal_solution_truth_cpu.py checks what this rests on.
The launch label of every case is asserted; the measured distances go to formal_solution_truth.RECORD
(scripts/formal_truth_table.py -> profiles/formal_truth_classes.json)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import contribution_reference as cref
import formal_solution_truth as T
from stardis_amd import _lib, ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu

GENERAL, STEP, LANE, CONT, BASIC, F32 = "k_raytrace_seg<8,7>", "k_raytrace_seg_step<8,7>", "k_raytrace<1>", "k_raytrace_cont<1>", "k_raytrace_basic", "k_raytrace_f32"
PLANE = [(2, 3), (3, 7), (9, 20), (55, 1), (56, 20), (57, 64)]
SPHERICAL = [(9, 20), (56, 20), (40, 7)]
FUSED = [(9, 20), (55, 1), (56, 20)]
STAND_ALONE = {1: GENERAL, 0: LANE}  # context option "segmented_raytrace" -> the kernel behind ops.raytrace_arrays at the shapes of PLANE


@pytest.fixture(autouse=True)
def extended_precision():
    if not T.EXTENDED:
        pytest.skip("no extended-precision long double on this host")


@contextlib.contextmanager
def launching(ctx, segmented_raytrace=-1, far_field=-1, mixed_precision=0):
    """the three context options for the launches inside, profiled (for the launch label); restored afterwards"""
    ctx.set_option("segmented_raytrace", segmented_raytrace)
    ctx.set_option("far_field", far_field)
    ctx.set_option("mixed_precision", mixed_precision)
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    try:
        yield
    finally:
        ctx.call("sdx_profile_enable", 0)
        ctx.set_option("segmented_raytrace", -1)
        ctx.set_option("far_field", -1)
        ctx.set_option("mixed_precision", 0)


def judge(c, label, quantity, a, truth, oracle_values, keep=None):
    """the criterion above for one output of one launch"""
    a = np.asarray(a)
    assert a.shape == oracle_values.shape, (label, quantity)
    assert np.array_equal(np.isnan(a), np.isnan(oracle_values)), (label, quantity, "NaN pattern")
    assert not np.isinf(a[~np.isinf(oracle_values)]).any(), (label, quantity, "inf")
    figures = T.per_class(c, a, truth, oracle_values, reduce_angles=a.ndim == 3, keep=keep)
    missed = []
    for name, (d_gpu, d_oracle) in figures.items():
        T.RECORD.append((label, quantity, "spherical" if c.spherical else "plane", c.n_depth, c.n_theta, c.order, name, d_gpu, d_oracle))
        print(f"{label} {quantity} {c.n_depth}/{c.n_theta} {c.order} {name}: kernel {d_gpu:.2e} oracle {d_oracle:.2e}")
        if name != "underflow" and not d_gpu <= T.bound(d_oracle, c.n_depth):
            missed.append((name, d_gpu, d_oracle))
    assert not missed, (label, quantity, c.n_depth, c.n_theta, c.order, missed)


def zeros(c, F, F0=None):
    """transparent columns are exactly 0 (with a caller's flux: exactly that flux), and so is the first row"""
    base = np.zeros_like(F) if F0 is None else F0
    if "transparent" in c.classes:
        cols = c.columns("transparent")
        assert np.array_equal(F[:, cols], base[:, cols])
    if not c.spherical:
        assert np.array_equal(F[0], base[0])


def trace(ctx, c, option, expect, nus=None, alphas=None, **kw):
    with launching(ctx, segmented_raytrace=option):
        F, I = ops.raytrace_arrays(c.nus if nus is None else nus, c.temps, c.ray, c.weights, c.alphas if alphas is None else alphas, track=True,
                                   ctx=ctx, inward_rays=c.spherical, photospheric_correction=c.correction if c.spherical else 1.0, **kw)
        label = ctx.profile_variant("k_raytrace")
    assert label == expect, (label, expect)
    return F, I


def stand_alone(ctx, c, option, expect):
    ref = c.reference()
    F, I = trace(ctx, c, option, expect)
    judge(c, expect, "F", F, ref["Ft"], ref["Fo"])
    judge(c, expect, "I", I, ref["It"], ref["Io"])
    zeros(c, F)
    if "transparent" in c.classes:
        assert not I[:, c.columns("transparent")].any()
    return F, I


# ---- the stand-alone entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", [1, 0])
@pytest.mark.parametrize("order", ["grouped", "interleaved"])
@pytest.mark.parametrize("n_depth,n_theta", PLANE)
def test_stand_alone(ctx, n_depth, n_theta, order, option):
    stand_alone(ctx, T.case(n_depth, n_theta, 16, order), option, STAND_ALONE[option])


@pytest.mark.parametrize("option", [1, 0])
@pytest.mark.parametrize("name", ["thin", "thick"])
@pytest.mark.parametrize("n_depth,n_theta", [(55, 1), (56, 20)])
def test_whole_launch_in_one_regime(ctx, n_depth, n_theta, name, option):
    stand_alone(ctx, T.case(n_depth, n_theta, 130, "grouped", (name,)), option, STAND_ALONE[option])


@pytest.mark.parametrize("n_depth,n_theta", PLANE)
def test_accumulate(ctx, n_depth, n_theta):
    """a caller's F_nu is added to (radiation_field_solvers/base.py:336): k_raytrace<1> whatever the option; the truth is F0 + F"""
    c = T.case(n_depth, n_theta)
    ref = c.reference()
    rng = np.random.default_rng(7)
    scale = np.nanmax(np.abs(np.where(np.isfinite(ref["Fo"]), ref["Fo"], 0.0)), axis=0)  # of each column's own size: the sum keeps both
    F0 = rng.uniform(0.5, 1.5, ref["Fo"].shape) * np.where(scale > 0, scale, 1e-5)
    Fo, _ = c.oracle(F_nu=F0.copy())
    F, I = trace(ctx, c, 1, LANE, F_nu=F0)
    judge(c, LANE + " (accumulate)", "F", F, ref["Ft"] + F0, Fo)
    judge(c, LANE + " (accumulate)", "I", I, ref["It"], ref["Io"])
    zeros(c, F, F0)


def test_deep_model(ctx):
    """985 depth points: the columns do not fit LDS, every lane recomputes its own (k_raytrace_basic)"""
    stand_alone(ctx, T.case(985, 20, 2), -1, BASIC)


@pytest.mark.parametrize("n_depth,n_theta", SPHERICAL)
def test_spherical(ctx, n_depth, n_theta):
    """the inward sweep first (its index wrap included), chords that miss the inner shells, the photospheric correction"""
    stand_alone(ctx, T.case(n_depth, n_theta, 16, "grouped", T.CLASSES, True), 1, LANE)


def independent(ctx, c, option, expect):
    perm = np.random.default_rng(11).permutation(c.n_nu)
    F, I = trace(ctx, c, option, expect)
    Fp, Ip = trace(ctx, c, option, expect, nus=np.ascontiguousarray(c.nus[perm]), alphas=np.ascontiguousarray(c.alphas[:, perm]))
    assert np.array_equal(Fp, F[:, perm], equal_nan=True), int((Fp != F[:, perm]).sum())
    assert np.array_equal(Ip, I[:, perm], equal_nan=True)


@pytest.mark.parametrize("option", [1, 0])
@pytest.mark.parametrize("n_depth,n_theta", PLANE)
def test_columns_are_independent(ctx, n_depth, n_theta, option):
    """permuting the columns (with their frequencies) permutes F and I bit for bit: a lane's value does not depend on the branch its
    wave took (the exponential form is skipped when every lane of a wave takes the series; a wave of the segmented kernels with a
    flagged lane walks its segment again, and only the flagged lanes may take the reference's form there)"""
    independent(ctx, T.case(n_depth, n_theta), option, STAND_ALONE[option])


def test_columns_are_independent_deep_and_spherical(ctx):
    independent(ctx, T.case(985, 20, 2), -1, BASIC)
    independent(ctx, T.case(40, 7, 16, "grouped", T.CLASSES, True), 1, LANE)


# ---- the fused shape: the hostile plane as the step's whole continuum ------------------------------------------------------------------
def lines_for(c, n_lines):
    if not n_lines:
        return dict(line_nus=np.zeros(0), doppler_widths=np.zeros((0, c.n_depth)), gammas=np.zeros((0, c.n_depth)), alphas=np.zeros((0, c.n_depth)))
    atm = dict(temperatures=c.temps, n_e=np.geomspace(1e15, 1e11, c.n_depth), microturbulence=1.0e5)
    return synth.synth_lines(c.nus, atm, n_lines, seed=3)


def step(ctx, c, option, n_lines=0, far_field=0, keep_total=True, keep_continuum_flux=False):
    """one fused step whose continuum is exactly the hostile plane (a finished file plane, no other source) -> (outputs, label)"""
    syn = SpectralSynthesizer(c.nus, c.temps, c.dist, c.thetas, c.weights, lines_for(c, n_lines), None, ctx=ctx, keep_line=False,
                              track_evaluations=False, keep_total=keep_total, keep_continuum_flux=keep_continuum_flux)
    plane = ctx.upload(c.alphas)
    syn.cont.n_file_planes, syn.cont.file_plane_ld = 1, c.n_nu
    syn.cont.file_plane[0] = plane.ptr
    with launching(ctx, segmented_raytrace=option, far_field=far_field):
        if c.spherical:  # the chord table and the two spherical options through the entry point the engine's step uses
            assert keep_continuum_flux
            ray = ctx.upload(c.ray)
            opt = _lib.SynthesisOptions()
            opt.F_nu_continuum, opt.continuum_ld = syn.d_Fc.ptr, c.n_nu
            opt.inward_rays, opt.photospheric_correction = 1, float(c.correction)
            ctx.call("sdx_synthesize_opt_dev", syn.n_depth, syn.n_nu, syn.d_nus.ptr, 0, syn.count, syn.n_lines, syn.d_ln.ptr, syn.d_dw.ptr,
                     syn.d_g.ptr, syn.gamma_cols, syn.d_a.ptr, C.byref(syn.cont), syn.n_theta, syn.d_t.ptr, ray.ptr, syn.d_w.ptr, None,
                     syn.d_total.ptr if keep_total else None, syn.flux_ptr, syn.count, C.byref(opt), None)
        else:
            syn.step()
        ctx.synchronize()
        label = ctx.profile_variant("k_raytrace")
        if n_lines:
            assert ctx.lib.sdx_far_field_active(ctx.handle, c.n_nu) == far_field  # (two line planes without the far field, three with it)
    out = {"F": syn.F_nu().copy()}
    if keep_total:
        out["total"] = syn.total_alphas().copy()
    if keep_continuum_flux:
        out["Fc"] = syn.F_nu_continuum.copy()
    syn.close()
    del plane
    return out, label


def judge_step(c, label, out):
    """F_nu against the truth traced from the step's own total_alphas (checked against the oracle elsewhere), the continuum flux
    against the truth of the hostile plane itself"""
    ref = c.reference()
    if np.array_equal(out["total"], c.alphas):
        Ft, Fo, keep = ref["Ft"], ref["Fo"], None
        zeros(c, out["F"])
    else:
        (Ft, _), (Fo, _) = c.truth(out["total"]), c.oracle(out["total"])
        keep = ~T.near_threshold(out["total"], c.ray)  # (a total that lands on a threshold of the weights is not comparable)
        assert keep.sum() >= 0.99 * keep.size  # (a tau within 1e-9 of a threshold is a one-in-a-million event per gap and angle)
    judge(c, label, "F", out["F"], Ft, Fo, keep)
    if "Fc" in out:
        judge(c, label, "F continuum", out["Fc"], ref["Ft"], ref["Fo"])
        zeros(c, out["Fc"])


@pytest.mark.parametrize("n_lines,far_field", [(0, 0), (60, 0), (60, 1)], ids=["0 planes", "2 planes", "3 planes"])
@pytest.mark.parametrize("n_depth,n_theta", FUSED)
def test_step_kernel(ctx, n_depth, n_theta, n_lines, far_field):
    c = T.case(n_depth, n_theta)
    kept, label = step(ctx, c, 2, n_lines, far_field)
    assert label == STEP
    if n_lines:
        assert not np.array_equal(kept["total"], c.alphas)
    else:
        assert np.array_equal(kept["total"], c.alphas)  # the continuum is exactly the plane
    judge_step(c, STEP, kept)
    bare, label = step(ctx, c, 2, n_lines, far_field, keep_total=False)
    assert label == STEP and np.array_equal(bare["F"], kept["F"], equal_nan=True)
    both, label = step(ctx, c, 2, n_lines, far_field, keep_continuum_flux=True)
    assert label == STEP + " (continuum)" and np.array_equal(both["F"], kept["F"], equal_nan=True)
    assert np.array_equal(both["total"], kept["total"])
    judge_step(c, label, both)


@pytest.mark.parametrize("n_depth,n_theta", FUSED)
def test_general_kernel_in_the_step(ctx, n_depth, n_theta):
    """the general segmented kernel behind the fused step, and its continuum launch"""
    c = T.case(n_depth, n_theta)
    out, label = step(ctx, c, 1, 60, 0, keep_continuum_flux=True)
    assert label == GENERAL + " (continuum)"
    judge_step(c, label, out)


@pytest.mark.parametrize("n_depth,n_theta", [(56, 20), (175, 20)])
def test_two_chains_per_lane(ctx, n_depth, n_theta):
    """k_raytrace_cont<1>: the total and the continuum traced by the same lane"""
    c = T.case(n_depth, n_theta)
    out, label = step(ctx, c, 0, 60, 0, keep_continuum_flux=True)
    assert label == CONT
    judge_step(c, CONT, out)
    none, label = step(ctx, c, 0, 0, 0, keep_continuum_flux=True)
    assert label == CONT and np.array_equal(none["F"], none["Fc"], equal_nan=True)
    judge_step(c, CONT, none)


@pytest.mark.parametrize("n_depth,n_theta", SPHERICAL)
def test_two_chains_per_lane_spherical(ctx, n_depth, n_theta):
    c = T.case(n_depth, n_theta, 16, "grouped", T.CLASSES, True)
    out, label = step(ctx, c, 0, 60, 0, keep_continuum_flux=True)
    assert label == CONT
    judge_step(c, CONT, out)


# ---- the contribution function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth,n_theta,per", [(9, 20, 16), (56, 20, 16), (302, 20, 4)])
def test_contribution(ctx, n_depth, n_theta, per):
    c = T.case(n_depth, n_theta, per)
    ref = c.reference()
    Ft, _, Ct = c.truth(contribution=True)
    Co = cref.contribution_function(c.nus, c.temps, c.ray, c.weights, c.alphas)  # the definition in numpy's double precision: the oracle's part
    with launching(ctx):
        Cg = ops.contribution_arrays(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx)
        label = ctx.profile_variant("k_contribution")
    assert label == "k_contribution<1>"
    judge(c, label, "C", Cg, Ct, Co)
    assert np.array_equal(np.isnan(Cg).any(axis=0), np.isnan(ref["Fo"][-1]))  # a column is undefined in C exactly where the flux is
    zeros(c, Cg)
    # sum_k C[k] against the truth's emergent flux, on the scale of the column's flux; the sums in extended precision (no rounding of their own)
    ok = ~np.isnan(ref["Fo"][-1])
    scale = np.maximum(np.abs(np.where(np.isfinite(ref["Fo"]), Ft, 0)).max(axis=0), T.L(1e-300))
    d_gpu = np.abs(Cg.astype(T.L).sum(axis=0) - Ft[-1]) / scale
    d_oracle = np.abs(Co.astype(T.L).sum(axis=0) - Ft[-1]) / scale
    missed = []
    for name in c.classes:
        cols = c.columns(name) & ok
        if not cols.any():
            continue
        g, o = float(d_gpu[cols].max()), float(d_oracle[cols].max())
        T.RECORD.append((label, "sum C", "plane", n_depth, n_theta, c.order, name, g, o))
        print(f"{label} sum C {n_depth}/{n_theta} {name}: kernel {g:.2e} oracle {o:.2e}")
        if name != "underflow" and not g <= T.bound(o, n_depth):
            missed.append((name, g, o))
    assert not missed, missed


# ---- the fp32 formal solution (mixed_precision = 1) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["grouped", "interleaved"])
@pytest.mark.parametrize("n_depth,n_theta", [(9, 20), (56, 20)])
def test_fp32_formal_solution(ctx, n_depth, n_theta, order):
    """the tolerance path on the classes its header documents: finite everywhere, within the mode's stated 1e-4 of the column's scale
    from the truth, transparent columns exactly 0"""
    c = T.case(n_depth, n_theta, 16, order, T.F32_CLASSES)
    Ft = c.reference()["Ft"]
    with launching(ctx, segmented_raytrace=0, mixed_precision=1):
        F, _ = ops.raytrace_arrays(c.nus, c.temps, c.ray, c.weights, c.alphas, ctx=ctx)
        label = ctx.profile_variant("k_raytrace")
    assert label == F32
    assert np.isfinite(F).all()
    d = T.distance(F, Ft, np.ones(F.shape, dtype=bool))
    for name in c.classes:
        worst = float(d[c.columns(name)].max())
        T.RECORD.append((F32, "F", "plane", n_depth, n_theta, order, name, worst, float("nan")))
        print(f"{F32} F {n_depth}/{n_theta} {order} {name}: kernel {worst:.2e}")
    assert d.max() <= 1e-4, {name: float(d[c.columns(name)].max()) for name in c.classes}
    zeros(c, F)
