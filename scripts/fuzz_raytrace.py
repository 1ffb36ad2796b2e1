"""GPU experiment: the formal-solution entry points on random shapes and optical-depth regimes against the oracle
(radiation_field_solvers/base.py:85-346): 2 - 200 depth points, 1 - 140 angles (chunks of 64 above that; angle counts that do not
divide 64), 1 - 6000 frequencies (segmented kernel below its size threshold, k_raytrace<1> above, the per-lane kernel for very deep
models), columns that are transparent (alpha = 0), optically thin (tau ~ 1e-9: the series of the weights), thick (tau >= 50) or
mixed within one ray, plane-parallel and spherical (inward sweep + photospheric correction), a flux that is written or added
to, with and without tracked intensities, and the fp32 formal solution of the mixed mode against the fp64 one.
Criterion: on random rough columns the reference's formulas are ill-conditioned (w1 = w0 - tau e^-tau, w2 = 2 w1 - tau^2 e^-tau for
tau >= 5e-4: one ulp of exp times 1 / tau^3), so the double-precision oracle itself is 1e-9 .. 4e-7 from an exact evaluation of the
same formulas; the GPU is therefore measured against an 80-bit evaluation (tests/formal_solution_truth.py) and must be no further from it
than four times the oracle's own distance (+ 1e-10; over 200 seeds the ratio was below 1.2 in all but two cases: 2.4 and 3.2).
python scripts/fuzz_raytrace.py FIRST LAST"""
import os, sys, traceback
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import oracle
sys.path.insert(0, os.path.join(root, "tests"))
from formal_solution_truth import truth
from stardis_amd import ops, synth
from stardis_amd._lib import default_context

ctx = default_context()
TOL = 1e-10


def scaled(a, ref, axis=0):
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref).max(axis=axis, keepdims=True), 1e-300)))


bad = 0
for seed in range(int(sys.argv[1]), int(sys.argv[2])):
    try:
        rng = np.random.default_rng(31000 + seed)
        n_depth = int(rng.choice([2, 3, 5, 9, 30, 56, 57, 64, 65, 90, 130, 200]))
        n_theta = int(rng.choice([1, 2, 3, 7, 20, 21, 33, 64, 65, 70, 140]))
        n_nu = int(rng.choice([1, 2, 5, 63, 64, 65, 300, 1500, 6000]))
        n_nu = max(1, min(n_nu, int(1.5e6 // (n_depth * n_theta))))  # (the 80-bit evaluation on the host bounds the size)
        spherical = bool(rng.random() < 0.3)
        track = bool(rng.random() < 0.4)
        accumulate = bool(rng.random() < 0.3) and not spherical
        temps = np.sort(rng.uniform(2500.0, 12000.0, n_depth))
        if rng.random() < 0.5:
            temps = temps[::-1].copy()
        dist = rng.uniform(2e5, 4e7, n_depth - 1)
        nus = np.sort(rng.uniform(2.5e14, 1.2e15, n_nu))[::-1].copy()
        regime = rng.integers(0, 5, n_nu)  # per column: 0 transparent, 1 thin, 2 moderate, 3 thick, 4 everything along the ray
        lo = np.choose(regime, [-30.0, -16.0, -9.0, -4.5, -16.0])
        hi = np.choose(regime, [-30.0, -13.0, -5.0, -2.0, -2.0])
        alphas = 10.0 ** rng.uniform(lo, hi, (n_depth, n_nu))
        alphas[:, regime == 0] = 0.0
        if rng.random() < 0.3 and n_depth > 3:  # a transparent LAYER inside otherwise opaque columns
            alphas[int(rng.integers(0, n_depth)), :] = 0.0
        th, w = synth.thetas_and_weights(n_theta)
        if spherical:
            r = 6.0e10 + np.concatenate([[0.0], np.cumsum(dist)])
            ref_r = float(r[-int(rng.integers(1, n_depth))])
            rd = oracle.calculate_spherical_ray(th, r)
            corr = (r[-1] / ref_r) ** 2
            with np.errstate(all="ignore"):
                ref, Iref = oracle.raytrace(nus, temps, None, th, w, alphas, track=True, spherical_r=r, reference_r=ref_r)
                Ft, It = truth(nus, temps, dist, th, w, alphas, ray_table=rd, correction=corr)
            F, I = ops.raytrace_arrays(nus, temps, rd, w, alphas, track=track, inward_rays=True, photospheric_correction=corr)
        else:
            rd = dist.reshape(-1, 1) / np.cos(th)
            F0 = rng.uniform(0.0, 1e-5, (n_depth, n_nu)) if accumulate else None
            with np.errstate(all="ignore"):
                ref, Iref = oracle.raytrace(nus, temps, dist, th, w, alphas, F_nu=None if F0 is None else F0.copy(), track=True)
                Ft, It = truth(nus, temps, dist, th, w, alphas)
            if F0 is not None:
                Ft = Ft + F0
            F, I = ops.raytrace_arrays(nus, temps, rd, w, alphas, F_nu=F0, track=track)
        assert np.array_equal(np.isnan(F), np.isnan(ref)), "NaN pattern of the flux"
        ok = ~np.isnan(ref)
        z = lambda a: np.where(ok, np.asarray(a, dtype=np.float64), 0.0)  # noqa: E731
        eF, oF = scaled(z(F), z(Ft)), scaled(z(ref), z(Ft))
        eI = scaled(np.nan_to_num(I), np.nan_to_num(np.asarray(It, dtype=np.float64))) if track else 0.0
        oI = scaled(np.nan_to_num(Iref), np.nan_to_num(np.asarray(It, dtype=np.float64))) if track else 0.0
        assert eF <= 4 * oF + TOL and eI <= 4 * oI + TOL, ("flux GPU / oracle vs 80-bit", eF, oF, "intensity", eI, oI)
        e32 = 0.0
        if not spherical and not accumulate and not track and n_theta <= 64:  # the shape the fp32 formal solution takes
            ctx.set_option("mixed_precision", 1)
            try:
                F32, _ = ops.raytrace_arrays(nus, temps, rd, w, alphas)
            finally:
                ctx.set_option("mixed_precision", 0)
            # (a transparent gap AHEAD of an opaque one makes the reference — and the fp64 kernels — divide by zero: NaN from there on;
            # the tolerance path takes such a step to first order and stays finite, by design: those columns are left out)
            fin = np.isfinite(F).all(axis=0)
            e32 = scaled(F32[:, fin], F[:, fin]) if fin.any() else 0.0
            assert np.isfinite(F32[:, fin]).all()
            assert e32 < 1e-4, ("fp32", e32)
        print(f"seed {seed}: ok  depth {n_depth} theta {n_theta} nu {n_nu}{' spherical' if spherical else ''}{' tracked' if track else ''}{' accumulate' if accumulate else ''}: flux {eF:.1e} (oracle {oF:.1e}) intensity {eI:.1e} (oracle {oI:.1e}) fp32 {e32:.1e}", flush=True)
    except Exception:
        bad += 1
        print(f"seed {seed}: FAILED", flush=True)
        traceback.print_exc()
print("failures:", bad)
