"""Whose error is it?  The formal solution of random columns (the cases of scripts/fuzz_raytrace.py, plane-parallel) three times:
the reference's formulas in 80-bit extended precision (numpy longdouble: the "truth" for these formulas), the double-precision
oracle, and the GPU — errors of the last two against the first, scaled by the largest intensity of the ray / flux of the column.
For 5e-4 <= tau < 50 the reference forms w1 = w0 - tau e^-tau and w2 = 2 w1 - tau^2 e^-tau (radiation_field_solvers/base.py:38-45):
one ulp of exp is amplified by 1 / tau^2 and 1 / tau^3, so ANY double-precision evaluation is ~1e-16 / tau^3 off near tau = 5e-4.
python scripts/r4/rt_truth.py SEED..."""
import os, sys
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import oracle
from formal_solution_truth import truth  # noqa: F401  (the one definition; the suite holds every kernel to it: tests/test_gpu_formal_solution_truth.py)
from stardis_amd import ops, synth


def scaled(a, ref):
    a, ref = np.nan_to_num(np.asarray(a, dtype=np.float64)), np.nan_to_num(np.asarray(ref, dtype=np.float64))
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1e-300)))


for seed in map(int, sys.argv[1:] if __name__ == "__main__" else []):
    rng = np.random.default_rng(31000 + seed)
    n_depth = int(rng.choice([2, 3, 5, 9, 30, 56, 57, 64, 65, 90, 130, 200]))
    n_theta = int(rng.choice([1, 2, 3, 7, 20, 21, 33, 64, 65, 70, 140]))
    n_nu = int(rng.choice([1, 2, 5, 63, 64, 65, 300, 1500, 6000]))
    spherical = bool(rng.random() < 0.3); track = bool(rng.random() < 0.4); accumulate = bool(rng.random() < 0.3) and not spherical
    temps = np.sort(rng.uniform(2500.0, 12000.0, n_depth))
    if rng.random() < 0.5:
        temps = temps[::-1].copy()
    dist = rng.uniform(2e5, 4e7, n_depth - 1)
    nus = np.sort(rng.uniform(2.5e14, 1.2e15, n_nu))[::-1].copy()
    regime = rng.integers(0, 5, n_nu)
    lo = np.choose(regime, [-30.0, -16.0, -9.0, -4.5, -16.0]); hi = np.choose(regime, [-30.0, -13.0, -5.0, -2.0, -2.0])
    alphas = 10.0 ** rng.uniform(lo, hi, (n_depth, n_nu)); alphas[:, regime == 0] = 0.0
    if rng.random() < 0.3 and n_depth > 3:
        alphas[int(rng.integers(0, n_depth)), :] = 0.0
    if spherical or n_depth * n_theta * n_nu > 3e6:
        print(f"seed {seed}: skipped (spherical or large: depth {n_depth} theta {n_theta} nu {n_nu})"); continue
    th, w = synth.thetas_and_weights(n_theta)
    Ft, It = truth(nus, temps, dist, th, w, alphas)
    with np.errstate(all="ignore"):
        Fo, Io = oracle.raytrace(nus, temps, dist, th, w, alphas, track=True)
    Fg, Ig = ops.raytrace_arrays(nus, temps, dist.reshape(-1, 1) / np.cos(th), w, alphas, track=True)
    print(f"seed {seed}: depth {n_depth} theta {n_theta} nu {n_nu}:  oracle vs truth: flux {scaled(Fo, Ft):.1e} intensity {scaled(Io, It):.1e};  "
          f"GPU vs truth: flux {scaled(Fg, Ft):.1e} intensity {scaled(Ig, It):.1e};  GPU vs oracle: flux {scaled(Fg, Fo):.1e} intensity {scaled(Ig, Io):.1e}", flush=True)
