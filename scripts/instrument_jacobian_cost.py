"""What the instrument's forward mode costs, in ONE process after warm-up:
  kernels   k_observe_tangent with ALL its outputs (out, dout_velocity, dout_lsf, dout_flux with dflux and dreference) beside k_observe
            and k_observe_adjoint, and k_rotate_tangent beside k_rotate, each the median of `samples` single profiled calls (the
            library's own HIP-event timing per stage) on the workload's grid with a random spectrum:
            S-c2 (7634 points) with 2048 pixels at R = 5e4 (72 points per window: a wave per pixel) and R = 2e5 (20: eight lanes per
            pixel), v sin i = 30 km/s;  S-c3 with its 90 297-pixel instrument at R = 3e4
  jacobian  on S-c2 with rotation and macroturbulence, per call of SpectralSynthesizer.observed_jacobian with all four names, beside
            what a user does without it: four central differences of whole steps (two steps per parameter under the setters; for
            sigma two steps of a synthesizer with a rebuilt Instrument) — host wall-clock per call including the wait for the
            stream, the median of `samples` calls, both in the same run
  accuracy  the distance of obs_response and of obs_response_grad from 50-digit mpmath on the points of
            tests/test_gpu_observe_tangent.py (its own function), and what the test allows
    python scripts/instrument_jacobian_cost.py [--samples 51] [--out profiles/instrument_jacobian_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from observe_cost import pixels  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import Instrument, pixel_sigma  # noqa: E402

V_ROT, V_MAC, V_RAD = 30.0, 5.0, 12.0


def stage_us(ctx, stage, call, samples):
    """median microseconds recorded under `stage` over single profiled calls"""
    for _ in range(3):
        call()
    us = []
    for _ in range(samples):
        ctx.call("sdx_profile_reset")
        call()
        ctx.synchronize()
        us.append(ctx.profile(stage)[1] * 1e3)
    return round(float(np.median(us)), 2)


def kernels(ctx, tag, lam, edges, R, samples):
    n, n_pix = int(lam.size), int(edges.size - 1)
    rng = np.random.default_rng(11)
    inst = Instrument(edges, resolving_power=R, ctx=ctx, v_rot=V_ROT)
    inst.set_radial_velocity(V_RAD)
    d_lam, d_nus = ctx.upload(lam), ctx.upload(K.C_CGS * 1.0e8 / lam)
    d_f, d_g, d_df, d_dg = (ctx.upload(a) for a in (1.0 + 0.1 * rng.standard_normal(n), 2.0 + 0.5 * np.sin(lam / 3.0), rng.standard_normal(n), rng.standard_normal(n)))
    d_c = ctx.upload(rng.standard_normal(n_pix))
    pix = [ctx.empty((n_pix,)) for _ in range(4)]
    grid = [ctx.empty((n,)) for _ in range(4)]
    common = (n, d_lam.ptr, d_f.ptr, d_g.ptr, n_pix, inst.d_edges.ptr, inst.d_sigma.ptr, inst.d_doppler.ptr)
    calls = {
        "k_observe": lambda: ctx.call("sdx_observe_dev", *common, pix[0].ptr),
        "k_observe_adjoint": lambda: ctx.call("sdx_observe_adjoint_dev", *common, d_c.ptr, d_nus.ptr, grid[0].ptr, grid[1].ptr),
        "k_observe_tangent": lambda: ctx.call("sdx_observe_tangent_dev", *common, d_df.ptr, d_dg.ptr, *(a.ptr for a in pix)),
        "k_rotate": lambda: ctx.call("sdx_rotate_dev", n, d_lam.ptr, d_f.ptr, d_g.ptr, inst.d_rot.ptr, grid[0].ptr, grid[1].ptr),
        "k_rotate_tangent": lambda: ctx.call("sdx_rotate_tangent_dev", n, d_lam.ptr, d_f.ptr, d_g.ptr, inst.d_rot.ptr, *(a.ptr for a in grid)),
    }
    us = {k: stage_us(ctx, k, call, samples) for k, call in calls.items()}
    per_angstrom = (n - 1) / (lam[-1] - lam[0])
    return dict(n_nu=n, n_pix=n_pix, resolving_power=R, v_rot=V_ROT,
                points_per_observe_window=round(float(np.mean(np.diff(edges) + 16.0 * inst.sigma) * per_angstrom), 1),
                points_per_rotation_window=round(float(2 * V_ROT / K.C_KMS * np.median(lam) * per_angstrom), 1), median_us=us,
                tangent_over_observe=round(us["k_observe_tangent"] / us["k_observe"], 2),
                tangent_over_observe_plus_adjoint=round(us["k_observe_tangent"] / (us["k_observe"] + us["k_observe_adjoint"]), 2),
                rotate_tangent_over_rotate=round(us["k_rotate_tangent"] / us["k_rotate"], 2))


def wall_us(ctx, call, samples):
    for _ in range(3):
        call()
    ctx.synchronize()
    us = []
    for _ in range(samples):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(us)), 1)


def jacobian(ctx, samples):
    w = synth.make_workload("S-c2")
    atm = w["atm"]
    lam = K.nu_to_angstrom(w["nus"])
    edges, R = pixels("S-c2", lam)
    sigma = pixel_sigma(edges, resolving_power=R)[1]
    make = lambda k=1.0: Instrument(edges, sigma=k * sigma, ctx=ctx, v_rot=V_ROT, v_mac=V_MAC)  # noqa: E731
    inst, wider, narrower = make(), make(1.01), make(0.99)
    args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
    common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=False)
    syn, syn_wider, syn_narrower = (SpectralSynthesizer(*args, instrument=i, **common) for i in (inst, wider, narrower))
    for s in (syn, syn_wider, syn_narrower):
        s.instrument.set_radial_velocity(V_RAD)
        for _ in range(5):
            s.step()
    names = ("v_rad", "lsf", "v_mac", "limb_darkening")

    def differences():
        out = []
        for knob, h in ((inst.set_radial_velocity, (V_RAD + 0.02, V_RAD - 0.02, V_RAD)), (inst.set_macroturbulence, (V_MAC * 1.008, V_MAC * 0.992, V_MAC)),
                        (lambda e: inst.set_rotation(V_ROT, e), (0.62, 0.58, 0.6))):
            for value in h[:2]:
                knob(value)
                syn.step()
                out.append(syn.observed.numpy())
            knob(h[2])
        for s in (syn_wider, syn_narrower):
            s.step()
            out.append(s.observed.numpy())
        return out

    us = dict(step=wall_us(ctx, syn.step, samples), observed_jacobian=wall_us(ctx, lambda: [v.numpy() for v in syn.observed_jacobian(names).values()], samples),
              four_central_differences=wall_us(ctx, differences, samples))
    for s in (syn, syn_wider, syn_narrower):
        s.close()
    return dict(n_nu=int(lam.size), n_pix=int(edges.size - 1), resolving_power=R, v_rot=V_ROT, v_mac=V_MAC, names=list(names), wall_us=us,
                differences_over_jacobian=round(us["four_central_differences"] / us["observed_jacobian"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=51)
    ap.add_argument("--out", default=None, help="also write the result to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = {"kernels": {}}
    ctx.call("sdx_profile_enable", 1)
    try:
        lam = K.nu_to_angstrom(synth.tracing_grid(6500.0, 6600.0, R=5.0e5))
        for R in (5.0e4, 2.0e5):
            res["kernels"][f"S-c2, R = {R:.0e}"] = kernels(ctx, "S-c2", lam, pixels("S-c2", lam)[0], R, a.samples)
        cfg = synth.WORKLOADS["S-c3"]
        lam = K.nu_to_angstrom(synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R"), cfg.get("step")))
        edges, R = pixels("S-c3", lam)
        res["kernels"]["S-c3"] = kernels(ctx, "S-c3", lam, edges, R, a.samples)
    finally:
        ctx.call("sdx_profile_enable", 0)
    print(json.dumps(res["kernels"]), flush=True)
    res["jacobian"] = jacobian(ctx, a.samples)
    print(json.dumps(res["jacobian"]), flush=True)
    import test_gpu_observe_tangent as G  # noqa: E402  (the test's own measurement)

    d_r, d_rx, d_rs = G.response_gradient_distances(ctx)
    res["accuracy"] = dict(points=int(G.tref.response_grad_points()[0].size), obs_response=d_r, dr_dx=d_rx, dr_dlnsigma=d_rs, allowed=4 * d_r)
    print(json.dumps(res["accuracy"]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
