"""What the transpose and the V-derivative of the disk integration and the per-angle response cost: in ONE process, after warm-up, at
S-c2 and at the S-c3 shape (S-c3's grid, model and 20 angles; 2000 lines), 20 rings, V = 10 and 100 km/s, the median over `samples`
single profiled calls (sdx_profile_get: HIP events on the context's stream) of
  k_disk_integrate<false>      sdx_disk_integrate_dev on the step's intensities, converted to per Angstrom
  k_disk_integrate<true>       sdx_disk_integrate_deriv_dev on the same: out and d out / d ln V
  k_disk_integrate_adjoint     sdx_disk_integrate_adjoint_dev with nus (both launches: denominators, gather)
  k_response                   sdx_response_dev on the step's total_alphas, both outputs
  k_response_angles            sdx_response_angles_dev on the same, a cotangent plane in the flux weights' place
  20 one-hot k_response        the n_theta launches of sdx_response_dev with one-hot weights that k_response_angles replaces (their sum)
and, wall clock around calls that wait for the stream (time.perf_counter, the median), of
  chi2_disk_gradient           one call: chi-square, d chi2 / dV and the gradient to ln gf of every line
  central difference + lines   two observed_disk_integrated (V (1 +- 1e-3), downloaded) and one chi2_line_gradient
    python scripts/disk_adjoint_cost.py [--samples 31] [--warmup 10] [--out profiles/disk_adjoint_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import Instrument  # noqa: E402

VELOCITIES = (10.0, 100.0)
LINES = {"S-c2": None, "S-c3": 2000}


def median_us(ctx, stage, call, samples):
    us = []
    for _ in range(samples):
        ctx.call("sdx_profile_reset")
        call()
        ctx.synchronize()
        us.append(ctx.profile(stage)[1] * 1e3)
    return round(float(np.median(us)), 2)


def median_wall_ms(ctx, call, samples):
    ms = []
    for _ in range(samples):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=31)
    ap.add_argument("--wall-samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag, n_lines=LINES.get(tag))
        atm = w["atm"]
        lam = K.nu_to_angstrom(w["nus"])
        span = lam[-1] - lam[0]
        inst = Instrument(np.linspace(lam[0] + 0.05 * span, lam[-1] - 0.05 * span, 2049), resolving_power=5.0e4, ctx=ctx, v_mac=3.0)
        syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                                  track_evaluations=False, keep_line=False, keep_intensities=True, keep_response=True, instrument=inst)
        for _ in range(a.warmup):
            syn.step()
        ctx.synchronize()
        n, nd, nt = syn.n_nu, syn.n_depth, syn.n_theta
        syn.disk_integrated(0.0)  # makes the disk buffers and converts the rings
        disk = syn._disk
        rng = np.random.default_rng(1)
        d_u = ctx.upload(rng.standard_normal(n))
        out, dout, W = ctx.empty((n,)), ctx.empty((n,)), ctx.empty((nt, n))
        d_rot = ctx.empty((2,))
        d_cot = ctx.upload(rng.standard_normal((nt, n)))
        d_Ra, d_Rs = ctx.empty((nd, n)), ctx.empty((nd, n))
        one_hot = [ctx.upload(np.eye(nt)[k]) for k in range(nt)]
        res = dict(n_nu=int(n), n_depth=int(nd), n_theta=int(nt), n_lines=int(syn.n_lines), n_pix=int(inst.n_pix), samples=a.samples, kernel_us={},
                   velocities={})
        ctx.call("sdx_profile_enable", 1)
        try:
            def response(weights):
                ctx.call("sdx_response_dev", nd, n, nt, syn.d_nus.ptr, syn.d_t.ptr, syn.d_ray.ptr, weights.ptr, syn.d_total.ptr, n, None, 0, d_Ra.ptr, n,
                         d_Rs.ptr, n)

            def all_one_hot():
                for wts in one_hot:
                    response(wts)

            calls = {
                "k_response": ("k_response", lambda: response(syn.d_w)),
                "k_response_angles": ("k_response_angles", lambda: ctx.call(
                    "sdx_response_angles_dev", nd, n, nt, syn.d_nus.ptr, syn.d_t.ptr, syn.d_ray.ptr, d_cot.ptr, n, syn.d_total.ptr, n, None, 0, d_Ra.ptr, n,
                    d_Rs.ptr, n)),
                "one_hot_k_response_x_n_theta": ("k_response", all_one_hot),
            }
            for name, (stage, call) in calls.items():
                for _ in range(3):
                    call()
                res["kernel_us"][name] = median_us(ctx, stage, call, a.samples)
            res["kernel_us"]["angles_over_response"] = round(res["kernel_us"]["k_response_angles"] / res["kernel_us"]["k_response"], 3)
            for V in VELOCITIES:
                d_rot.set(np.array([V, 0.0]))
                common = (n, disk["lambdas"].ptr, nt, disk["scale"].ptr, syn.d_w.ptr)
                per_v = {
                    "k_disk_integrate<false>": ("k_disk_integrate", lambda: ctx.call(
                        "sdx_disk_integrate_dev", *common, disk["I_lambda"].ptr, n, None, d_rot.ptr, out.ptr, None)),
                    "k_disk_integrate<true>": ("k_disk_integrate", lambda: ctx.call(
                        "sdx_disk_integrate_deriv_dev", *common, disk["I_lambda"].ptr, n, None, d_rot.ptr, out.ptr, None, dout.ptr, None)),
                    "k_disk_integrate_adjoint": ("k_disk_integrate_adjoint", lambda: ctx.call(
                        "sdx_disk_integrate_adjoint_dev", *common, d_rot.ptr, d_u.ptr, None, syn.d_nus.ptr, W.ptr, n, None)),
                }
                us = {}
                for name, (stage, call) in per_v.items():
                    for _ in range(3):
                        call()
                    us[name] = median_us(ctx, stage, call, a.samples)
                res["velocities"][f"{V:g}"] = dict(kernel_us=us, deriv_over_forward=round(us["k_disk_integrate<true>"] / us["k_disk_integrate<false>"], 3),
                                                   adjoint_over_forward=round(us["k_disk_integrate_adjoint"] / us["k_disk_integrate<false>"], 3))
        finally:
            ctx.call("sdx_profile_enable", 0)
        # the chi-square calls wait for the stream and work on the host as well: wall clock
        for V in VELOCITIES:
            base = np.array(syn.observed_disk_integrated(V).numpy())
            data = base * (1.0 + 0.01 * rng.standard_normal(base.size))
            ivar = np.full(base.size, 1.0 / np.nanmax(base) ** 2)

            def by_differences():
                hi = syn.observed_disk_integrated(V * (1 + 1e-3)).numpy().copy()
                lo = syn.observed_disk_integrated(V * (1 - 1e-3)).numpy().copy()
                return hi, lo, syn.chi2_line_gradient(data, ivar)[1].numpy()

            gradient = lambda: syn.chi2_disk_gradient(data, ivar, V)[2].numpy()  # noqa: E731
            for call in (gradient, by_differences):
                call()
            res["velocities"][f"{V:g}"]["wall_ms"] = dict(chi2_disk_gradient=median_wall_ms(ctx, gradient, a.wall_samples),
                                                          central_difference_plus_chi2_line_gradient=median_wall_ms(ctx, by_differences, a.wall_samples))
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
        syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
