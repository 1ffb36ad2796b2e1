"""What the emergent intensities and the disk integration cost: in ONE process, after warm-up, at S-c2 and at the S-c3 shape (S-c3's
grid, model and 20 angles; 2000 lines, which none of the kernels below reads), the median over `samples` single profiled calls
(sdx_profile_get: HIP events on the context's stream) of
  k_emergent_intensity     on the step's total_alphas
  k_raytrace<1>            the plain formal-solution kernel on the same plane, flux only ("segmented_raytrace" = 0): the same walk
  k_disk_integrate         at V = 10 and 100 km/s on the 20 rings of the step's intensities, converted to per Angstrom
  k_rotate_integrated      at the same V on the step's F_lambda, without reference and derivatives: one spectrum, Gray's profile
and, at S-c2, the largest distance of k_disk_integrate from its longdouble restatement (tests/disk_integration_reference.py) on every
`stride`-th point, in units of the tests' allowance 1e-11 sum_r |w_r| max_window |I_r|.
    python scripts/disk_integration_cost.py [--samples 31] [--warmup 10] [--out profiles/disk_integration_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stride", type=int, default=191)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag, n_lines=LINES.get(tag))
        atm = w["atm"]
        syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                                  track_evaluations=False, keep_line=False, keep_intensities=True)
        for _ in range(a.warmup):
            syn.step()
        ctx.synchronize()
        n, nd, nt = syn.n_nu, syn.n_depth, syn.n_theta
        lam = K.nu_to_angstrom(w["nus"])
        flat = syn.disk_integrated(0.0)  # F_lambda of the step, on the device; also makes the disk buffers
        d_Flam, out = ctx.upload(np.array(flat.numpy())), ctx.empty((n,))
        d_F = ctx.empty((nd, n))
        d_rot = ctx.empty((2,))
        disk = syn._disk
        res = dict(n_nu=int(n), n_depth=int(nd), n_theta=int(nt), samples=a.samples, sum_ring_scale=round(float(np.sin(w["thetas"]).sum()), 3), kernel_us={},
                   velocities={})
        ctx.call("sdx_profile_enable", 1)
        ctx.set_option("segmented_raytrace", 0)
        try:
            calls = {
                "k_emergent_intensity": ("k_emergent_intensity", lambda: syn._enqueue_intensities()),
                "k_raytrace<1>": ("k_raytrace", lambda: ctx.call("sdx_raytrace_dev", nd, n, nt, syn.d_nus.ptr, syn.d_t.ptr, syn.d_ray.ptr, syn.d_w.ptr,
                                                                 syn.d_total.ptr, n, d_F.ptr, n, None, 0)),
            }
            for name, (stage, call) in calls.items():
                for _ in range(3):
                    call()
                res["kernel_us"][name] = median_us(ctx, stage, call, a.samples)
            res["raytrace_variant"] = ctx.profile_variant("k_raytrace")
            for V in VELOCITIES:
                d_rot.set(np.array([V, 0.6]))
                per_v = {
                    "k_disk_integrate": ("k_disk_integrate", lambda: ctx.call(
                        "sdx_disk_integrate_dev", n, disk["lambdas"].ptr, nt, disk["scale"].ptr, syn.d_w.ptr, disk["I_lambda"].ptr, n, None, d_rot.ptr,
                        out.ptr, None)),
                    "k_rotate_integrated": ("k_rotate_integrated", lambda: ctx.call(
                        "sdx_rotate_integrated_dev", n, disk["lambdas"].ptr, d_Flam.ptr, None, d_rot.ptr, out.ptr, None, None, None, None, None)),
                }
                us = {}
                for name, (stage, call) in per_v.items():
                    for _ in range(3):
                        call()
                    us[name] = median_us(ctx, stage, call, a.samples)
                points = round(float(2 * V / K.C_KMS * np.median(lam) * (n - 1) / (lam[-1] - lam[0])), 1)
                res["velocities"][f"{V:g}"] = dict(points_per_window_at_scale_1=points, kernel_us=us,
                                                   ratio=round(us["k_disk_integrate"] / us["k_rotate_integrated"], 2))
        finally:
            ctx.set_option("segmented_raytrace", -1)
            ctx.call("sdx_profile_enable", 0)
        if tag == "S-c2":
            import disk_integration_reference as D

            if D.EXTENDED:
                points = list(range(0, n, a.stride)) + [n - 1]
                rings = np.array(disk["I_lambda"].numpy())
                scale, wts = np.sin(w["thetas"]), np.asarray(w["weights"], dtype=np.float64)
                dist = {}
                for V in VELOCITIES:
                    got = np.array(syn.disk_integrated(V).numpy())[points]
                    want, allow = D.disk_integrate(lam, rings, scale, wts, V, points)
                    dist[f"{V:g}"] = float(np.max(np.abs(got.astype(D.LD) - want) / (D.ROT_TOL * allow)))
                res["distance_from_restatement_in_allowances"] = dict(points=len(points), **dist)
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
        syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
