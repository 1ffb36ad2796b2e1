"""What the cell-integrated rotation profile costs beside the sampled one: in ONE process, after warm-up, per configuration
      S-c2: 2048 pixels at R = 50 000, V = 2, 10 and 100 km/s (about 7, 33 and 334 points per rotation window)
      S-c3: the 90 297-pixel instrument at R = 30 000, V = 10
the median over `samples` single profiled calls (sdx_profile_get: HIP events on the context's stream) of
  k_rotate_integrated             without and with its four derivative outputs (flux and reference)
  k_rotate_integrated_adjoint     both launches, with nus
  k_rotate, k_rotate_adjoint      the sampled mode: the code path as it was before the integrated mode existed
  k_macroturbulence               at the same window length (zeta = V / 6), without its derivative
on the step's own F_lambda and continuum, and — event-timed, the median of `rounds` — one observed_jacobian call with all five names
beside the two whole steps of the central difference that "v_rot" replaces.
    python scripts/rotation_integrated_cost.py [--samples 31] [--rounds 7] [--warmup 10] [--out profiles/rotation_integrated_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from observe_cost import pixels, timed_ms  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import Instrument  # noqa: E402

VELOCITIES = {"S-c2": (2.0, 10.0, 100.0), "S-c3": (10.0,)}
NAMES = ("v_rad", "lsf", "v_mac", "limb_darkening", "v_rot")


def median_us(ctx, stage, call, samples):
    us = []
    for _ in range(samples):
        ctx.call("sdx_profile_reset")
        call()
        ctx.synchronize()
        us.append(ctx.profile(stage)[1] * 1e3)
    return round(float(np.median(us)), 2)


def event_ms(ctx, call):
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    call()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag)
        atm = w["atm"]
        lam = K.nu_to_angstrom(w["nus"])
        n = int(lam.size)
        edges, R = pixels(tag, lam)
        inst = Instrument(edges, resolving_power=R, ctx=ctx, v_rot=VELOCITIES[tag][0], v_mac=3.0, rotation="integrated")
        syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], instrument=inst,
                                  ctx=ctx, track_evaluations=False, keep_line=False, keep_total=False, keep_continuum_flux=True)
        for _ in range(a.warmup):
            syn.step()
        ctx.synchronize()
        lam_p, f_p, g_p, nus_p = syn.d_lambdas.ptr, syn.d_Flam.ptr, syn.d_Fclam.ptr, syn.d_nus.ptr
        o = [ctx.empty((n,)) for _ in range(6)]
        d_mac = ctx.empty((1,))
        res = dict(n_nu=n, n_pix=int(edges.size - 1), resolving_power=R, samples=a.samples, rounds=a.rounds, velocities={})
        for V in VELOCITIES[tag]:
            inst.set_rotation(V)
            d_mac.set(np.array([V / 6.0]))
            rot = inst.d_rot.ptr
            calls = {
                "k_rotate_integrated": ("k_rotate_integrated", lambda: ctx.call(
                    "sdx_rotate_integrated_dev", n, lam_p, f_p, g_p, rot, o[0].ptr, o[1].ptr, None, None, None, None)),
                "k_rotate_integrated, derivatives": ("k_rotate_integrated", lambda: ctx.call(
                    "sdx_rotate_integrated_dev", n, lam_p, f_p, g_p, rot, *(b.ptr for b in o))),
                "k_rotate_integrated_adjoint": ("k_rotate_integrated_adjoint", lambda: ctx.call(
                    "sdx_rotate_integrated_adjoint_dev", n, lam_p, rot, f_p, g_p, nus_p, o[0].ptr, o[1].ptr)),
                "k_rotate": ("k_rotate", lambda: ctx.call("sdx_rotate_dev", n, lam_p, f_p, g_p, rot, o[0].ptr, o[1].ptr)),
                "k_rotate_adjoint": ("k_rotate_adjoint", lambda: ctx.call(
                    "sdx_rotate_adjoint_dev", n, lam_p, rot, f_p, g_p, nus_p, o[0].ptr, o[1].ptr)),
                "k_macroturbulence, zeta = V / 6": ("k_macroturbulence", lambda: ctx.call(
                    "sdx_macroturbulence_dev", n, lam_p, f_p, g_p, d_mac.ptr, o[0].ptr, o[1].ptr, None, None)),
            }
            ctx.call("sdx_profile_enable", 1)
            try:
                for _, call in calls.values():
                    for _ in range(3):
                        call()
                kernels = {k: median_us(ctx, stage, call, a.samples) for k, (stage, call) in calls.items()}
            finally:
                ctx.call("sdx_profile_enable", 0)
            syn.observed_jacobian(NAMES, normalized=True)
            ctx.synchronize()
            jac = [event_ms(ctx, lambda: syn.observed_jacobian(NAMES, normalized=True)) * 1e3 for _ in range(a.rounds)]
            two = [2 * timed_ms(ctx, syn, 2) * 1e3 for _ in range(a.rounds)]
            points = round(float(2 * V / K.C_KMS * np.median(lam) * (n - 1) / (lam[-1] - lam[0])), 1)
            res["velocities"][f"{V:g}"] = dict(points_per_window=points, kernel_us=kernels,
                                               jacobian_five_columns_us=round(float(np.median(jac)), 2),
                                               two_whole_steps_us=round(float(np.median(two)), 2))
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
        syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
