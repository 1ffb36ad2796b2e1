"""What the instrument model costs: in ONE process, alternating two variants after warm-up, with HIP-event timing on the context's
stream, at S-c2 and at full-size S-c3:
  (a) plain   the fused step (SpectralSynthesizer): the yardstick, the step as it is without the option
  (b) instr   the same step with instrument=Instrument(...): sdx_flux_nu_to_lambda_dev and sdx_observe_dev behind the synthesis
      S-c2: 2048 equal pixels over 6502 - 6598 A at R = 50 000 (about 72 grid points per window: one wave per pixel)
      S-c3: pixels of 1 / 2.5 FWHM at R = 30 000 over the whole range (about 24 points per window: eight pixels per wave)
Each variant is timed in `rounds` interleaved rounds of `steps` eager steps; the spread of (a) across its rounds is the run-to-run
spread against which the difference is read.  A second, profiled pass reports sdx_profile_get("k_observe"), ("k_flux_nu_to_lambda")
and ("k_raytrace") per step.
    python scripts/observe_cost.py [--steps 50] [--rounds 7] [--warmup 20] [--out profiles/observe_cost.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import Instrument  # noqa: E402


def timed_ms(ctx, syn, steps):
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    for _ in range(steps):
        syn.step()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return ms.value / steps


def pixels(tag, lam):
    """-> (edges, resolving power) of the workload's instrument"""
    if tag == "S-c2":
        return np.linspace(6502.0, 6598.0, 2049), 5.0e4
    R = 3.0e4
    n = int(math.floor(math.log(lam[-1] / lam[0]) * R * 2.5))  # pixel = FWHM / 2.5 = lambda / (2.5 R)
    return lam[0] * np.exp(np.arange(n + 1) / (R * 2.5)), R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag)
        atm = w["atm"]
        lam = K.nu_to_angstrom(w["nus"])
        edges, R = pixels(tag, lam)
        inst = Instrument(edges, resolving_power=R, ctx=ctx)
        args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
        common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=False)
        variants = {"plain": SpectralSynthesizer(*args, **common), "instr": SpectralSynthesizer(*args, instrument=inst, **common)}
        for syn in variants.values():
            for _ in range(a.warmup):
                syn.step()
        ctx.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, syn in variants.items():
                times[k].append(timed_ms(ctx, syn, a.steps) * 1e3)
        prof = {}
        ctx.call("sdx_profile_enable", 1)
        for k, syn in variants.items():
            ctx.call("sdx_profile_reset")
            for _ in range(a.steps):
                syn.step()
            ctx.synchronize()
            prof[k] = {}
            for kernel in ("k_raytrace", "k_flux_nu_to_lambda", "k_observe"):
                n, ms = ctx.profile(kernel)
                prof[k][kernel] = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=n / a.steps)
        raytrace_variant = ctx.profile_variant("k_raytrace")
        ctx.call("sdx_profile_enable", 0)
        observed = variants["instr"].observed.numpy()
        sigma_pts = inst.sigma / np.interp((edges[:-1] + edges[1:]) / 2, lam[:-1], np.diff(lam))
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = dict(
            n_nu=int(w["nus"].size), n_pix=int(inst.n_pix), resolving_power=R, steps_per_round=a.steps, rounds=a.rounds,
            points_per_window=round(float(np.median(16 * sigma_pts + np.diff(edges) / (inst.sigma / sigma_pts))), 1),
            sigma_in_grid_points=round(float(np.median(sigma_pts)), 2),
            nan_pixels=int(np.isnan(observed).sum()),
            us_per_step={k: [round(x, 2) for x in v] for k, v in times.items()},
            median_us={k: round(v, 2) for k, v in med.items()},
            plain_spread_us=round(float(np.max(times["plain"]) - np.min(times["plain"])), 2),
            extra_us=round(med["instr"] - med["plain"], 2),
            profiled=prof, raytrace_variant=raytrace_variant,
        )
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
        for syn in variants.values():
            syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
