"""What the flux contribution function costs: in ONE process, alternating three variants after warm-up, with HIP-event timing on the
context's stream, at S-c2 and at full-size S-c3:
  (a) plain   the fused step (SpectralSynthesizer): the yardstick, the step as it is without the option
  (b) contr   the same step with keep_contribution=True (implies keep_total; sdx_contribution_dev behind the synthesis)
  (c) total   the same step with keep_total=True only: what (b) pays for the total_alphas plane it reads
Each variant is timed in `rounds` interleaved rounds of `steps` eager steps; the spread of (a) across its rounds is the run-to-run
spread against which the differences are read.  (b) - (c) is the contribution launch itself; a second, profiled pass reports
sdx_profile_get("k_contribution") and ("k_raytrace") per step.
    python scripts/contribution_cost.py [--steps 50] [--rounds 7] [--warmup 20] [--out profiles/contribution_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402


def timed_ms(ctx, syn, steps):
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    for _ in range(steps):
        syn.step()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return ms.value / steps


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
        args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
        common = dict(ctx=ctx, track_evaluations=False, keep_line=False)
        variants = {
            "plain": SpectralSynthesizer(*args, keep_total=False, **common),
            "contr": SpectralSynthesizer(*args, keep_total=False, keep_contribution=True, **common),
            "total": SpectralSynthesizer(*args, keep_total=True, **common),
        }
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
            for kernel in ("k_raytrace", "k_contribution"):
                n, ms = ctx.profile(kernel)
                prof[k][kernel] = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=n / a.steps)
        # like for like: k_raytrace<1>, whose layout k_contribution<1> shares, at this size (small grids run k_raytrace_seg by default)
        ctx.set_option("segmented_raytrace", 0)
        try:
            ctx.call("sdx_profile_reset")
            for _ in range(a.steps):
                variants["plain"].step()
            ctx.synchronize()
            n, ms = ctx.profile("k_raytrace")
            p1 = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=n / a.steps, variant=ctx.profile_variant("k_raytrace"))
        finally:
            ctx.set_option("segmented_raytrace", -1)
        ctx.call("sdx_profile_reset")
        variants["plain"].step()
        ctx.synchronize()
        default_variant = ctx.profile_variant("k_raytrace")
        ctx.call("sdx_profile_enable", 0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = dict(
            n_nu=int(w["nus"].size), steps_per_round=a.steps, rounds=a.rounds,
            us_per_step={k: [round(x, 2) for x in v] for k, v in times.items()},
            median_us={k: round(v, 2) for k, v in med.items()},
            plain_spread_us=round(float(np.max(times["plain"]) - np.min(times["plain"])), 2),
            contribution_launch_us=round(med["contr"] - med["total"], 2),
            keep_total_us=round(med["total"] - med["plain"], 2),
            extra_us=round(med["contr"] - med["plain"], 2),
            profiled=prof, default_raytrace_variant=default_variant, k_raytrace_one_wave_per_ray=p1,
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
