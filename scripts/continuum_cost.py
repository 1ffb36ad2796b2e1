"""What the continuum flux costs: in ONE process, alternating three variants after warm-up, with HIP-event timing on the context's
stream, at S-c2 and at full-size S-c3:
  (a) plain   the fused step (SpectralSynthesizer)
  (b) cont    the same step with keep_continuum_flux=True (k_raytrace_cont, or a second k_raytrace_seg launch on small grids)
  (c) zero    a zero-line synthesis of the same model: what a caller runs today to get the continuum
Each variant is timed in `rounds` interleaved rounds of `steps` eager steps; the spread of (a) across its rounds is the run-to-run
spread against which (b) - (a) is read.  A second, profiled pass reports sdx_profile_get("k_raytrace") per step of each variant.
    python scripts/continuum_cost.py [--steps 50] [--rounds 7] [--warmup 20]"""
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
    a = ap.parse_args()
    ctx = _lib.default_context()
    out = {}
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag)
        atm = w["atm"]
        nd = atm["temperatures"].size
        zero_lines = dict(line_nus=np.zeros(0), doppler_widths=np.zeros((0, nd)), gammas=np.zeros((0, nd)), alphas=np.zeros((0, nd)))
        args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"])
        common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=False)
        variants = {
            "plain": SpectralSynthesizer(*args, w["lines"], w["cont"], **common),
            "cont": SpectralSynthesizer(*args, w["lines"], w["cont"], keep_continuum_flux=True, **common),
            "zero": SpectralSynthesizer(*args, zero_lines, w["cont"], **common),
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
            n, ms = ctx.profile("k_raytrace")
            prof[k] = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=n / a.steps)
        ctx.call("sdx_profile_enable", 0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = dict(
            n_nu=int(w["nus"].size), steps_per_round=a.steps, rounds=a.rounds,
            us_per_step={k: [round(x, 2) for x in v] for k, v in times.items()},
            median_us={k: round(v, 2) for k, v in med.items()},
            plain_spread_us=round(float(np.max(times["plain"]) - np.min(times["plain"])), 2),
            extra_us=round(med["cont"] - med["plain"], 2),
            zero_line_us=round(med["zero"], 2),
            k_raytrace=prof,
        )
        res["extra_below_zero_line_synthesis"] = bool(res["extra_us"] < res["zero_line_us"])
        out[tag] = res
        print(json.dumps({tag: res}), flush=True)
        for syn in variants.values():
            syn.close()
    return out


if __name__ == "__main__":
    main()
