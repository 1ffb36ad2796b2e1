"""What the response functions cost: in ONE process, alternating the variants after warm-up, with HIP-event timing on the context's
stream, at S-c2:
  (a) plain   the fused step (SpectralSynthesizer): the yardstick, the step as it is without the option
  (b) total   the same step with keep_total=True only: what (c) and (d) pay for the total_alphas plane they read
  (c) resp    the same step with keep_response=True (implies keep_total; sdx_response_dev behind the synthesis)
  (d) contr   the same step with keep_contribution=True: the companion launch, for scale
Each variant is timed in `rounds` interleaved rounds of `steps` steps, once as plain launches (eager) and once as a replayed hipGraph
(capture()); the spread of (a) across its rounds is the run-to-run spread against which the differences are read.  (c) - (b) is the
response launch itself.  A second, profiled pass reports sdx_profile_get("k_response") next to ("k_contribution") and
("k_raytrace") per step, from the same session.
    python scripts/response_cost.py [--steps 200] [--rounds 7] [--warmup 50] [--out profiles/response_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

VARIANTS = {"plain": dict(keep_total=False), "total": dict(keep_total=True), "resp": dict(keep_total=False, keep_response=True),
            "contr": dict(keep_total=False, keep_contribution=True)}


def timed_us(ctx, syn, steps):
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    for _ in range(steps):
        syn.step()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return ms.value * 1e3 / steps


def rounds_of(ctx, variants, a):
    for syn in variants.values():
        for _ in range(a.warmup):
            syn.step()
    ctx.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, syn in variants.items():
            times[k].append(timed_us(ctx, syn, a.steps))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(us_per_step={k: [round(x, 2) for x in v] for k, v in times.items()}, median_us={k: round(v, 2) for k, v in med.items()},
                plain_spread_us=round(float(np.max(times["plain"]) - np.min(times["plain"])), 2),
                response_launch_us=round(med["resp"] - med["total"], 2), contribution_launch_us=round(med["contr"] - med["total"], 2),
                keep_total_us=round(med["total"] - med["plain"], 2), extra_us=round(med["resp"] - med["plain"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="S-c2")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    w = synth.make_workload(a.workload)
    atm = w["atm"]
    args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
    common = dict(ctx=ctx, track_evaluations=False, keep_line=False)
    variants = {k: SpectralSynthesizer(*args, **kw, **common) for k, kw in VARIANTS.items()}
    res = dict(workload=a.workload, n_nu=int(w["nus"].size), n_depth=int(atm["temperatures"].size), n_theta=int(w["thetas"].size),
               steps_per_round=a.steps, rounds=a.rounds, eager=rounds_of(ctx, variants, a))
    prof = {}
    ctx.call("sdx_profile_enable", 1)
    for k, syn in variants.items():
        ctx.call("sdx_profile_reset")
        for _ in range(a.steps):
            syn.step()
        ctx.synchronize()
        prof[k] = {}
        for kernel in ("k_raytrace", "k_contribution", "k_response"):
            n, ms = ctx.profile(kernel)
            prof[k][kernel] = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=n / a.steps)
        prof[k]["raytrace_variant"] = ctx.profile_variant("k_raytrace")
    ctx.call("sdx_profile_enable", 0)
    res["profiled"] = prof
    for syn in variants.values():
        syn.capture()
    res["graph"] = rounds_of(ctx, variants, a)
    line = json.dumps(res)
    print(line, flush=True)
    for syn in variants.values():
        syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
