"""What the isolated-line equivalent widths cost: ONE process, warm, 7 alternated rounds, the median of the rounds.
  ew     SpectralSynthesizer.equivalent_widths — all 2 000 lines of S-c2 at K = 1 and K = 5 strengths (-1 ... +1 dex), a seeded 1 000-line
         subset of S-c3 at K = 1 — timed by the library's HIP events around the stage k_line_ew (sdx_profile_*), per call.
  (a)    what it replaces: a one-line SpectralSynthesizer stepped with keep_continuum_flux=True, on a seeded sample of 50 lines of the
         same selection, as recorded graph replays between two synchronisations (wall clock; the step's launches one behind the other
         without host gaps).  The figure reported for the whole selection is SCALED from the sample: mean step x lines x K.
  (b)    the yardstick: k_raytrace_cont's time per column (stage k_raytrace of a step with the continuum flux and
         segmented_raytrace = 0, HIP events) at the same depths and angles, times the number of (line, strength, point) columns the
         call walks — the lengths of the unions of the windows, from ops.line_windows on the host.  That count is reported.
No time is fixed in advance; ratio_to_yardstick = ew / (b).  Run it under a time limit; it stops at the first error.
    python scripts/line_ew_cost.py [--rounds 7] [--calls 3] [--out profiles/line_ew_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, ops, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

LN10 = float(np.log(10.0))
CASES = [("S-c2", None, 1), ("S-c2", None, 5), ("S-c3", 1000, 1)]  # workload, lines selected (None: all), strengths


def synthesizer(ctx, w, lines, **kw):
    atm = w["atm"]
    return SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], lines, w["cont"], ctx=ctx,
                               track_evaluations=False, keep_line=False, keep_total=False, **kw)


def columns_walked(w, sel, ln_s):
    """sum over (line, strength) of the length of the union over depth of the line's windows"""
    L = w["lines"]
    nd = w["atm"]["temperatures"].size
    total = 0
    for v in ln_s:
        lo, hi = ops.line_windows(nd, w["nus"], L["line_nus"][sel], L["doppler_widths"][sel], L["gammas"][sel], L["alphas"][sel] * np.exp(v))
        total += int((hi.max(axis=1) - lo.min(axis=1)).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    work, jobs = {}, []
    for tag, n_sel, k in CASES:
        if tag not in work:
            w = synth.make_workload(tag)
            full = synthesizer(ctx, w, w["lines"], keep_continuum_flux=True)
            work[tag] = (w, full)
        w, full = work[tag]
        n_lines = w["lines"]["line_nus"].size
        rng = np.random.default_rng(7)
        sel = np.arange(n_lines) if n_sel is None else np.sort(rng.choice(n_lines, n_sel, replace=False))
        ln_s = np.zeros(1) if k == 1 else np.linspace(-1.0, 1.0, k) * LN10
        sample = np.sort(rng.choice(sel, min(a.sample, sel.size), replace=False))
        ones = []
        for l in sample:
            one = {key: np.ascontiguousarray(v[l:l + 1]) for key, v in w["lines"].items()}
            syn = synthesizer(ctx, w, one, keep_continuum_flux=True)
            syn.step()
            ctx.synchronize()
            syn.capture()
            ones.append(syn)
        jobs.append(dict(tag=tag, k=k, sel=sel, ln_s=ln_s, ones=ones, full=full, w=w, ew_us=[], step_us=[], rt_us=[], columns=columns_walked(w, sel, ln_s)))
    for job in jobs:  # warm: scratch, the continuum plane, the line tables
        job["full"].equivalent_widths(lines=job["sel"], ln_strength=job["ln_s"])
        ctx.set_option("segmented_raytrace", 0)
        job["full"].step()
        ctx.set_option("segmented_raytrace", -1)
    ctx.synchronize()
    for _ in range(a.rounds):
        for job in jobs:
            full = job["full"]
            ctx.call("sdx_profile_enable", 1)
            ctx.call("sdx_profile_reset")
            for _ in range(a.calls):
                out = full.equivalent_widths(lines=job["sel"], ln_strength=job["ln_s"])
            ctx.synchronize()
            job["ew_us"].append(ctx.profile("k_line_ew")[1] * 1e3 / a.calls)
            ctx.call("sdx_profile_reset")
            ctx.set_option("segmented_raytrace", 0)  # (k_raytrace_cont itself; the one-line steps below run as the library chooses)
            for _ in range(a.calls):
                full.step()
            ctx.synchronize()
            ctx.set_option("segmented_raytrace", -1)
            job["rt_us"].append(ctx.profile("k_raytrace")[1] * 1e3 / a.calls)
            job["rt_variant"] = ctx.profile_variant("k_raytrace")
            ctx.call("sdx_profile_enable", 0)
            t0 = time.perf_counter()
            for syn in job["ones"]:
                syn.step()
            ctx.synchronize()
            job["step_us"].append((time.perf_counter() - t0) * 1e6 / len(job["ones"]))
            job["finite"] = bool(np.isfinite(out[0].numpy()).all() and np.isfinite(out[1].numpy()).all())
    results = []
    for job in jobs:
        n_nu, n_sel = int(job["w"]["nus"].size), int(job["sel"].size)
        ew, step, rt = (float(np.median(job[key])) for key in ("ew_us", "step_us", "rt_us"))
        yard = rt / n_nu * job["columns"]
        results.append(dict(workload=job["tag"], n_nu=n_nu, n_depth=int(job["w"]["atm"]["temperatures"].size), n_theta=int(job["w"]["thetas"].size),
                            lines_selected=n_sel, strengths=job["k"], columns_walked=job["columns"], columns_over_grid=round(job["columns"] / n_nu, 2),
                            ew_us_per_call=round(ew, 1), ew_us_rounds=[round(v, 1) for v in job["ew_us"]],
                            one_line_step_us=round(step, 1), one_line_steps_sampled=len(job["ones"]),
                            replaced_us_scaled_from_sample=round(step * n_sel * job["k"], 1), replaced_over_ew=round(step * n_sel * job["k"] / ew, 1),
                            raytrace_cont_us_per_step=round(rt, 1), raytrace_variant=str(job["rt_variant"]),
                            yardstick_us=round(yard, 1), ratio_to_yardstick=round(ew / yard, 2), finite=job["finite"]))
    line = json.dumps(dict(rounds=a.rounds, calls=a.calls, results=results))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
