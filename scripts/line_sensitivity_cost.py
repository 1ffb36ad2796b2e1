"""What the per-line flux sensitivities cost: in ONE process, per workload (S-c2, S-c3), with the library's own per-stage HIP-event
timing (sdx_profile_*), after warm-up:
  (a) the line-opacity kernels of a step with far_field = 0 (k_line_all, or k_line_wide + k_line_narrow, and k_line_far — zero here):
      the direct sum, which performs the Voigt evaluations the adjoint performs;
  (b) k_response_weight and k_line_adjoint per call of SpectralSynthesizer.line_sensitivities (the six launches of sdx_line_adjoint_dev
      are one stage), per line and per (line, depth);
  (c) the same step with the far field as the library chooses it, for scale.
The target is (b) k_line_adjoint <= 2 x (a), per line and per (line, depth).  Sizes other than the workload's own (--n-nu, --n-lines) are stated in the result.
    python scripts/line_sensitivity_cost.py [--workloads S-c2,S-c3] [--calls 20] [--warmup 3] [--out profiles/line_sensitivity_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

LINE_STAGES = ("k_line_all", "k_line_wide", "k_line_narrow", "k_line_far")


def stage_us(ctx, stages, calls):
    return {s: round(ctx.profile(s)[1] * 1e3 / calls, 2) for s in stages if ctx.profile(s)[0]}


def measure(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.n_lines, n_nu_override=a.n_nu)
    atm = w["atm"]
    syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                              track_evaluations=False, keep_line=False, keep_response=True)
    res = dict(workload=tag, n_nu=int(w["nus"].size), n_depth=int(atm["temperatures"].size), n_lines=int(w["lines"]["line_nus"].size),
               full_size=a.n_lines is None and a.n_nu is None, calls=a.calls)
    weights = np.random.default_rng(1).standard_normal(w["nus"].size)
    d_weights = ctx.upload(weights)
    for far in (0, -1):
        ctx.set_option("far_field", far)
        for _ in range(a.warmup):
            syn.step()
        ctx.synchronize()
        ctx.call("sdx_profile_enable", 1)
        ctx.call("sdx_profile_reset")
        for _ in range(a.calls):
            syn.step()
        ctx.synchronize()
        res["direct_sum_step" if far == 0 else "default_step"] = stage_us(ctx, LINE_STAGES + ("k_prepass_continuum", "k_response"), a.calls)
        ctx.call("sdx_profile_enable", 0)
    direct = sum(res["direct_sum_step"].get(s, 0.0) for s in LINE_STAGES)
    for per_depth in (False, True):
        for _ in range(a.warmup):
            out = syn.line_sensitivities(d_weights, per_depth=per_depth)
        ctx.synchronize()
        ctx.call("sdx_profile_enable", 1)
        ctx.call("sdx_profile_reset")
        for _ in range(a.calls):
            out = syn.line_sensitivities(d_weights, per_depth=per_depth)
        ctx.synchronize()
        us = stage_us(ctx, ("k_line_adjoint", "k_response_weight"), a.calls)
        ctx.call("sdx_profile_enable", 0)
        us["adjoint_over_direct_sum"] = round(us["k_line_adjoint"] / direct, 3)
        res["per_depth" if per_depth else "per_line"] = us
        us["finite"] = bool(np.isfinite(out.numpy()).all())
    res["direct_sum_line_kernels_us"] = round(direct, 2)
    res["target_met"] = all(res[k]["adjoint_over_direct_sum"] <= 2.0 and res[k]["finite"] for k in ("per_line", "per_depth"))
    syn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-nu", type=int, default=None, help="n_nu_override of synth.make_workload (a reduced size is stated in the result)")
    ap.add_argument("--n-lines", type=int, default=None)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = dict(results=[measure(ctx, tag, a) for tag in a.workloads.split(",")])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
