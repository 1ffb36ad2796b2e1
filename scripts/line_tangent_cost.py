"""What the tangent of the line-opacity sum costs: in ONE process, per workload (S-c2, S-c3), HIP-event timed (the library's per-stage
sdx_profile_* for the kernels, sdx_timer_* for whole regions), after warm-up, alternating so that the rivals see the same clocks:
  (a) k_line_tangent per call of SpectralSynthesizer.line_tangent — all four directions per (line, depth), and strength alone per line
      (the five launches of sdx_line_tangent_dev are one stage) — beside the line kernel of a step on a context with far_field = 0
      (k_line_all: the same terms by the direct sum, without the gradient rationals);
  (b) the same beside k_line_param_adjoint per call of line_sensitivities(per_depth=True, wrt=("damping", "doppler", "centre")): the same
      evaluations, plus a weight load and reductions;
  (c) one column of observed_line_jacobian — "X": strength = a 0 / 1 mask over every tenth line, and "xi": the microturbulence — as a
      whole region (direction upload, tangent, projection, instrument) beside TWO whole default steps, the central difference it
      replaces.
Nobody has measured these before, so there is no threshold: the figures are the ratios within the session.  The wide items (half-width
above 256 grid points: walked by every tile of their depth) and the others say where the terms are.  Sizes other than the workload's own
(--n-nu, --n-lines) are stated in the result.
    python scripts/line_tangent_cost.py [--workloads S-c2,S-c3] [--calls 10] [--warmup 2] [--out profiles/line_tangent_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from observe_cost import pixels  # noqa: E402
from stardis_amd import _lib, ops, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import Instrument  # noqa: E402

SHAPE = ("damping", "doppler", "centre")
LINE_STAGES = ("k_line_all", "k_line_narrow", "k_line_wide")
WIDE = 256  # kTanWide


def stage_us(ctx, stages, calls, warmup, call):
    """microseconds per call recorded under the stage names, over `calls` profiled calls"""
    for _ in range(warmup):
        call()
    ctx.synchronize()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    for _ in range(calls):
        call()
    ctx.synchronize()
    got = [ctx.profile(s) for s in stages]
    ctx.call("sdx_profile_enable", 0)
    assert sum(n for n, _ in got) >= calls, (stages, got)
    return round(sum(ms for _, ms in got) * 1e3 / calls, 2)


def region_us(ctx, calls, warmup, call):
    """microseconds per call between two events around `calls` calls: everything the calls put on the stream, and its gaps"""
    for _ in range(warmup):
        call()
    ctx.synchronize()
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    for _ in range(calls):
        call()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return round(ms.value * 1e3 / calls, 2)


def classes(w, n_depth):
    L = w["lines"]
    lo, hi = ops.line_windows(n_depth, w["nus"], L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"])
    length = (hi - lo).astype(np.int64)
    d_nu = -np.diff(w["nus"]).max()
    g = L["gammas"] if L["gammas"].shape[1] > 1 else np.broadcast_to(L["gammas"], L["alphas"].shape)
    half = np.maximum(10, (g + L["doppler_widths"]) * L["alphas"] / d_nu * 20)
    wide = half >= WIDE + 1
    return {name: dict(items=int(m.sum()), terms=int(length[m].sum())) for name, m in (("wide", wide), ("others", ~wide))}


def measure(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.n_lines, n_nu_override=a.n_nu)
    atm, L = w["atm"], w["lines"]
    n_depth, n_lines = int(atm["temperatures"].size), int(L["line_nus"].size)
    make = lambda **kw: SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], L, w["cont"], ctx=ctx,  # noqa: E731
                                            track_evaluations=False, keep_line=False, **kw)
    res = dict(workload=tag, n_nu=int(w["nus"].size), n_depth=n_depth, n_lines=n_lines, full_size=a.n_lines is None and a.n_nu is None,
               calls=a.calls, classes=classes(w, n_depth))
    # the yardstick: the default step, and its line kernel on a context without the far field
    plain = make(keep_total=False)
    res["step_us"] = [region_us(ctx, a.calls, a.warmup, plain.step)]
    ctx.set_option("far_field", 0)
    try:
        direct = make(keep_total=False)
        res["k_line_all_far_field_0_us"] = [stage_us(ctx, LINE_STAGES, a.calls, a.warmup, direct.step)]
        direct.close()
    finally:
        ctx.set_option("far_field", -1)
    lam = K.nu_to_angstrom(w["nus"])
    edges, R = pixels(tag, lam)
    syn = make(keep_response=True, instrument=Instrument(edges, resolving_power=R, ctx=ctx))
    syn.step()
    ctx.synchronize()
    rng = np.random.default_rng(1)
    four = {k: rng.standard_normal((n_lines, n_depth)) for k in ("strength", "damping", "doppler")}
    four["centre"] = rng.standard_normal((n_lines, n_depth)) * float(np.median(L["doppler_widths"]))
    d_weights = ctx.upload(rng.standard_normal(w["nus"].size))
    mask = (np.arange(n_lines) % 10 == 0).astype(np.float64)
    xi_direction = 1.5e5 * (L["line_nus"] / K.C_CGS)[:, None] ** 2 / L["doppler_widths"] ** 2  # what the "xi" column moves the lines along
    rows = {"k_line_tangent_four_us": lambda: syn.line_tangent(**four), "k_line_tangent_strength_us": lambda: syn.line_tangent(strength=1.0),
            "k_line_tangent_mask_tenth_us": lambda: syn.line_tangent(strength=mask), "k_line_tangent_xi_us": lambda: syn.line_tangent(doppler=xi_direction)}
    for rep in range(2):  # alternate
        for key, call in rows.items():
            res.setdefault(key, []).append(stage_us(ctx, ("k_line_tangent",), a.calls, a.warmup, call))
        res.setdefault("k_line_param_adjoint_us", []).append(stage_us(ctx, ("k_line_param_adjoint",), a.calls, a.warmup,
                                                                      lambda: syn.line_sensitivities(d_weights, per_depth=True, wrt=SHAPE)))
        res.setdefault("column_X_us", []).append(region_us(ctx, a.calls, a.warmup, lambda: syn.observed_line_jacobian({"X": dict(strength=mask)})))
        res.setdefault("column_xi_us", []).append(region_us(ctx, a.calls, a.warmup, lambda: syn.observed_line_jacobian({"xi": dict(microturbulence=1.5e5)})))
        res["step_us"].append(region_us(ctx, a.calls, a.warmup, plain.step))
    res["finite"] = bool(np.isfinite(syn.line_tangent(**four).numpy()).all() and np.isfinite(syn.flux_tangent(strength=mask).numpy()).all())
    best = {k: min(v) for k, v in res.items() if isinstance(v, list)}
    res["tangent_four_over_line_all"] = round(best["k_line_tangent_four_us"] / best["k_line_all_far_field_0_us"], 3)
    res["tangent_strength_over_line_all"] = round(best["k_line_tangent_strength_us"] / best["k_line_all_far_field_0_us"], 3)
    res["tangent_four_over_param_adjoint"] = round(best["k_line_tangent_four_us"] / best["k_line_param_adjoint_us"], 3)
    res["column_X_over_two_steps"] = round(best["column_X_us"] / (2 * best["step_us"]), 3)
    res["column_xi_over_two_steps"] = round(best["column_xi_us"] / (2 * best["step_us"]), 3)
    syn.close()
    plain.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-nu", type=int, default=None, help="n_nu_override of synth.make_workload (a reduced size is stated in the result)")
    ap.add_argument("--n-lines", type=int, default=None)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = dict(results=[])
    for tag in a.workloads.split(","):
        res["results"].append(measure(ctx, tag, a))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
