"""What the line-profile sensitivities cost beside the strength adjoint: in ONE process, per workload (S-c2, S-c3), with the library's own
per-stage HIP-event timing (sdx_profile_*), after warm-up, alternating so that both see the same clocks:
  (a) k_line_adjoint per call of SpectralSynthesizer.line_sensitivities(wrt="strength") (the six launches of sdx_line_adjoint_dev are one
      stage);
  (b) k_line_param_adjoint per call of line_sensitivities(wrt=("damping", "doppler", "centre")) (the six launches of
      sdx_line_param_adjoint_dev), per line and per (line, depth), and with one output only (wrt="damping": the same sums, fewer stores).
Nobody has measured (b) before, so there is no threshold: the figure is the ratio (b) / (a) in the same session.  The items per class
(short: four lanes per item, long: a wave per item, tiled: the transpose of the wide role) say where the terms are.  Sizes other than the
workload's own (--n-nu, --n-lines) are stated in the result.
    python scripts/line_param_sensitivity_cost.py [--workloads S-c2,S-c3] [--calls 20] [--warmup 3] [--out profiles/line_param_sensitivity_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, ops, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

SHAPE = ("damping", "doppler", "centre")


def timed(ctx, stage, calls, warmup, call):
    for _ in range(warmup):
        out = call()
    ctx.synchronize()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    for _ in range(calls):
        out = call()
    ctx.synchronize()
    n, ms = ctx.profile(stage)
    ctx.call("sdx_profile_enable", 0)
    assert n == calls, (stage, n, calls)
    outs = out.values() if isinstance(out, dict) else [out]
    return round(ms * 1e3 / calls, 2), bool(all(np.isfinite(o.numpy()).all() for o in outs))


def classes(w, n_depth):
    """items per class of the adjoint's plan, from the windows (short: half-width <= 64; tiled: more than 4096 points)"""
    L = w["lines"]
    lo, hi = ops.line_windows(n_depth, w["nus"], L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"])
    length = (hi - lo).astype(np.int64)
    d_nu = -np.diff(w["nus"]).max()
    g = L["gammas"] if L["gammas"].shape[1] > 1 else np.broadcast_to(L["gammas"], L["alphas"].shape)
    half = np.maximum(10, (g + L["doppler_widths"]) * L["alphas"] / d_nu * 20).astype(np.int64)
    short, tiled = half <= 64, (half > 64) & (length > 4096)
    long_ = ~short & ~tiled
    return {name: dict(items=int(m.sum()), terms=int(length[m].sum())) for name, m in (("short", short), ("long", long_), ("tiled", tiled))}


def measure(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.n_lines, n_nu_override=a.n_nu)
    atm = w["atm"]
    syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                              track_evaluations=False, keep_line=False, keep_response=True)
    n_depth = int(atm["temperatures"].size)
    res = dict(workload=tag, n_nu=int(w["nus"].size), n_depth=n_depth, n_lines=int(w["lines"]["line_nus"].size),
               full_size=a.n_lines is None and a.n_nu is None, calls=a.calls, classes=classes(w, n_depth))
    d_weights = ctx.upload(np.random.default_rng(1).standard_normal(w["nus"].size))
    syn.step()
    ctx.synchronize()
    for per_depth in (False, True):
        row = {}
        for rep in range(2):  # alternate: strength, shape, strength, shape
            row.setdefault("k_line_adjoint_us", []).append(timed(ctx, "k_line_adjoint", a.calls, a.warmup, lambda: syn.line_sensitivities(d_weights, per_depth=per_depth)))
            row.setdefault("k_line_param_adjoint_us", []).append(timed(ctx, "k_line_param_adjoint", a.calls, a.warmup, lambda: syn.line_sensitivities(d_weights, per_depth=per_depth, wrt=SHAPE)))
        row["k_line_param_adjoint_damping_only_us"] = [timed(ctx, "k_line_param_adjoint", a.calls, a.warmup, lambda: syn.line_sensitivities(d_weights, per_depth=per_depth, wrt="damping"))]
        out = {k: [v[0] for v in vals] for k, vals in row.items()}
        out["finite"] = all(v[1] for vals in row.values() for v in vals)
        out["param_over_strength"] = round(min(out["k_line_param_adjoint_us"]) / min(out["k_line_adjoint_us"]), 3)
        res["per_depth" if per_depth else "per_line"] = out
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
