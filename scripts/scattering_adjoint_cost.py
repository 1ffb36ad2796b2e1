"""What the scattering adjoint costs: in ONE process, HIP-event timing on the context's stream, at S-c2 and at the S-c3 shape (S-c3's
grid and atmosphere with a short line list: the launches timed here do not depend on the lines), beside the forward kernels in the
same rounds:
  (1) application     one k_lambda_adjoint<false> (Lambda^T z alone) beside k_lambda<false> (J alone) and k_response
  (2) differentiated  k_lambda_adjoint<false> with G alone (a forward sweep with stash and a reverse walk, per sweep) beside the same
  (3) iteration       sdx_scatter_response_dev (y alone: no differentiated pass) and sdx_scatter_source_dev with tol = 0 and an albedo of
                      0.9 everywhere at two values of max_iter: the difference per iteration is an in-kernel iteration of either
  (4) tail            the step with scattering=True and keep_response=True (the model's Thomson albedo, tol = 1e-12) beside the step
                      with scattering=True alone and with keep_response=True alone, eager; the profiled time of k_lambda_adjoint per
                      step, and the adjoint's iteration counts beside the forward solve's
    python scripts/scattering_adjoint_cost.py [--reps 50] [--rounds 7] [--out profiles/scattering_adjoint_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scattering_cost import medians  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402


def one_workload(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.lines if tag != "S-c2" else None)
    atm = w["atm"]
    args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
    common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=True)
    scat = SpectralSynthesizer(*args, scattering=True, **common)
    resp = SpectralSynthesizer(*args, keep_response=True, **common)
    both = SpectralSynthesizer(*args, scattering=True, keep_response=True, **common)
    for syn in (scat, resp, both):
        syn.step()
    ctx.synchronize()
    nd, n, nt = both.n_depth, both.count, both.n_theta
    res = dict(workload=tag, n_nu=int(n), n_depth=int(nd), n_theta=int(nt), n_lines=int(w["lines"]["line_nus"].size))
    base = (nd, n, nt, both.d_nus.ptr, both.d_t.ptr, both.d_ray.ptr)
    total, S, z = both.d_total.ptr, both.d_Ssc.ptr, both.d_sc_cotangent.ptr
    out = [ctx.empty((nd, n)) for _ in range(2)]
    fns = {
        "k_lambda<false>": lambda: ctx.call("sdx_mean_intensity_dev", *base, both.d_mean_w.ptr, total, n, S, n, out[0].ptr, n, None, 0),
        "k_response": lambda: ctx.call("sdx_response_dev", *base, both.d_w.ptr, total, n, S, n, out[0].ptr, n, out[1].ptr, n),
        "k_lambda_adjoint<false> Lt": lambda: ctx.call("sdx_mean_intensity_adjoint_dev", *base, both.d_mean_w.ptr, total, n, z, n, S, n, out[0].ptr, n, None, 0),
        "k_lambda_adjoint<false> G": lambda: ctx.call("sdx_mean_intensity_adjoint_dev", *base, both.d_mean_w.ptr, total, n, z, n, S, n, None, 0, out[1].ptr, n),
    }
    med, spread = medians(ctx, fns, a.reps, a.rounds)
    res["application_us"], res["application_spread_us"] = med, spread
    res["application_ratio"] = dict(transposed_over_forward=round(med["k_lambda_adjoint<false> Lt"] / med["k_lambda<false>"], 3),
                                    differentiated_over_k_response=round(med["k_lambda_adjoint<false> G"] / med["k_response"], 3))
    # the time of an in-kernel iteration of either solve: at tol = 0 and albedo 0.9 no column stops before max_iter
    counts = (8, 40)
    d_scatter = ctx.upload(0.9 * both.total_alphas())
    d_count = ctx.empty((n,), np.int32)

    def forward(k):
        return lambda: ctx.call("sdx_scatter_source_dev", *base, both.d_mean_w.ptr, total, n, d_scatter.ptr, n, None, 0, 0.0, k, out[0].ptr, n, None, 0,
                                d_count.ptr, None, None)

    def adjoint(k):
        return lambda: ctx.call("sdx_scatter_response_dev", *base, both.d_mean_w.ptr, total, n, d_scatter.ptr, n, None, 0, S, n, z, n, None, 0, 0.0, k,
                                out[0].ptr, n, None, 0, None, 0, None, 0, d_count.ptr, None, None)

    for k in counts:
        for fn in (forward, adjoint):
            fn(k)()
            assert (d_count.numpy() == k).all(), "a column stopped early: the difference below would not be the time of an iteration"
    fns = {f"{name} max_iter {k}": fn(k) for name, fn in (("k_lambda<true>", forward), ("k_lambda_adjoint<true>", adjoint)) for k in counts}
    med, spread = medians(ctx, fns, max(a.reps // 5, 5), a.rounds)
    per = {name: (med[f"{name} max_iter {counts[1]}"] - med[f"{name} max_iter {counts[0]}"]) / (counts[1] - counts[0]) for name in ("k_lambda<true>", "k_lambda_adjoint<true>")}
    res["iteration_us"] = dict(median=med, spread=spread, per_iteration={k: round(v, 2) for k, v in per.items()},
                               intercept={k: round(med[f"{k} max_iter {counts[0]}"] - counts[0] * v, 2) for k, v in per.items()},
                               adjoint_over_forward=round(per["k_lambda_adjoint<true>"] / per["k_lambda<true>"], 3))
    # the whole tail
    steps = {"scattering": scat.step, "keep_response": resp.step, "scattering and keep_response": both.step}
    med, spread = medians(ctx, steps, a.reps, a.rounds)
    res["step_eager_us"] = dict(median=med, spread=spread, tail=round(med["scattering and keep_response"] - med["scattering"], 2))
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    for _ in range(a.reps):
        both.step()
    ctx.synchronize()
    prof = {}
    for kernel in ("k_lambda", "k_lambda_adjoint", "k_response"):
        cnt, ms = ctx.profile(kernel)
        prof[kernel] = dict(us_per_step=round(ms * 1e3 / a.reps, 2), launches_per_step=cnt / a.reps)
    ctx.call("sdx_profile_enable", 0)
    res["tail_profiled"] = prof
    res["tail_ratio"] = dict(adjoint_over_forward_solve=round(prof["k_lambda_adjoint"]["us_per_step"] / prof["k_lambda"]["us_per_step"], 3))
    fw, ad = both.scattering_iterations.astype(np.int64), both.scattering_response_iterations.astype(np.int64)
    res["iterations"] = dict(forward=dict(min=int(fw.min()), mean=round(float(fw.mean()), 2), max=int(fw.max())),
                             adjoint=dict(min=int(ad.min()), mean=round(float(ad.mean()), 2), max=int(ad.max())),
                             status_nonzero=int(np.count_nonzero(both.scattering_response_status)))
    for syn in (scat, resp, both):
        syn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lines", type=int, default=2000, help="lines of the S-c3 shape's list")
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = dict(what="the scattering adjoint: one transposed application, the differentiated pass, one in-kernel iteration and the step's tail, beside "
                    "k_lambda<false>, k_lambda<true> and k_response in the same rounds (scripts/scattering_adjoint_cost.py)",
               reps=a.reps, rounds=a.rounds, workloads=[one_workload(ctx, tag, a) for tag in a.workloads.split(",")])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
