"""What continuum scattering costs: in ONE process, HIP-event timing on the context's stream, at S-c2 and at the S-c3 shape (S-c3's grid
and atmosphere with a short line list: the launches timed here do not depend on the lines), three things:
  (1) application   one k_lambda<false> (J alone) on the step's total_alphas, beside k_contribution<1> and k_response — the one-walk and the
                    two-walk kernels of the same layout — each as the median of `rounds` interleaved rounds of `reps` launches
  (2) iteration     sdx_scatter_source_dev with tol = 0 and an albedo of 0.9 everywhere (alpha_scatter = 0.9 total_alphas: no column stops
                    before max_iter, which the reported counts confirm) at two values of max_iter: the difference per iteration is an
                    in-kernel iteration, the intercept the staging, the diagonal and the stores; beside (1)
  (3) tail          the step with scattering=True (Thomson albedo of the model, tol = 1e-12) beside the same step without it (keep_total
                    on in both), eager and as a replayed graph; the iteration counts of the columns, their mean per wave of the launch and
                    the mean of the waves' LARGEST counts — if a wave's time is set by its slowest column, the tail's k_lambda time is
                    intercept + (mean of the waves' maxima) x the time of an iteration
    python scripts/scattering_cost.py [--reps 50] [--rounds 7] [--out profiles/scattering_cost.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402


def timed_us(ctx, fn, reps):
    _lib.check(ctx.lib.sdx_timer_start(ctx.handle))
    for _ in range(reps):
        fn()
    ms = C.c_double()
    _lib.check(ctx.lib.sdx_timer_stop(ctx.handle, C.byref(ms)))
    ctx.synchronize()
    return ms.value * 1e3 / reps


def medians(ctx, fns, reps, rounds):
    for fn in fns.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed_us(ctx, fn, reps))
    return {k: round(float(np.median(v)), 2) for k, v in times.items()}, {k: round(float(np.max(v) - np.min(v)), 2) for k, v in times.items()}


def one_workload(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.lines if tag != "S-c2" else None)
    atm = w["atm"]
    args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
    common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=True)
    plain, scat = SpectralSynthesizer(*args, **common), SpectralSynthesizer(*args, scattering=True, **common)
    for syn in (plain, scat):
        syn.step()
    ctx.synchronize()
    nd, n, nt = scat.n_depth, scat.count, scat.n_theta
    res = dict(workload=tag, n_nu=int(n), n_depth=int(nd), n_theta=int(nt), n_lines=int(w["lines"]["line_nus"].size))
    base = (nd, n, nt, scat.d_nus.ptr, scat.d_t.ptr, scat.d_ray.ptr)
    out = [ctx.empty((nd, n)) for _ in range(2)]
    # (1) one application beside the one-walk and the two-walk kernel
    fns = {
        "k_lambda<false>": lambda: ctx.call("sdx_mean_intensity_dev", *base, scat.d_mean_w.ptr, scat.d_total.ptr, n, None, 0, out[0].ptr, n, None, 0),
        "k_lambda<false> J and L": lambda: ctx.call("sdx_mean_intensity_dev", *base, scat.d_mean_w.ptr, scat.d_total.ptr, n, None, 0, out[0].ptr, n, out[1].ptr, n),
        "k_contribution<1>": lambda: ctx.call("sdx_contribution_dev", *base, scat.d_w.ptr, scat.d_total.ptr, n, None, 0, out[0].ptr, n),
        "k_response": lambda: ctx.call("sdx_response_dev", *base, scat.d_w.ptr, scat.d_total.ptr, n, None, 0, out[0].ptr, n, out[1].ptr, n),
    }
    res["application_us"], res["application_spread_us"] = medians(ctx, fns, a.reps, a.rounds)
    # (2) the time of an in-kernel iteration: at tol = 0 and albedo 0.9 no column stops before max_iter
    counts = (8, 40)
    d_scatter = ctx.upload(0.9 * scat.total_alphas())
    d_count = ctx.empty((n,), np.int32)

    def iterate(k, J):
        return lambda: ctx.call("sdx_scatter_source_dev", *base, scat.d_mean_w.ptr, scat.d_total.ptr, n, d_scatter.ptr, n, None, 0, 0.0, k, out[0].ptr, n,
                                out[1].ptr if J else None, n, d_count.ptr, None, None)

    for k in counts:
        iterate(k, False)()
        assert (d_count.numpy() == k).all(), "a column stopped early: the difference below would not be the time of an iteration"

    fns = {f"max_iter {k}": iterate(k, False) for k in counts}
    fns[f"max_iter {counts[0]} with J"] = iterate(counts[0], True)
    med, spread = medians(ctx, fns, max(a.reps // 5, 5), a.rounds)
    per_iteration = (med[f"max_iter {counts[1]}"] - med[f"max_iter {counts[0]}"]) / (counts[1] - counts[0])
    intercept = med[f"max_iter {counts[0]}"] - counts[0] * per_iteration
    res["iteration_us"] = dict(median=med, spread=spread, per_iteration=round(per_iteration, 2), intercept=round(intercept, 2),
                               final_J=round(med[f"max_iter {counts[0]} with J"] - med[f"max_iter {counts[0]}"], 2),
                               per_iteration_over_application=round(per_iteration / res["application_us"]["k_lambda<false>"], 3))
    # (3) the whole tail beside the step
    steps = {"plain": plain.step, "scattering": scat.step}
    med, spread = medians(ctx, steps, a.reps, a.rounds)
    res["step_eager_us"] = dict(median=med, spread=spread, tail=round(med["scattering"] - med["plain"], 2))
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    for _ in range(a.reps):
        scat.step()
    ctx.synchronize()
    prof = {}
    for kernel in ("k_lambda", "k_raytrace"):
        cnt, ms = ctx.profile(kernel)
        prof[kernel] = dict(us_per_step=round(ms * 1e3 / a.reps, 2), launches_per_step=cnt / a.reps)
    ctx.call("sdx_profile_enable", 0)
    res["tail_profiled"] = prof
    it = scat.scattering_iterations.astype(np.int64)
    gpw = max(1, 64 // nt)
    pad = np.concatenate([it, np.zeros((-it.size) % gpw, dtype=np.int64)]).reshape(-1, gpw)
    wave_max = float(pad.max(axis=1).mean())
    res["iterations"] = dict(min=int(it.min()), mean=round(float(it.mean()), 2), max=int(it.max()), mean_of_wave_maxima=round(wave_max, 2),
                             status_nonzero=int(np.count_nonzero(scat.scattering_status)),
                             predicted_k_lambda_us=round(intercept + res["iteration_us"]["final_J"] + wave_max * per_iteration, 2))
    F, F_lte = scat.scattering_flux.numpy(), scat.F_nu()[-1]
    res["largest_change_of_emergent_flux"] = float(np.abs(F / F_lte - 1).max())
    for syn in (plain, scat):
        syn.capture()
    med, spread = medians(ctx, steps, a.reps, a.rounds)
    res["step_graph_us"] = dict(median=med, spread=spread, tail=round(med["scattering"] - med["plain"], 2))
    for syn in (plain, scat):
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
    res = dict(what="continuum scattering: one application, one in-kernel iteration, the step's tail (scripts/scattering_cost.py)",
               reps=a.reps, rounds=a.rounds, workloads=[one_workload(ctx, tag, a) for tag in a.workloads.split(",")])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
