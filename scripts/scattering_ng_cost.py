"""What Ng acceleration of the scattering source iteration buys and costs: in ONE process, plain and accelerated alternating, HIP-event
timing on the context's stream, at S-c2 and at the S-c3 shape (S-c3's grid and atmosphere with a short line list: the launches timed
here do not depend on the lines), on the step's own total_alphas:
  (1) solve     sdx_scatter_source_dev beside sdx_scatter_source_ng_dev at tol = 1e-12 with a uniform albedo 0.5 / 0.9 / 0.99 / 0.999
                (alpha_scatter = albedo x total_alphas) and with the model's own Thomson opacity: updates (min, mean, max over the
                columns, and the mean of the waves' largest counts, which sets the launch's time), extrapolations, columns the safeguard
                may have sent back (not reported by the kernel: columns with fewer extrapolations than their count allows), the time of
                a solve as the median of `rounds` interleaved rounds of `reps` launches, and the largest difference of the two S.
                At the Thomson albedo no column reaches the first extrapolation: the two times there are the accelerated kernel's pure
                overhead.
  (2) update    one in-kernel update of each kernel: tol = 0 at albedo 0.9, max_iter 8 and 24, the difference per update (24, not the
                plain script's 40: by update 40 an accelerated column can sit on its rounding floor with a change of exactly 0 and stop) — the
                accelerated one includes the ring write of every update and an extrapolation (five sums, the new column) every fourth.
The adjoint solve has no accelerated kernel ("The scattering adjoint"): nothing of it is timed here.
    python scripts/scattering_ng_cost.py [--reps 20] [--rounds 7] [--out profiles/scattering_ng_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.scattering_cost import medians  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402

ALBEDOS = (0.5, 0.9, 0.99, 0.999)
TOL, MAX_ITER, START, PERIOD = 1e-12, 4000, 4, 4


def counts(it, gpw):
    it = it.astype(np.int64)
    pad = np.concatenate([it, np.zeros((-it.size) % gpw, dtype=np.int64)]).reshape(-1, gpw)
    return dict(min=int(it.min()), mean=round(float(it.mean()), 2), max=int(it.max()), mean_of_wave_maxima=round(float(pad.max(axis=1).mean()), 2))


def one_workload(ctx, tag, a):
    w = synth.make_workload(tag, n_lines=a.lines if tag != "S-c2" else None)
    atm = w["atm"]
    syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx, track_evaluations=False,
                              keep_line=False, keep_total=True, scattering=True)
    syn.step()
    ctx.synchronize()
    nd, n, nt = syn.n_depth, syn.count, syn.n_theta
    gpw = max(1, 64 // nt)
    res = dict(workload=tag, n_nu=int(n), n_depth=int(nd), n_theta=int(nt), solves=[])
    base = (nd, n, nt, syn.d_nus.ptr, syn.d_t.ptr, syn.d_ray.ptr, syn.d_mean_w.ptr, syn.d_total.ptr, n)
    S = {k: ctx.empty((nd, n)) for k in ("plain", "ng")}
    it = {k: ctx.empty((n,), np.int32) for k in ("plain", "ng")}
    st = {k: ctx.empty((n,), np.int32) for k in ("plain", "ng")}
    acc = ctx.empty((n,), np.int32)
    total = syn.total_alphas()

    def calls(scatter_ptr, scatter_ld, tol, max_iter):
        tail = lambda k: (scatter_ptr, scatter_ld, None, 0, tol, max_iter, S[k].ptr, n, None, 0, it[k].ptr, st[k].ptr, None)  # noqa: E731
        return {"plain": lambda: ctx.call("sdx_scatter_source_dev", *base, *tail("plain")),
                "ng": lambda: ctx.call("sdx_scatter_source_ng_dev", *base, *tail("ng"), START, PERIOD, acc.ptr)}

    cases = [(f"albedo {x}", ctx.upload(x * total), n) for x in ALBEDOS] + [("Thomson", syn.d_thomson, 0)]
    for name, d_scatter, ld in cases:
        fns = calls(d_scatter.ptr, ld, TOL, MAX_ITER)
        med, spread = medians(ctx, fns, a.reps, a.rounds)
        Sp, Sn = S["plain"].numpy(), S["ng"].numpy()
        accs, it_ng = acc.numpy().astype(np.int64), it["ng"].numpy().astype(np.int64)
        due = np.maximum((it_ng - 1) // PERIOD, 0)  # extrapolations a column that was never sent back nor skipped has had
        res["solves"].append(dict(case=name, updates_plain=counts(it["plain"].numpy(), gpw), updates_ng=counts(it_ng, gpw),
                                  status_nonzero=dict(plain=int(np.count_nonzero(st["plain"].numpy())), ng=int(np.count_nonzero(st["ng"].numpy()))),
                                  accelerations=dict(min=int(accs.min()), mean=round(float(accs.mean()), 2), max=int(accs.max())),
                                  columns_below_their_due=int(np.count_nonzero(accs < due)),
                                  solve_us=med, solve_spread_us=spread, speedup=round(med["plain"] / med["ng"], 3),
                                  largest_difference_of_S=float(np.abs(Sn / Sp - 1).max())))
    # (2) one in-kernel update of each kernel
    d_scatter = ctx.upload(0.9 * total)
    per = {}
    for k in (8, 24):
        fns = calls(d_scatter.ptr, n, 0.0, k)
        for fn in fns.values():
            fn()
        assert (it["plain"].numpy() == k).all() and (it["ng"].numpy() == k).all(), "a column stopped early"
        per[k], _ = medians(ctx, fns, a.reps, a.rounds)
    res["update_us"] = {key: round((per[24][key] - per[8][key]) / 16, 2) for key in ("plain", "ng")}
    res["update_us"]["intercept"] = {key: round(per[8][key] - 8 * (per[24][key] - per[8][key]) / 16, 2) for key in ("plain", "ng")}
    res["update_us"]["ng_over_plain"] = round(res["update_us"]["ng"] / res["update_us"]["plain"], 3)
    syn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lines", type=int, default=2000, help="lines of the S-c3 shape's list")
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = dict(what="Ng acceleration of the scattering source iteration beside the plain one: updates and time per solve, one in-kernel update "
                    "(scripts/scattering_ng_cost.py)", tol=TOL, max_iter=MAX_ITER, start=START, period=PERIOD, reps=a.reps, rounds=a.rounds,
               workloads=[one_workload(ctx, tag, a) for tag in a.workloads.split(",")])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
