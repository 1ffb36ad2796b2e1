"""The CPU table behind the Ng acceleration's safeguard (tests/scattering_ng_reference.py): on every grid of NG_GRIDS at 3 and 20 angles,
for the forward and the adjoint solve, per column of NG_COLUMNS — the plain iteration's updates and status, and for each safeguard
variant the updates, status, extrapolations applied, the update at which the column was sent back to the plain iteration (0: never) and
the distance from the long-double direct solve.  fp64, the dense operator of each grid, tol = 1e-12, max_iter = 4000.
    shipped       two strikes, judged a period after each extrapolation (the forward kernel's rule)
    one strike    the rule the design started from, with the copy taken back
    every update  one strike, judged at every update of the period
    bare          no safeguard
and per variant and solve the counts of the conditions missed (tests/test_scattering_ng_cpu.py states them; condition 4, half the plain
updates at albedo >= 0.99, is asked of the forward solve alone and is counted for the adjoint for comparison).
    python scripts/scattering_ng_table.py [--out profiles/scattering_ng_classes.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scattering_adjoint_reference as A  # noqa: E402
import scattering_ng_reference as N  # noqa: E402
import scattering_reference as R  # noqa: E402

VARIANTS = {"shipped": dict(strikes=2), "one strike": dict(strikes=1), "every update": dict(strikes=1, judge="every"), "bare": dict(strikes=0)}
HIGH = ("0.99", "0.999", "0.9999", "0.99999")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = R.L
    cases, missed = [], {v: {s: dict(condition_1=0, condition_2=0, condition_3=0, condition_4=0) for s in ("forward", "adjoint")} for v in VARIANTS}
    for n, lo, hi in N.NG_GRIDS:
        for n_theta in N.NG_ANGLES:
            p = N.problem(n, lo, hi, n_theta)
            op = R.operator(p.alphas[:, :1], p.ray, p.m, np.float64)
            lam, diag, c = op.matrix()[:, :, 0], op.diagonal(), N.cotangents(n, p.n_nu)
            op80 = R.operator(p.alphas, p.ray, p.m, L)
            exact = dict(forward=R.direct_solve(op80, p.albedo.astype(L), p.B), adjoint=A.dense_solve(op80, p.albedo, c))
            for solve in ("forward", "adjoint"):
                G, x0 = N.dense_forward_G(lam, diag, p.albedo, p.B) if solve == "forward" else N.dense_adjoint_G(lam, diag, p.albedo, c)
                dist = lambda x: (np.abs(x.astype(L) - exact[solve]).max(axis=0) / np.abs(exact[solve]).max(axis=0)).astype(np.float64)  # noqa: E731
                plain = N.iterate_ng(G, x0, N.TOL, N.MAX_ITER, dict(accelerate=False))
                d_plain = dist(plain["x"])
                row = dict(points=n, tau=[lo, hi], n_theta=n_theta, solve=solve, columns=[f"{al} / {s}" for al, s in p.columns],
                           plain=dict(updates=plain["iterations"].tolist(), status=plain["status"].tolist(), distance=[float(f"{d:.3e}") for d in d_plain]))
                high = np.array([al in HIGH for al, _ in p.columns]) & (n >= 20) & (plain["status"] == 0)
                for name, opts in VARIANTS.items():
                    r = N.iterate_ng(G, x0, N.TOL, N.MAX_ITER, opts)
                    d = dist(r["x"])
                    row[name] = dict(updates=r["iterations"].tolist(), status=r["status"].tolist(), accelerations=r["accelerations"].tolist(),
                                     switched_off=r["switched_off"].tolist(), distance=[float(f"{x:.3e}") for x in d])
                    ok = plain["status"] == 0
                    m = missed[name][solve]
                    m["condition_1"] += int((ok & (r["status"] != 0)).sum())
                    m["condition_2"] += int((ok & (r["status"] == 0) & (d > 4 * d_plain)).sum())
                    m["condition_3"] += int((r["iterations"] > plain["iterations"] + 2 * N.DEFAULTS["period"]).sum())
                    m["condition_4"] += int((high & (2 * r["iterations"] > plain["iterations"])).sum())
                cases.append(row)
    res = dict(what="Ng acceleration of the scattering iterations on the CPU: updates, extrapolations, switch-offs and distance from the direct solve per "
                    "column, plain and under four safeguard variants (scripts/scattering_ng_table.py)", tol=N.TOL, max_iter=N.MAX_ITER,
               start=N.DEFAULTS["start"], period=N.DEFAULTS["period"], columns_missing_a_condition=missed, cases=cases)
    text = json.dumps(res)
    print(json.dumps(missed, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
