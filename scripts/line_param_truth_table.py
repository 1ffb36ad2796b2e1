"""The measured distances of the line-profile sensitivities from their truth, as tests/test_gpu_voigt_grad.py and
tests/test_gpu_line_param_adjoint.py measure them (their own functions are called here), written to
profiles/line_param_truth_classes.json:
  points   per point set (G1, G2, the region boundaries) and Humlicek region: the worst |got - truth| / |w'| of K_x and K_y from
           sdx_voigt_grad_dev, the yardstick's (the same formulas in complex128), what is allowed, and K against the reference's Re w;
  sums     per model of tests/line_adjoint_truth.py and output: the worst |got - ref| / bound per (line, depth) item and per line.
    python scripts/line_param_truth_table.py [--out profiles/line_param_truth_classes.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_line_param_adjoint as S  # noqa: E402
import test_gpu_voigt_grad as G  # noqa: E402
from stardis_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_param_truth_classes.json"))
    a = ap.parse_args()
    ctx = _lib.default_context()
    res = dict(points={which: {f"region {r}": v for r, v in G.measure(which).items()} for which in ("g1", "g2", "boundaries")}, sums={})
    for name in S.NAMES:
        m, r = S.T.model(name), S.restated(name)
        got = S.param_adjoint(ctx, m)
        row = {}
        for k in S.KEYS:
            q = getattr(r, k)
            per_item = np.abs(got[k][1] - q.s_ld) / np.where(q.scale_ld > 0, S.T.bound(q.scale_ld, q.terms_ld), 1.0)
            per_line = np.abs(got[k][0] - q.s_l) / np.where(q.scale_l > 0, S.T.bound(q.scale_l, q.terms_l), 1.0)
            row[k] = dict(worst_over_bound_per_item=float(per_item.max()), worst_over_bound_per_line=float(per_line.max()))
        row["items"], row["longest_window"] = int(r.damping.terms_ld.size), int(r.damping.terms_ld.max())
        res["sums"][name] = row
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
