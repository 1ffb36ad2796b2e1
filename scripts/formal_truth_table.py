"""GPU record: how far every kernel of the formal solution is from the 80-bit evaluation of the reference's formulas, next to the
double-precision oracle's own distance, per kernel label, shape and class of hostile columns (tests/formal_solution_truth.py).
Runs tests/test_gpu_formal_solution_truth.py in this process — the figures are the ones the tests assert on — and writes the largest
of each (kernel, quantity, geometry, shape, class) over the orders and runs that reached it.
python scripts/formal_truth_table.py [OUT.json]     (default: profiles/formal_truth_classes.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import formal_solution_truth as T  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_formal_solution_truth.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    worst = {}
    for label, quantity, geometry, n_depth, n_theta, _order, name, d_gpu, d_oracle in T.RECORD:
        key = (label, quantity, geometry, n_depth, n_theta, name)
        g, o, r = worst.get(key, (0.0, 0.0, 0.0))
        ratio = d_gpu / d_oracle if d_oracle and d_oracle > 0 else float("nan")
        worst[key] = (max(g, d_gpu), d_oracle if math.isnan(d_oracle) else max(o, d_oracle), r if math.isnan(ratio) else max(r, ratio))
    rows = [dict(kernel=k[0], quantity=k[1], geometry=k[2], n_depth=k[3], n_theta=k[4], column_class=k[5], kernel_distance=number(g),
                 oracle_distance=number(o), largest_ratio=number(r) if r else None) for k, (g, o, r) in sorted(worst.items())]
    doc = dict(what="distance from the 80-bit evaluation of the reference's formulas, scaled by the column's (ray's) largest value: the kernel's, "
                    "the fp64 oracle's, and the largest ratio of the two over the runs (tests/test_gpu_formal_solution_truth.py)",
               criterion=f"kernel <= {T.FACTOR:g} x oracle + {T.PER_GAP:g} x (n_depth - 1); `underflow` carries no bound; k_raytrace_f32: <= 1e-4",
               pytest_exit_code=rc, kernels=sorted({r["kernel"] for r in rows}), rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    # the worst class of every (kernel, quantity, shape)
    seen = {}
    for r in rows:
        key = (r["kernel"], r["quantity"], r["geometry"], r["n_depth"], r["n_theta"])
        if r["column_class"] != "underflow" and isinstance(r["largest_ratio"], float) and r["largest_ratio"] >= seen.get(key, (-1.0, None))[0]:
            seen[key] = (r["largest_ratio"], r)
    for key, (ratio, r) in sorted(seen.items()):
        print(f"{key[0]:42s} {key[1]:12s} {key[2]:9s} {key[3]:4d}/{key[4]:<3d} worst ratio {ratio:8.3g} in {r['column_class']} "
              f"(kernel {r['kernel_distance']}, oracle {r['oracle_distance']})")
    print("kernels:", ", ".join(doc["kernels"]))
    print("wrote", out, "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "formal_truth_classes.json")))
