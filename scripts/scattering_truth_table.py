"""GPU record: how far one application of k_lambda (J and the diagonal L) is from the 80-bit restatement of the definition, next to the
fp64 restatement's own distance, per shape and class of hostile columns (tests/scattering_reference.py).  Runs
tests/test_gpu_scattering.py in this process — the figures are the ones the tests assert on — and writes the largest of each
(kernel label, quantity, shape, class) over the runs that reached it.
python scripts/scattering_truth_table.py [OUT.json]     (default: profiles/scattering_truth_classes.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import formal_solution_truth as T  # noqa: E402
import scattering_reference as R  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_scattering.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k", "one_application"]))
    worst = {}
    for label, quantity, n_depth, n_theta, name, d_gpu, d_ref in R.RECORD:
        key = (label, quantity, n_depth, n_theta, name)
        g, o = worst.get(key, (0.0, 0.0))
        worst[key] = (max(g, d_gpu), max(o, d_ref))
    rows = [dict(kernel=k[0], quantity=k[1], n_depth=k[2], n_theta=k[3], column_class=k[4], kernel_distance=number(g), restatement_distance=number(o),
                 bound=number(T.bound(o, k[2])), within=bool(k[4] == "underflow" or g <= T.bound(o, k[2]))) for k, (g, o) in sorted(worst.items())]
    doc = dict(what="distance from the 80-bit restatement of sdx_mean_intensity_dev's definition, scaled by the column's largest value: the kernel's and "
                    "the fp64 restatement's (tests/test_gpu_scattering.py, 16 columns per class)",
               criterion=f"kernel <= {T.FACTOR:g} x restatement + {T.PER_GAP:g} x (n_depth - 1); `underflow` carries no bound",
               pytest_exit_code=rc, outside=[r for r in rows if not r["within"]], rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    for r in doc["outside"]:
        print("outside the bound:", r)
    print("wrote", out, "| rows", len(rows), "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "scattering_truth_classes.json")))
