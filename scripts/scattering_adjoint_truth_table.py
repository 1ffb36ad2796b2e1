"""GPU record of the scattering adjoint: per shape and class of hostile columns how far one transposed application (Lambda^T z and the
opacity derivative G) is from the 80-bit restatement (tests/scattering_adjoint_reference.py) next to the fp64 restatement's own distance;
the dot identity with the forward kernel; per grid and column the solve's outputs; and the end-to-end gaps against Richardson quotients
next to the fp64 restatement's.  Runs tests/test_gpu_scattering_adjoint.py in this process — the figures are the ones the tests assert
on — and writes the largest of each (label, quantity, shape, class or column).
python scripts/scattering_adjoint_truth_table.py [OUT.json]     (default: profiles/scattering_adjoint_truth.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import formal_solution_truth as T  # noqa: E402
import scattering_adjoint_reference as A  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_scattering_adjoint.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                          "-k", "one_application or dot_identity or solve_and_outputs or end_to_end"]))
    worst = {}
    for label, quantity, n_depth, n_theta, name, d_gpu, d_ref in A.RECORD:
        key = (label, quantity, n_depth, n_theta, str(name))
        g, o = worst.get(key, (0.0, 0.0))
        worst[key] = (max(g, d_gpu), max(o, d_ref))
    rows = []
    for k, (g, o) in sorted(worst.items()):
        allowed = 2 * o if k[0] == "end to end" else T.bound(o, k[2])
        rows.append(dict(kernel=k[0], quantity=k[1], n_depth=k[2], n_theta=k[3], column=k[4], device=number(g), restatement=number(o), allowed=number(allowed),
                         within=bool(g <= allowed)))
    doc = dict(what="the scattering adjoint on the device against the 80-bit restatement of its definitions, next to the fp64 restatement's own figure "
                    "(tests/test_gpu_scattering_adjoint.py): distances scaled by the column's largest value; `end to end`: the gap between sum_k R[k] p[k] and "
                    "a Richardson quotient of the flux, relative to sum_k |R[k] p[k]| + |flux|",
               criterion=f"device <= {T.FACTOR:g} x restatement + {T.PER_GAP:g} x (n_depth - 1); end to end: device <= 2 x restatement",
               pytest_exit_code=rc, outside=[r for r in rows if not r["within"]], rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    for r in doc["outside"]:
        print("outside the bound:", r)
    print("wrote", out, "| rows", len(rows), "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "scattering_adjoint_truth.json")))
