"""GPU record: how far k_observe and the k_observe_adjoint_* kernels are from the extended-precision evaluation of their definition, next
to the fp64 restatement's own distance and the allowance, per hostile case and quantity (tests/observe_truth.py), and the error of the
device's double-precision erf and erfc in units of 2^-53 |value| with the U chosen from it (the worst figure rounded up, plus 1).
Measures U first, then runs tests/test_gpu_observe_truth.py in this process with that U — the figures are the ones the tests assert on —
and writes the largest of each (case, quantity).
python scripts/observe_truth_table.py [OUT.json]     (default: profiles/observe_truth_classes.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import observe_truth as OT  # noqa: E402
from stardis_amd import ops  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def measure_U():
    p, a_c, b_c, a_e, b_e = OT.ulp_arguments()
    worst, where = OT.ulp_figure(p, 2.0 * ops.observe_response_grad(a_c, b_c, 0.0, 1.0)[0], 2.0 * ops.observe_response_grad(a_e, b_e, 0.0, 1.0)[0])
    return worst, where, OT.chosen_U(worst)


def main(out):
    worst, where, U = measure_U()
    try:
        before = OT.device_U()
    except (OSError, KeyError, ValueError):
        before = None
    print(f"erf / erfc on the device: worst {worst:.3f} x 2^-53 |value| at {where}; U = {U}" + ("" if before in (None, U) else f" (recorded before: {before})"))
    OT.U_OVERRIDE = U
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_observe_truth.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    best = {}
    for r in OT.RECORD:
        key = (r["case"], r["quantity"])
        if key not in best or r["worst_ratio"] > best[key]["worst_ratio"]:
            best[key] = r
    rows = [dict(case=k[0], quantity=k[1], kernel_distance=number(r["kernel"]), restatement_distance=number(r["restatement"]), allowance=number(r["allowance"]),
                 kernel_over_allowance=number(r["worst_ratio"]), within=bool(r["worst_ratio"] <= 1.0)) for k, r in sorted(best.items())]
    doc = dict(what="distance from the extended-precision evaluation of sdx_observe_dev's and sdx_observe_adjoint_dev's definitions, against the sum of the absolute "
                    "terms: the kernel's and the fp64 restatement's, the largest over a case's 16 pixels or its grid points; `allowance` is that of the element "
                    "where kernel / allowance is largest (tests/test_gpu_observe_truth.py)",
               criterion=f"kernel <= {OT.FACTOR:g} x restatement + (U Lambda / A + T + {OT.ROUNDINGS}) x 2^-53 per pixel / point",
               erf_erfc_worst_units_of_2e_minus_53=number(worst), erf_erfc_worst_at=where, U=U, pytest_exit_code=rc, outside=[r for r in rows if not r["within"]], rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    for r in doc["outside"]:
        print("outside the allowance:", r)
    print("wrote", out, "| rows", len(rows), "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "observe_truth_classes.json")))
