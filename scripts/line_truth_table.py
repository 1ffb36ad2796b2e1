"""GPU record: how far every route of the line path is from the extended-precision evaluation of the reference's own sum, point by point
and relative to it, next to the double-precision oracle's own distance and the share of terms left out of the tight comparison because
they hug a Humlicek boundary — per route, hostile list and shape (tests/line_opacity_truth.py).  Runs
tests/test_gpu_line_opacity_truth.py in this process — the figures are the ones the tests assert on — and writes the largest of each
(route, list, shape).
python scripts/line_truth_table.py [OUT.json]     (default: profiles/line_truth_classes.json)"""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import line_opacity_truth as T  # noqa: E402


def number(v):
    return float(f"{v:.3e}")


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_line_opacity_truth.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    worst = {}
    for r in T.RECORD:
        key = (r["route"], r["case"], r["n_depth"], r["n_nu"], r["n_lines"])
        k, o, e = worst.get(key, (0.0, 0.0, 0.0))
        worst[key] = (max(k, r["kernel"]), max(o, r["oracle"]), max(e, r["excluded_share"]))
    rows = [dict(route=key[0], list=key[1], line_class=T.case(key[1]).cls, n_depth=key[2], n_nu=key[3], n_lines=key[4], kernel_distance=number(k),
                 oracle_distance=number(o), excluded_share=number(e)) for key, (k, o, e) in sorted(worst.items())]
    doc = dict(what="largest pointwise distance from the extended-precision evaluation of the reference's line-opacity sum, relative to it: the "
                    "kernel's and the fp64 oracle's, outside the points where a term lies within 1e-12 of a Humlicek boundary (excluded_share "
                    "of the terms; the mixed mode: within 1e-4) (tests/test_gpu_line_opacity_truth.py)",
               criterion=f"kernel <= {T.FACTOR:g} x oracle + {T.TERM:g} (+ {T.FAR_VS_DIRECT:g} with the far field); mixed_precision: <= {T.MIXED_LINE:g}",
               pytest_exit_code=rc, routes=sorted({r["route"] for r in rows}), rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    by_route = {}
    for r in rows:
        if r["kernel_distance"] >= by_route.get(r["route"], (-1.0, None))[0]:
            by_route[r["route"]] = (r["kernel_distance"], r)
    for route, (k, r) in sorted(by_route.items()):
        print(f"{route:40s} worst {k:9.3g} on {r['list']} (oracle {r['oracle_distance']})")
    print("wrote", out, "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "line_truth_classes.json")))
