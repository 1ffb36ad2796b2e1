"""GPU record: how far every route of the continuum opacity is from the 80-bit evaluation of the reference's formulas, next to the
double-precision oracle's own distance, per route, source and class of hostile columns (tests/continuum_truth.py).
Runs tests/test_gpu_continuum_truth.py in this process — the figures are the ones the tests assert on — and writes, for every
(route, source, class), the largest kernel distance, the largest oracle distance, the largest ratio of the two, the operation count of
the bound and the routes (kernel, tiled, depths per block, table in LDS, planned) that the tests asserted when they reached it.
python scripts/continuum_truth_table.py [OUT.json]     (default: profiles/continuum_truth_classes.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import continuum_truth as T  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_continuum_truth.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    worst = {}
    for r in T.RECORD:
        key = (r["route"], r["source"], r["cls"])
        w = worst.setdefault(key, dict(kernel=0.0, oracle=0.0, ratio=0.0, n_ops=0, bound=0.0, cases=set(), ran=set()))
        w["kernel"], w["oracle"] = max(w["kernel"], r["kernel"]), max(w["oracle"], r["oracle"])
        if r["oracle"] > 0:
            w["ratio"] = max(w["ratio"], r["kernel"] / r["oracle"])
        w["n_ops"], w["bound"] = max(w["n_ops"], r["n_ops"]), max(w["bound"], r["bound"])
        w["cases"].add(r["case"])
        if r["ran"]:
            k = r["ran"]
            w["ran"].add((k["kernel"], k["tiled"], k["depths_per_block"], k["table_in_lds"], k["planned"]))
    rows = [dict(route=k[0], source=k[1], column_class=k[2], kernel_distance=number(w["kernel"]), oracle_distance=number(w["oracle"]),
                 largest_ratio=number(w["ratio"]) if w["ratio"] else None, n_ops=w["n_ops"], largest_bound=number(w["bound"]), cases=len(w["cases"]),
                 asserted=[dict(kernel=a, tiled=b, depths_per_block=c, table_in_lds=d, planned=e) for a, b, c, d, e in sorted(w["ran"])])
            for k, w in sorted(worst.items())]
    doc = dict(what="pointwise distance from the 80-bit evaluation of the reference's continuum formulas, relative to it: the kernel's, the fp64 "
                    "oracle's, and the largest ratio of the two over the cases of a class (tests/test_gpu_continuum_truth.py); routes A stand-alone "
                    "sources, B stand-alone sum, C fused untiled, D fused tiles, E planned tiles, F tiles riding the classification launch",
               criterion=f"kernel <= {T.FACTOR:g} x oracle + n_ops x 2^-53 at every point; zeros, NaNs and infinities where the truth has them; every "
                         "route gives route B's bits",
               pytest_exit_code=rc, routes=sorted({r["route"] for r in rows}), rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    for route in doc["routes"]:
        mine = [r for r in rows if r["route"] == route and isinstance(r["largest_ratio"], float)]
        if mine:
            r = max(mine, key=lambda r: r["largest_ratio"])
            ran = sorted({(a["depths_per_block"], a["table_in_lds"]) for q in rows if q["route"] == route for a in q["asserted"]})
            print(f"route {route}: worst ratio {r['largest_ratio']:.3g} in {r['column_class']} / {r['source']} (kernel {r['kernel_distance']}, "
                  f"oracle {r['oracle_distance']}); (depths per block, table in LDS) asserted: {ran}")
    print("wrote", out, "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "continuum_truth_classes.json")))
