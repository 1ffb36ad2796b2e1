"""GPU record: how far every route of the line parameters (gamma, Doppler width, alpha_line) is from the 80-bit evaluation of the
reference's formulas, per class of hostile lines and route (tests/line_params_truth.py).
Runs tests/test_gpu_line_params_truth.py in this process — the figures are the ones the tests assert on — and writes, for every (class,
route, quantity), the largest distance from the truth in units of 2^-53 |truth|, that distance as a share of bound(), the fp64 oracle's
own largest distance, and the value of LIB (the roundings a pow, log or tgamma of the device library is counted as) the bound was
formed with: the measured numbers a later change can tighten LIB from.
python scripts/line_params_truth_table.py [OUT.json]     (default: profiles/line_params_truth_classes.json)"""
import json
import math
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pytest  # noqa: E402

import line_params_truth as T  # noqa: E402


def number(v):
    return None if v is None or math.isnan(v) else (float(f"{v:.3e}") if math.isfinite(v) else str(v))


def main(out):
    rc = int(pytest.main([os.path.join(root, "tests", "test_gpu_line_params_truth.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    worst = {}
    for r in T.RECORD:
        key = (r["cls"], r["route"], r["what"] if r["what"] != "term" else r["label"])
        w = worst.setdefault(key, dict(kernel=0.0, oracle=0.0, share=0.0, bound=0.0, k_sub=0.0, o_sub=0.0, calls=0, labels=set()))
        w["kernel"], w["oracle"] = max(w["kernel"], r["kernel_ulp"]), max(w["oracle"], r["oracle_ulp"])
        w["share"], w["bound"] = max(w["share"], r["share"]), max(w["bound"], r["largest_bound"])
        w["k_sub"], w["o_sub"] = max(w["k_sub"], r["kernel_subnormal"]), max(w["o_sub"], r["oracle_subnormal"])
        w["calls"] += 1
        w["labels"].add(r["label"])
    rows = [dict(line_class=k[0], route=k[1], quantity=k[2], kernel_distance_ulp=number(w["kernel"]), share_of_bound=number(w["share"]),
                 oracle_distance_ulp=number(w["oracle"]), largest_bound=number(w["bound"]), kernel_subnormal_distance=number(w["k_sub"]),
                 oracle_subnormal_distance=number(w["o_sub"]), tables_judged=w["calls"], kernels=sorted(w["labels"]))
            for k, w in sorted(worst.items())]
    doc = dict(what="pointwise distance of gamma, the Doppler width and alpha_line from the 80-bit evaluation of the reference's formulas, in units "
                    "of 2^-53 |truth| (normal values) and of 2^-1074 (subnormal ones): the kernel's, as a share of bound(), and the fp64 oracle's "
                    "(tests/test_gpu_line_params_truth.py); routes A direct formulas, B k_line_params, drop-in the DataFrame entry points",
               criterion=f"kernel <= {T.FACTOR:g} x oracle + A x 2^-53, A the amplification-weighted count of rounded operations with a library call "
                         "counted as LIB; capped by 1e-13 / 1e-15 / 3e-15 (gamma / Doppler width / alpha) where no amplification exceeds 1; zeros, "
                         "NaNs and infinities where the truth has them; B gives A's bits for gamma and the Doppler width; the generating pre-pass "
                         "gives the dense line opacity's bits",
               LIB=T.LIB, LIB_source=T.LIB_SOURCE, EXP_LIB=T.EXP_LIB, pytest_exit_code=rc, classes=list(T.CLASSES), rows=rows)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    for route in sorted({r["route"] for r in rows}):
        mine = [r for r in rows if r["route"] == route and isinstance(r["share_of_bound"], float)]
        if mine:
            r = max(mine, key=lambda r: r["share_of_bound"])
            print(f"route {route}: largest share of the bound {r['share_of_bound']:.3g} in {r['line_class']} / {r['quantity']} (kernel "
                  f"{r['kernel_distance_ulp']} ulp, oracle {r['oracle_distance_ulp']} ulp)")
    print("wrote", out, "| pytest exit code", rc)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "line_params_truth_classes.json")))
