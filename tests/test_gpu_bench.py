"""bench.py on one GPU as every pull request runs it: a plain run prints the headline line (the other figures are --full's),
and --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(ctx, tmp_path):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                           "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    out = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = out["config"]
    assert out["metric"] == "spectral points/sec (N_nu x N_depth)" and out["unit"] == "spectral points/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["steps"] == 7 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - cfg["n_nu_global"] * cfg["n_depth"]) < 1e-9 * cfg["n_nu_global"] * cfg["n_depth"]
    assert not {"roofline", "roofline_fp64_valu", "cpu_baseline", "secondary", "dropin", "throughput_two_syntheses_in_flight"} & set(out)

    import bench
    from stardis_amd.engine import SpectralSynthesizer

    w = bench.build_workload("S-c2", 1)
    syn = SpectralSynthesizer(w["nus"], w["atm"]["temperatures"], w["atm"]["dist"], w["thetas"], w["weights"], w["lines"], w["cont"],
                              ctx=ctx, keep_line=False)
    try:
        syn.step()
        F, total = syn.F_nu(), syn.total_alphas()
    finally:
        syn.close()
    F_b, total_b = np.load(tmp_path / "F_nu.npy"), np.load(tmp_path / "total_alphas.npy")
    assert F_b.dtype == total_b.dtype == np.float64
    assert F_b.shape == total_b.shape == (cfg["n_depth"], cfg["n_nu_global"])
    assert rel_err(F_b, F) < 1e-12 and rel_err(total_b, total) < 1e-12
