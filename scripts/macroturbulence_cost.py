"""What radial-tangential macroturbulence costs in the instrument: in ONE process, after warm-up, alternating variants with HIP-event
timing on the context's stream:
  (a) instr    the fused step with the present instrument (SpectralSynthesizer(instrument=Instrument(...))): the yardstick
  (b) v_mac    the same step with Instrument(..., v_mac=zeta): one k_macroturbulence in front of k_observe
  (c) v_rot    the same step with Instrument(..., v_rot=6 zeta): one k_rotate whose window has the macroturbulence's length (the
               window is 2 (6 zeta) / c wide against 2 V / c), so that the two kernels are read at equal numbers of terms
      S-c2: 2048 pixels at R = 50 000, zeta = 1.5 km/s (about 30 points per window: eight lanes per point), 5 (about 100) and 35
            (about 700: a wave per point, eleven trips per lane);  S-c3: the 90 297-pixel instrument at R = 30 000, zeta = 5
Each variant is timed in `rounds` interleaved rounds of `steps` eager steps; the spread of (a) across its rounds is the run-to-run
spread against which the added time is read.  A second, profiled pass reports k_macroturbulence and k_rotate beside k_observe per step
(with the mean number of points in k_observe's windows), and — one call per sample, the median — the adjoint stages for
pixel_weights_to_grid's call of Instrument.adjoint with nus.
    python scripts/macroturbulence_cost.py [--steps 50] [--rounds 7] [--warmup 20] [--samples 51] [--out profiles/macroturbulence_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from observe_cost import pixels, timed_ms  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.engine import SpectralSynthesizer  # noqa: E402
from stardis_amd.instrument import MACROTURBULENCE_REACH, Instrument  # noqa: E402

ZETAS = {"S-c2": (1.5, 5.0, 35.0), "S-c3": (5.0,)}
FORWARD = ("k_raytrace", "k_flux_nu_to_lambda", "k_rotate", "k_macroturbulence", "k_observe")
ADJOINT = ("k_observe_adjoint", "k_rotate_adjoint", "k_macroturbulence_adjoint")


def adjoint_us(ctx, inst, d_lam, d_nus, d_c, out, n, samples):
    """median microseconds of the adjoint stages over single profiled calls of inst.adjoint"""
    us = {stage: [] for stage in ADJOINT}
    for _ in range(samples):
        ctx.call("sdx_profile_reset")
        inst.adjoint(d_lam, n, d_c, nus=d_nus, out=out)
        ctx.synchronize()
        for stage, v in us.items():
            v.append(ctx.profile(stage)[1] * 1e3)
    return {stage: round(float(np.median(v)), 2) for stage, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--samples", type=int, default=51)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        w = synth.make_workload(tag)
        atm = w["atm"]
        lam = K.nu_to_angstrom(w["nus"])
        n = int(lam.size)
        edges, R = pixels(tag, lam)
        instruments = {"instr": Instrument(edges, resolving_power=R, ctx=ctx)}
        for zeta in ZETAS[tag]:
            instruments[f"v_mac={zeta:g}"] = Instrument(edges, resolving_power=R, ctx=ctx, v_mac=zeta)
            instruments[f"v_rot={MACROTURBULENCE_REACH * zeta:g}"] = Instrument(edges, resolving_power=R, ctx=ctx, v_rot=MACROTURBULENCE_REACH * zeta)
        args = (w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"])
        common = dict(ctx=ctx, track_evaluations=False, keep_line=False, keep_total=False)
        variants = {k: SpectralSynthesizer(*args, instrument=inst, **common) for k, inst in instruments.items()}
        for syn in variants.values():
            for _ in range(a.warmup):
                syn.step()
        ctx.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, syn in variants.items():
                times[k].append(timed_ms(ctx, syn, a.steps) * 1e3)
        d_lam, d_nus, d_c = ctx.upload(lam), ctx.upload(w["nus"]), ctx.upload(np.random.default_rng(3).standard_normal(edges.size - 1))
        out = ctx.empty((n,))
        prof = {}
        ctx.call("sdx_profile_enable", 1)
        try:
            for k, syn in variants.items():
                ctx.call("sdx_profile_reset")
                for _ in range(a.steps):
                    syn.step()
                ctx.synchronize()
                prof[k] = {}
                for kernel in FORWARD:
                    cnt, ms = ctx.profile(kernel)
                    prof[k][kernel] = dict(us_per_step=round(ms * 1e3 / a.steps, 2), launches_per_step=cnt / a.steps)
                for _ in range(3):
                    instruments[k].adjoint(d_lam, n, d_c, nus=d_nus, out=out)
                prof[k]["adjoint_us"] = adjoint_us(ctx, instruments[k], d_lam, d_nus, d_c, out, n, a.samples)
        finally:
            ctx.call("sdx_profile_enable", 0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        per_angstrom = (n - 1) / (lam[-1] - lam[0])
        reach = {k: (inst.v_rot or 0.0) + MACROTURBULENCE_REACH * (inst.v_mac or 0.0) for k, inst in instruments.items()}
        points = {k: round(float(2 * v / K.C_KMS * np.median(lam) * per_angstrom), 1) for k, v in reach.items() if v}
        sigma = instruments["instr"].sigma
        res = dict(n_nu=n, n_pix=int(edges.size - 1), resolving_power=R, steps_per_round=a.steps, rounds=a.rounds, samples=a.samples,
                   points_per_broadening_window=points,
                   points_per_observe_window=round(float(np.mean(np.diff(edges) + 16.0 * sigma) * per_angstrom), 1),
                   us_per_step={k: [round(x, 2) for x in v] for k, v in times.items()},
                   median_us={k: round(v, 2) for k, v in med.items()},
                   instr_spread_us=round(float(np.max(times["instr"]) - np.min(times["instr"])), 2),
                   added_us={k: round(v - med["instr"], 2) for k, v in med.items() if k != "instr"},
                   profiled=prof)
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
        for syn in variants.values():
            syn.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
