"""What the instrument adjoint costs beside the instrument itself: in ONE process, after warm-up, alternating the forward launch
(sdx_observe_dev, stage k_observe) and the adjoint's four launches (sdx_observe_adjoint_dev, stage k_observe_adjoint: per-pixel
factors, the two scans in two launches, the gather per grid point), each timed by its own profile stage, one call per sample, the median of `samples`:
  S-c2: the S-c2 grid (7634 points), 2048 equal pixels over 6502 - 6598 A at R = 50 000
  S-c3: the S-c3 grid (120 398 points), 90 297 pixels of 1 / 2.5 FWHM at R = 30 000 over the whole range
in the modes plain, with a reference (the forward then sums two numerators; the adjoint also writes the reference's cotangent) and with
the nu / lambda factor.  The adjoint evaluates the forward's r_ij twice (denominators, then the gather) and scans the pixels twice.
    python scripts/observe_adjoint_cost.py [--samples 101] [--warmup 20] [--out profiles/observe_adjoint_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from observe_cost import pixels  # noqa: E402
from stardis_amd import _lib, synth  # noqa: E402
from stardis_amd import constants as K  # noqa: E402
from stardis_amd.instrument import Instrument  # noqa: E402


def stage_us(ctx, stage, call, samples):
    """median microseconds of `stage` over single profiled calls"""
    us = []
    for _ in range(samples):
        ctx.call("sdx_profile_reset")
        call()
        ctx.synchronize()
        n, ms = ctx.profile(stage)
        assert n == 1, (stage, n)
        us.append(ms * 1e3)
    return float(np.median(us)), float(np.min(us)), float(np.max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=101)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="S-c2,S-c3")
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    ctx = _lib.default_context()
    lines = []
    for tag in a.workloads.split(","):
        cfg = synth.WORKLOADS[tag]
        nus = synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R"), cfg.get("step"))
        lam = K.nu_to_angstrom(nus)
        edges, R = pixels(tag, lam)
        inst = Instrument(edges, resolving_power=R, ctx=ctx)
        rng = np.random.default_rng(3)
        flux, ref = 1.0 + 0.1 * rng.standard_normal(lam.size), 2.0 + 0.5 * np.sin(lam / 3.0)
        d_lam, d_nus, d_f, d_g, d_c = (ctx.upload(x) for x in (lam, nus, flux, ref, rng.standard_normal(inst.n_pix)))
        out, out_ref, pix = ctx.empty((lam.size,)), ctx.empty((lam.size,)), ctx.empty((inst.n_pix,))
        calls = {
            "plain": (lambda: inst.observe(d_lam, d_f, lam.size, out=pix), lambda: inst.adjoint(d_lam, lam.size, d_c, out=out)),
            "nus": (lambda: inst.observe(d_lam, d_f, lam.size, out=pix), lambda: inst.adjoint(d_lam, lam.size, d_c, nus=d_nus, out=out)),
            "reference": (lambda: inst.observe(d_lam, d_f, lam.size, reference=d_g, out=pix),
                          lambda: inst.adjoint(d_lam, lam.size, d_c, flux=d_f, reference=d_g, nus=d_nus, out=out, out_reference=out_ref)),
        }
        for forward, adjoint in calls.values():
            for _ in range(a.warmup):
                forward(), adjoint()
        ctx.synchronize()
        member = np.searchsorted(edges[:-1] - 8 * inst.sigma, lam, "right") - np.searchsorted(edges[1:] + 8 * inst.sigma, lam, "left")
        res = dict(n=int(lam.size), n_pix=int(inst.n_pix), resolving_power=R, samples=a.samples,
                   pixels_per_point=round(float(np.median(member[member > 0])), 1),
                   estimate_pixels_per_point=round(float(np.median(1.0 + 16.0 * inst.sigma / ((edges[-1] - edges[0]) / inst.n_pix))), 1))
        ctx.call("sdx_profile_enable", 1)
        try:
            for mode, (forward, adjoint) in calls.items():
                f_us, a_us = stage_us(ctx, "k_observe", forward, a.samples), stage_us(ctx, "k_observe_adjoint", adjoint, a.samples)
                res[mode] = dict(k_observe_us=dict(median=round(f_us[0], 2), min=round(f_us[1], 2), max=round(f_us[2], 2)),
                                 k_observe_adjoint_us=dict(median=round(a_us[0], 2), min=round(a_us[1], 2), max=round(a_us[2], 2)),
                                 ratio=round(a_us[0] / f_us[0], 2))
        finally:
            ctx.call("sdx_profile_enable", 0)
        line = json.dumps({tag: res})
        lines.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
