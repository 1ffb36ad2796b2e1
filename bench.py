#!/usr/bin/env python
"""bench.py — spectral points / s of the STARDIS hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload S-c2] [--dump-outputs DIR] [--full]

With --gpus N > 1 and no WORLD_SIZE in the environment the script starts the N ranks itself (fresh child processes
through torch.distributed.run, before anything in this process touches the GPU) and relays rank 0's JSON line; under
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` it is one of the ranks.

One "step" = one full pass of the hot path over inputs already resident in HBM: window pre-pass + line opacity
(Voigt/Faddeeva over the whole line list) + continuum (H- bf table, H I bf/ff, Thomson) + total + LTE formal solution
over N_theta angles -> F_nu (N_d, N_nu).  Metric: spectral points per second = N_nu * N_depth * steps / time
(BASELINE.json).  At N = 1 `value` is measured on BASELINE configs[1] (S-c2, the 1-GPU config).  At N > 1 it is BASELINE
configs[2] — S-c3, the fixed 3000-10000 A grid (120 398 frequencies, 1.5e5 lines) split N ways in shards of equal estimated
work, `scaling: "strong"`; every step ends with ONE all-gather of the emergent flux (RCCL); `collective` says what
torch.distributed actually ran.  (--workload / --scaling override both, e.g. --workload S-c2 --scaling weak.)

A plain run sets up, warms up, times the K steps and prints `value` and `ms_per_step` (milliseconds per timed step) with the
workload's description.  --dump-outputs DIR then also writes what the last timed step handed its caller as DIR/<name>.npy
(float64; the inputs are seeded, so two builds can be compared array for array): F_nu.npy and total_alphas.npy (N_d, N_nu) on
one GPU, the gathered emergent flux spectrum.npy (N_nu,) on several.

With --full the JSON line also carries what takes runs of its own:
  ms_per_step_cold      the K steps timed right after the W warm-up steps (runs of fewer than 200 steps)
  throughput_two_syntheses_in_flight   one GPU: two syntheses on two streams, stepped alternately
  per_rank              several GPUs: every rank's shard and kernel times
  n1_same_workload      several GPUs: the one-GPU step of the same workload measured in the same run (speedup_vs_n1,
                        gathered_spectrum_equals_n1_bit_for_bit)
  roofline              HBM roofline of the dominant kernel (live HIP-event durations), traffic from profiles/
  roofline_fp64_valu    the bound that really limits the path: wave-level fp64 instructions per second against the spec issue rate
  cpu_baseline          the oracle (reference algorithm restated in C) on this box's host cores: one_core / best / all_cores
  secondary             BASELINE configs[2] and [3] at full size (S-c3: 1.5e5 lines, S-c4m: 1e6 lines): step time, per-kernel
                        times, Voigt evaluations/s, strided-column parity against the oracle
  secondary also holds  S-c5 (configs[4]: fp32-mixed synthesis + LSF + rotation on the device) and S-c4m-linelist (f1 inputs)
  dropin                wall time of the reference-shaped call path (RadiationField + calc_alphas + raytrace) at configs[0] and S-c2

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
FP64_VECTOR_PEAK_TFLOPS = 78.6
# wave-level fp64 VALU instructions per second: 256 CU x 4 SIMD x 2.4 GHz / 4 cycles per wave64 fp64 instruction — the ONE
# ceiling the VALU fractions are quoted against.  (Round 3 also quoted a "measured" 439 G/s from a pure-FMA loop; the line
# kernels beat it — the part clocks higher under their instruction mix — so it was not a ceiling of anything and is gone.)
FP64_VALU_SPEC = 256 * 4 * 2.4e9 / 4
KERNELS = ("k_dnu_partial", "k_classify", "k_prepass_continuum", "k_line_prepass", "k_hlist", "k_gather", "k_far_ranges", "k_line_all", "k_line_wide",
           "k_line_narrow", "k_line_far", "k_reduce_partials", "k_total_alphas", "k_raytrace")


# ------------------------------------------------------------------------------------------------ launch
def self_launch(args, argv):
    """--gpus N without a rendezvous: start the N ranks as fresh child processes.  Nothing in THIS process has touched
    HIP or torch.cuda yet (a GPU-initialised process must not exec or fork ranks)."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *argv]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    return proc.returncode if proc.returncode else (0 if line is not None else 1)


def build_workload(tag, world, inputs="dense", scaling="weak"):
    from stardis_amd import synth

    cfg = synth.WORKLOADS[tag]
    atm = synth.cool_dwarf_atmosphere() if cfg.get("atmosphere") == "cool_dwarf" else synth.solar_atmosphere()
    base = synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R"), cfg.get("step"))
    n_per_gpu = base.size
    # weak scaling: same window and line list, N x the resolving power -> N x the grid points
    # strong scaling: the workload's own grid, split N ways
    nus = base if (world == 1 or scaling == "strong") else synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R", 1.0), None, n_override=n_per_gpu * world)
    if inputs == "linelist":  # per-line scalars: alpha, gamma and the Doppler width are generated in the pre-pass
        lines = synth.synth_linelist(nus, atm, cfg["n_lines"], synth.SEED)
    else:
        lines = synth.synth_lines(nus, atm, cfg["n_lines"], synth.SEED, cfg["gamma_per_depth"])
    cont = synth.synth_continuum_state(atm)
    thetas, weights = synth.thetas_and_weights(synth.N_THETAS)
    return dict(tag=tag, atm=atm, nus=nus, lines=lines, cont=cont, thetas=thetas, weights=weights, n_per_gpu=n_per_gpu)


def synth_desc(tag):
    from stardis_amd import synth

    c = synth.WORKLOADS[tag]
    grid = f"R={c['R']:.0f}" if "R" in c else f"step {c['step']} A"
    star = "cool-dwarf (3800 K)" if c.get("atmosphere") == "cool_dwarf" else "solar"
    return f"{tag}: {star} MARCS structure, {c['lam0']:.0f}-{c['lam1']:.0f} A at {grid}, {c['n_lines']} lines, fp64"


def kernel_variant(ctx, stage):
    """which device kernel ran under a stage name in the last profiled pass (k_raytrace -> k_raytrace_seg<8,7> | k_raytrace<1> | ...)"""
    import ctypes as C

    buf = C.create_string_buffer(64)
    ctx.call("sdx_profile_variant", stage.encode(), buf, 64)
    return buf.value.decode() or stage


def sha16(a):
    import hashlib

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


PROFILED_PASS = {}  # id(ctx) -> the last kernel_times pass on that context: eager step wall time and kernel sum


def kernel_times(ctx, syn, n=10, settle_s=0.3):
    """Average duration of every kernel of one step: HIP events recorded by the library around each launch (eager launches on the
    context's stream), after `settle_s` of untimed eager steps — the same warm clocks as the timed graph replays (round 4 profiled
    right after the first step and reported kernel sums above the step time).  Events recorded during stream capture do not time
    the replayed graph on this runtime (scripts/r5/graph_events_probe.py: negative intervals), so the per-kernel figures come from
    THIS eager pass, whose own wall time per step is kept beside them: the kernels of a step sum to less than that."""
    import ctypes as C

    from stardis_amd import _lib

    def one():
        if getattr(syn, "m_max", None) is not None:  # two-collective mode: the classification launch is its own call
            syn.enqueue_classify()
        syn.enqueue()

    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        for _ in range(10):
            one()
        ctx.synchronize()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    ctx.synchronize()
    eager_ms = (time.perf_counter() - t0) / n * 1e3
    out = {}
    for name in KERNELS:
        cnt, ms = C.c_int64(), C.c_double()
        _lib.check(ctx.lib.sdx_profile_get(ctx.handle, name.encode(), C.byref(cnt), C.byref(ms)))
        if cnt.value:
            out[name] = ms.value / cnt.value * (cnt.value / n)  # per step (a kernel may run more than once per step)
    variant = kernel_variant(ctx, "k_raytrace")  # (before the records are cleared)
    line_variant = kernel_variant(ctx, "k_line_all")  # "k_line_all + far role": the far field's workgroups are part of this launch
    ctx.call("sdx_profile_enable", 0)
    ctx.call("sdx_profile_reset")
    PROFILED_PASS[id(ctx)] = {"eager_ms_per_step": eager_ms, "kernel_sum_ms": sum(out.values()), "steps": n, "k_raytrace_is": variant,
                              "k_line_all_is": line_variant,
                              "how": "eager launches bracketed by HIP events after %.1f s of eager settling; the timed step of "
                                     "`ms_per_step` runs the same kernels without the event records" % settle_s}
    return out


# ------------------------------------------------------------------------------------------------ CPU side (oracle = checker / baseline)
def cpu_one_pass(w):
    """The reference algorithm restated in C (oracle/): calc_alan_entries + continuum + raytrace, OpenMP where numba has prange."""
    import oracle
    from stardis_amd import constants as K

    atm, nus, ln, cont = w["atm"], w["nus"], w["lines"], w["cont"]
    nd = atm["temperatures"].size
    if not isinstance(ln, dict):  # per-line scalars: form what the reference forms on the host first (plasma/base.py:200-321, broadening.py:659-732)
        spec = ln
        args = (spec.atomic_number, spec.ion_number, spec.ionization_energy, spec.upper_energy, spec.lower_energy, spec.A_ul)
        state = (spec.electron_density, spec.temperature, spec.h_density)
        gam = (oracle.calc_vald_gamma(*args, spec.stark, spec.waals, spec.mass, *state, flags=spec.flags) if spec.gamma_mode == 1
               else oracle.calc_gamma(*args, *state, flags=spec.flags))
        ln = dict(line_nus=spec.nu, gammas=gam, doppler_widths=oracle.doppler_widths(spec.nu, spec.mass, spec.temperature, spec.microturbulence),
                  alphas=oracle.alpha_line_linelist(spec.e_low_ev, spec.g_lo, spec.strength, spec.nu, spec.pop_row, spec.pop, spec.temperature,
                                                    spec.alpha_coefficient))
    line = oracle.calc_alan_entries(nd, nus, ln["line_nus"], ln["doppler_widths"], ln["gammas"], ln["alphas"])
    lam = K.nu_to_angstrom(nus)
    cutoff = (cont["ionization_energy"] - cont["level_excitation"]) / K.H_CGS
    total = oracle.alpha_file_1d(lam, cont["hminus_bf_wavelength"], cont["hminus_bf_cross_section"], cont["n_hminus"])
    total = total + oracle.alpha_bf(nus, [0, len(cutoff)], [0], cutoff, cont["level_density"])
    total = total + oracle.alpha_ff(nus, atm["temperatures"], [1], cont["n_e"] * cont["n_h2"])
    total = total + oracle.alpha_electron(nus.size, cont["n_e"])
    total = total + line
    F, _ = oracle.raytrace(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], total)
    return F


def cpu_baseline(w, budget_s=25.0):
    """The oracle timed on this box's host cores on the same workload at several thread counts (a reported baseline, not the
    target; kind "port": numba cannot be installed).  -O3 -march=native, no fast-math (oracle/Makefile)."""
    import oracle

    nus, nd = w["nus"], w["atm"]["temperatures"].size
    max_threads = oracle.num_threads()
    pts = nus.size * nd
    sweep, F = {}, None
    counts = sorted({1, min(8, max_threads), min(16, max_threads), min(32, max_threads), max_threads})
    for n in counts:
        oracle.set_num_threads(n)
        times, spent = [], 0.0
        while len(times) < 2 or (spent < budget_s / len(counts) and len(times) < 6):
            t0 = time.perf_counter()
            F = cpu_one_pass(w)
            times.append(time.perf_counter() - t0)
            spent += times[-1]
        sweep[n] = min(times)
    oracle.set_num_threads(max_threads)
    best = min(sweep, key=sweep.get)
    n_l = w["lines"]["line_nus"].size if isinstance(w["lines"], dict) else w["lines"].n_lines
    return dict(
        value=pts / sweep[best], unit="spectral points/s", cores=best, kind="port",
        sample=f"full workload ({nus.size} nu x {nd} depths, {n_l} lines, {len(w['thetas'])} angles), best of >= 2 passes per thread count",
        one_core=pts / sweep[1], best=pts / sweep[best], best_threads=best, all_cores=pts / sweep[max_threads], host_cores=max_threads,
        ms_by_threads={str(n): round(t * 1e3, 2) for n, t in sweep.items()},
        build="gcc -O3 -march=native -fopenmp, no fast-math, no FMA contraction (oracle/Makefile)",
    ), F


def strided_parity(w, syn, stride):
    """Flux of a strided subset of columns recomputed by the oracle from the GPU's own total opacity (the formal solution is
    column-independent), and the GPU's evaluation count against the window rule on the host."""
    import oracle
    from stardis_amd import parallel

    atm, nus = w["atm"], w["nus"]
    F, total = syn.F_nu(), syn.total_alphas()
    cols = np.arange(0, nus.size, stride)
    F_ref, _ = oracle.raytrace(nus[cols], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], np.ascontiguousarray(total[:, cols]))
    ln = w["lines"]
    return dict(columns=int(cols.size), flux_max_rel_err=float(np.max(np.abs(F[1:, cols] - F_ref[1:]) / np.abs(F_ref[1:]))),
                evaluations_match_host_window_rule=bool(syn.evaluations() == parallel.window_evaluations(
                    nus, ln["line_nus"], ln["doppler_widths"], ln["gammas"], ln["alphas"])))


# ------------------------------------------------------------------------------------------------ secondary workloads
def secondary_block(tag, device, steps, check):
    from stardis_amd import _lib
    from stardis_amd.engine import SpectralSynthesizer

    t0 = time.perf_counter()
    w = build_workload(tag, 1)
    atm, nus = w["atm"], w["nus"]
    ctx = _lib.Context(device)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx, keep_line=False)
    syn.step()
    ctx.synchronize()
    setup_s = time.perf_counter() - t0
    evals = syn.evaluations()
    parity = strided_parity(w, syn, 601) if check else None
    syn.count_evaluations = False
    syn.capture()
    t_end = time.perf_counter() + 0.3  # settle (clocks), then time
    while time.perf_counter() < t_end:
        syn.step()
        ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        syn.step()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    kern = kernel_times(ctx, syn, 5)
    nd = atm["temperatures"].size
    line_ms = kern.get("k_line_all", 0.0) + kern.get("k_line_wide", 0.0) + kern.get("k_line_narrow", 0.0) + kern.get("k_line_far", 0.0)
    far_field = None
    if kern.get("k_line_far") or "far" in (PROFILED_PASS.get(id(ctx)) or {}).get("k_line_all_is", ""):
        # the far field of the line kernels is on for this grid (include/stardis_hip.h, option "far_field"): the same workload with
        # every window point evaluated where it lies, and how far the two spectra are apart
        F_far = syn.F_nu().copy()
        ctx.set_option("far_field", 0)
        syn.close()
        syn.capture()
        ctx.synchronize()
        F_direct = syn.F_nu().copy()
        t_end = time.perf_counter() + 0.3  # settle, as above
        while time.perf_counter() < t_end:
            syn.step()
            ctx.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            syn.step()
        ctx.synchronize()
        far_field = {"on": True, "ms_per_step_direct_sum": (time.perf_counter() - t1) / steps * 1e3,
                     "flux_max_rel_deviation_from_direct_sum": float(np.max(np.abs(F_far[1:] - F_direct[1:]) / np.abs(F_direct[1:]))),
                     "note": "window points at least three 256-point tiles from their line are summed at 16 Chebyshev nodes per tile and "
                             "interpolated; `voigt_evaluations` counts the reference's window points either way"}
        ctx.set_option("far_field", -1)
    out = {
        "workload": synth_desc(tag), "n_nu": int(nus.size), "n_lines": int(syn.n_lines), "steps": steps, "ms_per_step": ms,
        "spectral_points_per_s": nus.size * nd / (ms * 1e-3), "far_field": far_field, "voigt_evaluations": int(evals),
        "voigt_evaluations_per_s_line_kernel": evals / (line_ms * 1e-3) if line_ms else None,
        "voigt_evaluations_performed": performed_evaluations(w, bool(far_field)),
        "avg_kernel_ms": kern, "profiled_pass": PROFILED_PASS.get(id(ctx)), "algorithmic_bytes": int(syn.algorithmic_bytes()),
        "achieved_GBps": syn.algorithmic_bytes() / (ms * 1e-3) / 1e9, "frac_hbm": syn.algorithmic_bytes() / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
        "setup_s": setup_s,
    }
    if parity is not None:
        out["parity_vs_cpu_oracle"] = parity
    valu = profiled_valu(tag, kern)
    if valu is not None:
        out["roofline_fp64_valu"] = valu
    n_l, g_cols = syn.n_lines, syn.gamma_cols
    traffic = traffic_table(tag, kern, {"k_line_all": 8 * (n_l * (1 + 2 * nd + g_cols) + nus.size + nd * nus.size), "k_raytrace": 16 * nd * nus.size,
                                        "step": syn.algorithmic_bytes()})
    if traffic is not None:
        out["hbm_traffic"] = traffic
    syn.close()
    ctx.close()
    return out


def dropin_block(device, check):
    """Wall time of the reference-shaped call on a pandas stand-in for the plasma (synth.fake_plasma): what a user of
    create_stellar_radiation_field (stardis/radiation_field/base.py:71-117) pays, host objects in, F_nu on the host out —
    as one fused device pass with lazily materialised dictionary entries (the default), and source by source with every
    dictionary entry downloaded (`general_path_ms`: RadiationField + calc_alphas + raytrace), beside the oracle on the same arrays."""
    import stardis_amd.radiation_field.base as rf
    from stardis_amd import synth

    out = {}
    for label, tag, n_lines in (("configs[0] (1000-point grid)", "S-c1", 2000), ("S-c2", "S-c2", 2000)):
        cfg = synth.WORKLOADS[tag]
        atm = synth.solar_atmosphere()
        nus = synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R"), cfg.get("step"))
        plasma, model, config, arrays = synth.fake_plasma(nus, atm, n_lines, synth.SEED)

        def bench_path(fused, n=12):
            was = rf.FUSED
            rf.FUSED = fused
            try:
                times = []
                for _ in range(n):
                    t0 = time.perf_counter()
                    field = rf.create_stellar_radiation_field(nus.copy(), model, plasma, config)
                    times.append(time.perf_counter() - t0)
            finally:
                rf.FUSED = was
            return times, field

        times, field = bench_path(True)
        from stardis_amd.radiation_field import fused as fused_mod

        fused_mod.CACHE = False  # every derivation from the plasma's tables redone per call (sort, join, casts)
        try:
            uncached_times, _ = bench_path(True, 8)
        finally:
            fused_mod.CACHE = True
        gen_times, gen_field = bench_path(False, 6)
        entry = {"n_nu": int(nus.size), "n_lines": int(n_lines), "first_call_ms": times[0] * 1e3, "steady_ms": min(times[1:]) * 1e3,
                 "steady_ms_cache_off": min(uncached_times[1:]) * 1e3,
                 "cache": "derived tables kept per plasma object and verified by a 128-bit digest of the objects' values on every call: an edit in place is seen",
                 "spectral_points_per_s": nus.size * 56 / min(times[1:]), "path": type(field.opacities).__name__,
                 "general_path_ms": min(gen_times[1:]) * 1e3, "fused_equals_general_bit_for_bit": bool(np.array_equal(field.F_nu, gen_field.F_nu))}
        t0 = time.perf_counter()
        _ = field.opacities.total_alphas, [v for v in field.opacities.opacities_dict.values()]
        entry["materialise_every_dictionary_entry_ms"] = (time.perf_counter() - t0) * 1e3
        if check:
            import oracle

            od = field.opacities.opacities_dict  # broadening tables as the drop-in formed them (pinned to the reference by G3 / G9)
            lines = dict(arrays, gammas=np.asarray(od["alpha_line_at_nu_gammas"]), doppler_widths=np.asarray(od["alpha_line_at_nu_doppler_widths"]))
            w = dict(atm=atm, nus=nus, lines=lines, cont=synth.synth_continuum_state(atm), thetas=field.thetas, weights=field.I_nus_weights)
            t0 = time.perf_counter()
            F_cpu = cpu_one_pass(w)
            entry["oracle_all_cores_ms"] = (time.perf_counter() - t0) * 1e3
            entry["oracle_threads"] = oracle.num_threads()
            entry["emergent_flux_max_rel_err_vs_oracle"] = float(np.max(np.abs(field.F_nu[-1] - F_cpu[-1]) / np.abs(F_cpu[-1])))
        out[label] = entry
    # the configurations the fused call declined until round 4 — a molecular list next to the atomic one (include_molecules),
    # a spherical model, a line list without a dense alpha table (per-line scalars, f1) — at S-c2 size, fused against general
    cfg = synth.WORKLOADS["S-c2"]
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(cfg["lam0"], cfg["lam1"], cfg.get("R"), cfg.get("step"))

    def variant(name):
        plasma, model, config, _ = synth.fake_plasma(nus, atm, 2000, synth.SEED, n_molecule_lines=2000 if "molecules" in name else 0)
        if "molecules" in name:
            config.opacity.line.include_molecules = True
        if "spherical" in name:
            r = 6.96e10 + np.asarray(model.geometry.r, dtype=np.float64) - float(model.geometry.r[0])
            model.spherical, model.geometry.r, model.geometry.reference_r = True, r, float(r[-8])
        if "linelist" in name:
            plasma.alpha_line_from_linelist = None
            if "molecules" in name:
                plasma.molecule_alpha_line_from_linelist = None
        return plasma, model, config

    for name in ("S-c2 + molecules", "S-c2 spherical", "S-c2 linelist inputs (f1)", "S-c2 spherical + molecules + linelist inputs"):
        plasma, model, config = variant(name)
        res = {}
        for fused_on, n in ((True, 10), (False, 4)):
            was = rf.FUSED
            rf.FUSED = fused_on
            try:
                times = []
                for _ in range(n):
                    t0 = time.perf_counter()
                    field = rf.create_stellar_radiation_field(nus.copy(), model, plasma, config)
                    times.append(time.perf_counter() - t0)
            finally:
                rf.FUSED = was
            res[fused_on] = (times, field)
        (t_f, f_f), (t_g, f_g) = res[True], res[False]
        out[name] = {"n_nu": int(nus.size), "first_call_ms": t_f[0] * 1e3, "steady_ms": min(t_f[1:]) * 1e3, "path": type(f_f.opacities).__name__,
                     "general_path_ms": min(t_g[1:]) * 1e3, "fused_equals_general_bit_for_bit": bool(np.array_equal(f_f.F_nu, f_g.F_nu)),
                     "dictionary_keys": list(f_f.opacities.opacities_dict.keys())[-3:]}
    return out


# ------------------------------------------------------------------------------------------------ profiles/ (committed rocprofv3 passes)
def _profile_rows(workload, name):
    import csv
    import glob

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{workload}_pmc_{name}.csv")), reverse=True):
        return path, list(csv.DictReader(open(path)))
    return None, []


def profiled_traffic(workload, kernel):
    """HBM bytes per launch of `kernel` from the newest committed rocprofv3 PMC passes (profiles/, separate FETCH_SIZE and
    WRITE_SIZE runs, raw counters: profiles/README.md).  None when absent or when the kernel is not in them."""
    total = 0.0
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
        _, rows = _profile_rows(workload, name)
        vals = [float(r["Counter_Value"]) for r in rows if kernel_matches(kernel, r["Kernel_Name"]) and r["Counter_Name"] == name]
        if not vals:
            return None
        total += sum(vals) / len(vals) * 1024.0
    return total


def traffic_table(workload, kern, alg_bytes):
    """Per kernel of a step: counted HBM traffic per launch (committed FETCH_SIZE + WRITE_SIZE passes) and — for the kernels
    SURVEY §8d gives an algorithmic figure for — its ratio to the algorithmic bytes; plus the whole step."""
    out, total = {}, 0.0
    for name in kern:
        t = profiled_traffic(workload, name)
        if t is None:
            continue
        total += t
        out[name] = {"traffic_bytes": t}
        if name in alg_bytes:
            out[name]["algorithmic_bytes"] = int(alg_bytes[name])
            out[name]["traffic_over_algorithmic"] = t / alg_bytes[name]
    if out and "step" in alg_bytes:
        out["whole_step"] = {"traffic_bytes": total, "algorithmic_bytes": int(alg_bytes["step"]), "traffic_over_algorithmic": total / alg_bytes["step"]}
    return out or None


def measured_copy_bandwidth(device, gib=1.0, reps=5):
    """What this box's HBM sustains on a plain device-to-device copy (read + write counted), GB/s: the achievable ceiling
    SURVEY §8d asks for beside the 8 TB/s of the data sheet (the guide's own figure for the part is ~6.3 TB/s)."""
    import torch

    n = int(gib * (1 << 30)) // 8
    a = torch.empty(n, dtype=torch.float64, device=f"cuda:{device}").normal_()
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, 2.0 * n * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    del a, b
    torch.cuda.empty_cache()
    return best


def kernel_matches(short, full):
    alias = {"k_raytrace": ("k_raytrace", "k_formal"), "k_hlist": ("k_hlist", "k_hscan"), "k_gather": ("k_line_prepass",)}
    return any(a in full for a in alias.get(short, (short,)))


def profiled_valu(workload, kern):
    """The bound that actually limits this path: fp64 VALU issue.  Wave-level VALU instructions per step from the newest
    committed SQ_INSTS_VALU pass over the kernel time measured live in this run — reported only when the committed pass
    covers exactly the kernels that ran here (same names, same launches per step); otherwise the figure would silently lie.
    `per_kernel` gives the same ratio kernel by kernel."""
    path, rows = _profile_rows(workload, "SQ")
    # runtime-internal copy / fill kernels (input uploads of the profiled script) are not part of a step
    rows = [r for r in rows if r["Counter_Name"] == "SQ_INSTS_VALU" and not r["Kernel_Name"].startswith("__amd_rocclr_")]
    if not rows:
        return None
    by_kernel = {}
    for r in rows:
        by_kernel.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
    insts, t_ms, per_kernel = 0.0, 0.0, {}
    for name, ms in kern.items():
        matches = [v for k, v in by_kernel.items() if kernel_matches(name, k)]
        if not matches:
            return {"skipped": f"profiles/{os.path.basename(path)} does not cover kernel {name}: re-profile after changing the kernels"}
        n_inst = sum(sum(v) / len(v) for v in matches)  # a short name may cover several device kernels (k_hlist: count + scatter)
        insts += n_inst
        t_ms += ms
        per_kernel[name] = {"valu_wave_instr": n_inst, "ms": ms, "G_wave_instr_per_s": n_inst / (ms * 1e-3) / 1e9,
                            "frac_of_spec": n_inst / (ms * 1e-3) / FP64_VALU_SPEC}
    extra = [k for k in by_kernel if not any(kernel_matches(n, k) for n in kern)]
    if extra:
        return {"skipped": f"profiles/{os.path.basename(path)} holds kernels this run did not launch ({sorted(extra)[:2]}): re-profile"}
    achieved = insts / (t_ms * 1e-3)
    return {"bound": "fp64-valu-issue", "achieved": achieved / 1e9, "unit": "G wave-instr/s",
            "peak_spec": FP64_VALU_SPEC / 1e9, "frac_of_spec": achieved / FP64_VALU_SPEC,
            "valu_wave_instr_per_step": insts, "kernel_ms_per_step": t_ms, "per_kernel": per_kernel, "source": os.path.basename(path),
            "kernel_ms_regime": "the eager event-bracketed pass (`profiled_pass`): kernel_ms_per_step <= its eager_ms_per_step",
            "note": "peak_spec = 256 CU x 4 SIMD x 2.4 GHz / 4 cycles per wave64 fp64 instruction"}


# ------------------------------------------------------------------------------------------------ timed region
GRAPH_STEPS = 10  # at most this many steps per hipGraph launch of the one-GPU timed loop (--graph-steps)


class Runner:
    """One rank's synthesizer(s) + flux gather for a workload: step(), drain()."""

    def __init__(self, w, world, rank, local, ctx, scaling, use_graph, overlap, two_collectives=False, in_flight=1, graph_steps=10, steps=0):
        import torch

        from stardis_amd import _lib

        from stardis_amd import parallel
        from stardis_amd.engine import SpectralSynthesizer, shard_bounds

        nus, atm = w["nus"], w["atm"]
        self.nd = atm["temperatures"].size
        self.shards = None
        if scaling == "strong" and world > 1 and isinstance(w["lines"], dict):
            self.shards = parallel.balanced_shards(parallel.column_cost(nus, w["lines"]), world)
        self.begin, self.count = self.shards[rank] if self.shards else shard_bounds(nus.size, world, rank)
        self.world, self.overlap = world, overlap and world > 1
        dev = f"cuda:{local}"
        # the optional SECOND collective (--two-collectives): each rank classifies 1 / N of the line list, the shares of the per-line
        # maxima are all-gathered, the rest of the step runs on the gathered array (stardis_amd.parallel.ClassificationGatherer)
        self.classes = None
        two = two_collectives and world > 1 and scaling == "strong" and isinstance(w["lines"], dict)
        if two:
            self.classes = parallel.ClassificationGatherer(int(np.asarray(w["lines"]["line_nus"]).size), world, rank, dev)
        # --in-flight 2: the second lane is a synthesis on a context (HIP stream, scratch) of its own, stepped alternately with the first:
        # two independent syntheses of a queue (a grid of models) in flight per GPU — the stream-bound and launch-bound stretches of one
        # step run beside the arithmetic of the other.  Each lane's gather is ordered behind ITS stream.
        self.in_flight = 2 if in_flight == 2 else 1
        self.lane_classes = []  # (two collectives: every lane gathers into buffers of its own)
        self.lanes = []
        self.streams = [torch.cuda.current_stream()]
        self.contexts = [ctx]
        for k in range(2 if (self.overlap or self.in_flight == 2) else 1):
            if k > 0 and self.in_flight == 2:
                self.streams.append(torch.cuda.Stream(device=local))
                self.contexts.append(_lib.Context(local, stream=self.streams[-1].cuda_stream))
                ctx = self.contexts[-1]
            flux = torch.zeros((self.nd, self.count), dtype=torch.float64, device=dev)
            extra = {}
            if self.classes is not None:
                cls = self.classes if k == 0 else parallel.ClassificationGatherer(self.classes.n_lines, world, rank, dev)
                self.lane_classes.append(cls)
                extra = dict(classify_share=cls.share, m_max=cls.full, m_share_out=cls.send)
            syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                                      shard=(self.begin, self.count), flux_out=flux, track_evaluations=(k == 0 and self.classes is None),
                                      keep_line=False, **extra)
            self.lanes.append([syn, flux, parallel.FluxGatherer(nus.size, world, flux.device, shards=self.shards)])
        self.syn, self.flux = self.lanes[0][0], self.lanes[0][1]
        if self.classes is not None:
            for k, (lane, cls) in enumerate(zip(self.lanes, self.lane_classes)):  # (every lane's gathered array must be valid before its graphs are captured)
                with torch.cuda.stream(self.streams[k % len(self.streams)]):
                    lane[0].enqueue_classify()
                    cls.gather()
            torch.cuda.synchronize()
            self.evals = None  # (the counting pre-pass is the unculled one: not part of this mode)
        self.syn.step()
        self.contexts[0].synchronize()
        if self.classes is None:
            self.evals = self.syn.evaluations()
            self.syn.count_evaluations = False  # known now; the counter costs a memset + a copy per step
        # one GPU, one synthesis after the other: the timed steps are enqueued as hipGraph replays of up to --graph-steps (10) steps each (+ single-step
        # replays for a remainder, at drain()) — successive graph launches are ~8.5 us apart on this runtime whatever they hold, a tenth of
        # the S-c2 step; every step of a batch is the whole step (pre-pass, line kernel, formal solution) on the resident inputs
        # (the largest batch <= --graph-steps that divides the K timed steps: the timed region is then batch launches only — a launch of a
        # DIFFERENT graph than the stream's last one costs ~60-100 us on this runtime, so batches and single steps must not alternate)
        self.batch = 1
        # Runs of fewer than 100 timed steps keep one launch per step: a batch graph's own launch latency (the GPU is idle at the start
        # of the timed region) outweighs the gaps it saves over a handful of launches (measured at 20 steps: 95-111 us against 93-94).
        if use_graph and world == 1 and self.in_flight == 1 and self.classes is None and steps >= 100:
            self.batch = max([d for d in range(1, max(1, int(graph_steps)) + 1) if steps % d == 0])
        self.pending = 0
        if use_graph:
            for k, lane in enumerate(self.lanes):
                with torch.cuda.stream(self.streams[k % len(self.streams)]):
                    lane[0].capture(batch=self.batch if k == 0 else 1)
            if self.batch > 1:  # (a graph's first launch uploads it: part of the set-up, like the eager step above)
                self.syn.step_batch()
                self.contexts[0].synchronize()
        self.counter = 0
        self.last = None
        self.replay = use_graph  # (False with a captured graph: plain launches; calibrate() may switch)

    def calibrate(self, steps):
        """One GPU, neither --graph nor --no-graph given: time `steps` untimed steps as plain launches and as graph replays and keep the
        faster for the timed region (both run the same three kernels; which wins depends on the host's enqueue rate against the
        runtime's 8.5-9 us between graph launches).  -> {mode, plain_ms_per_step, graph_ms_per_step}"""
        import torch

        out = {}
        for mode in (False, True):
            self.replay = mode
            for _ in range(max(8, steps // 4)):
                self.step()
            self.drain()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step()
            self.drain()
            torch.cuda.synchronize()
            out["graph_ms_per_step" if mode else "plain_ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        self.replay = out["graph_ms_per_step"] < out["plain_ms_per_step"]
        out["mode"] = "hipGraph replay" if self.replay else "plain launches"
        # (the launches that precede the timed region are of the kind it uses)
        for _ in range(max(8, steps // 4)):
            self.step()
        self.drain()
        torch.cuda.synchronize()
        return out

    def _run(self, syn, k=0):
        if self.classes is not None:
            syn.step_classify()
            self.lane_classes[k].gather()
        if self.replay or syn.graph is None:
            syn.step()
        else:
            syn.enqueue()

    def step(self):
        import torch

        if self.batch > 1 and self.replay:  # (one GPU: a full batch goes out as one graph launch; drain() sends what is left, step by step)
            self.pending += 1
            if self.pending == self.batch:
                self.syn.step_batch()
                self.pending = 0
            return None
        k = self.counter % len(self.lanes)
        syn, flux, gather = self.lanes[k]
        self.counter += 1
        self.last = gather
        if self.in_flight == 2:
            with torch.cuda.stream(self.streams[k]):  # (the collective is enqueued behind the current torch stream: this lane's)
                gather.finish()
                self._run(syn, k)
                gather.start(flux[-1])
            return None
        if self.overlap:
            gather.finish()  # the gather that last read this lane's flux buffer
            self._run(syn, k)
            gather.start(flux[-1])
            return None
        self._run(syn, k)
        return gather(flux[-1])

    def drain(self):
        import torch

        while self.pending:
            self._run(self.syn)
            self.pending -= 1
        if self.in_flight == 2:
            for k, (_, _, gather) in enumerate(self.lanes):
                with torch.cuda.stream(self.streams[k]):
                    gather.finish()
        elif self.overlap:
            for _, _, gather in self.lanes:
                gather.finish()

    def last_spectrum(self):
        """the emergent flux the last step gathered (every rank holds it), as a host array"""
        if self.last is None:
            return None
        self.drain()
        import torch

        torch.cuda.synchronize()
        return self.last._assemble().cpu().numpy() if self.world > 1 else None

    def last_outputs(self):
        """what the last step handed its caller, as host arrays: one GPU F_nu and total_alphas (N_d, N_nu) of the lane that ran it,
        several GPUs the gathered emergent flux (N_nu,)"""
        if self.world > 1:
            return {"spectrum": self.last_spectrum()}
        import torch

        self.drain()
        torch.cuda.synchronize()
        syn, flux, _ = self.lanes[(self.counter - 1) % len(self.lanes)]  # (batched replays run lane 0 only and leave counter at 0)
        return {"F_nu": flux.cpu().numpy(), "total_alphas": np.array(syn.total_alphas(), dtype=np.float64)}

    def close(self):
        for syn, _, _ in self.lanes:
            syn.close()
        for extra in self.contexts[1:]:  # (the second lane's own context of --in-flight 2; the first is the caller's)
            extra.close()
        self.contexts = self.contexts[:1]


def performed_evaluations(w, far_field_on):
    """{nominal, performed, note}: the reference's window points (what `voigt_evaluations` counts: sum of hi - lo) next to what the
    line kernels evaluate — with the far field on, a (line, depth, tile) triple far from its line costs 16 Chebyshev nodes instead of
    256 points (stardis_amd.parallel.window_evaluations_performed, a host estimate; dense line tables only)."""
    from stardis_amd import parallel

    ln = w["lines"]
    if not isinstance(ln, dict):
        return None
    performed, nominal = parallel.window_evaluations_performed(w["nus"], ln["line_nus"], ln["doppler_widths"], ln["gammas"], ln["alphas"], far_field_on)
    return {"nominal_window_points": int(nominal), "performed": int(performed), "far_field": bool(far_field_on),
            "note": "performed = direct window points + 16 nodes per far (line, depth, tile) triple; a host estimate in index space"
                    if far_field_on else "no far field on this grid: every window point is evaluated where it lies"}


def timed(runner, steps, warmup, world, local, settle_s=0.5, cold=True):
    """-> dict(elapsed = max over ranks of the K timed steps after warm-up + settling, local = this rank's own time for them
    (before the closing barrier), cold = max over ranks of K steps timed right after the W requested warm-up steps, settle = number
    of untimed settling steps)."""
    import gc

    import torch
    import torch.distributed as dist

    dev = f"cuda:{local}" if (world > 1 and dist.get_backend() == "nccl") else "cpu"

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def rank_max(x, dtype):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=dtype, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.item()

    def run(k):
        gc_was_on = gc.isenabled()
        gc.disable()  # a collection pause between two enqueues leaves the device idle for longer than a step takes
        t0 = time.perf_counter()
        for _ in range(k):
            runner.step()
        runner.drain()
        torch.cuda.synchronize()
        t_local = time.perf_counter() - t0
        fence()
        t_all = time.perf_counter() - t0
        if gc_was_on:
            gc.enable()
        return float(rank_max(t_all, torch.float64)), t_local

    for _ in range(warmup):
        runner.step()
    runner.drain()
    fence()
    if settle_s <= 0:  # a long run: the W warm-up steps are all that precedes the timed region
        elapsed, t_local = run(steps)
        return dict(elapsed=elapsed, local=t_local, cold=elapsed, settle=0, launch=None)
    # the K steps right after the W requested warm-up steps: clocks still ramping (reported as ms_per_step_cold)
    t_cold = run(steps)[0] if cold else None
    # clocks and caches settle over the first tenths of a second of work: a short --steps run would otherwise time the ramp
    # (measured: 20 timed steps right after 0.1 s of settling varied between 102 and 116 us per step from run to run)
    # (untimed extra steps; the same number on every rank)
    t0 = time.perf_counter()
    runner.step()
    runner.drain()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    extra = int(rank_max(int(min(10000, settle_s / one)), torch.int64))
    b = int(getattr(runner, "batch", 1))
    extra = -(-extra // b) * b  # (whole batches: the launches that precede the timed region are of the graph it replays)
    for _ in range(extra):
        runner.step()
    runner.drain()
    fence()
    launch = None
    if getattr(runner, "auto_mode", False):
        n_cal = max(steps, 100)
        launch = runner.calibrate(n_cal)
        extra += 2 * n_cal + 3 * max(8, n_cal // 4)  # (the calibration's steps are untimed steps before the timed region too)
        fence()
    elapsed, t_local = run(steps)
    return dict(elapsed=elapsed, local=t_local, cold=t_cold, settle=extra + 1, launch=launch)


DUMP_BYTES = 64 * 10**6  # --dump-outputs writes at most this much


def dump_outputs(directory, arrays):
    """--dump-outputs: every array as <directory>/<name>.npy in float64.  Above DUMP_BYTES in all, a fixed, seeded sample of the
    frequency columns (the last axis, the same columns in every array) is written instead of the whole arrays."""
    os.makedirs(directory, exist_ok=True)
    arrays = {name: np.asarray(a, dtype=np.float64) for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    cols = None
    if total > DUMP_BYTES:
        n_nu = next(iter(arrays.values())).shape[-1]
        cols = np.sort(np.random.default_rng(0).choice(n_nu, size=n_nu * DUMP_BYTES // total, replace=False))
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a if cols is None else np.ascontiguousarray(a[..., cols]))


def n1_same_workload(w, local, steps, use_graph, in_flight=1):
    """The whole grid of `w` on ONE GPU (this rank's), graph-replayed like the timed loop: the denominator of the strong-scaling
    speed-up, measured in the same process and run — with as many syntheses in flight as the timed loop keeps."""
    import torch

    from stardis_amd import _lib
    from stardis_amd.engine import SpectralSynthesizer

    atm, nus = w["atm"], w["nus"]
    ctxs = [_lib.Context(local) for _ in range(in_flight)]
    syns = [SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=c,
                                track_evaluations=False, keep_line=False) for c in ctxs]
    if use_graph:
        for syn in syns:
            syn.capture()

    def sync():
        for c in ctxs:
            c.synchronize()

    t_end = time.perf_counter() + 0.3
    n = 0
    while n < 3 or time.perf_counter() < t_end:
        syns[n % in_flight].step()
        sync()
        n += 1
    t0 = time.perf_counter()
    for k in range(steps):
        syns[k % in_flight].step()
    sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    last = np.array(syns[0].F_nu()[-1], dtype=np.float64)
    spectrum_hash = sha16(last)
    for syn, c in zip(syns, ctxs):
        syn.close()
        c.close()
    torch.cuda.synchronize()
    return {"ms_per_step": ms, "value": nus.size * atm["temperatures"].size / (ms * 1e-3), "steps": steps, "spectrum_sha256_16": spectrum_hash,
            "in_flight": in_flight, "_spectrum": last,
            "how": "the unsharded grid on rank 0's GPU, same process, after the timed region (other ranks wait at a barrier)"}


def collective_info(world, runner):
    import torch
    import torch.distributed as dist

    if world == 1:
        return None
    info = {"op": "all_gather_into_tensor of the zero-padded F_nu[-1] shards", "backend": dist.get_backend(), "world_size_seen_by_dist": dist.get_world_size(),
            "bytes_per_rank": int(runner.lanes[0][2].per * 8), "overlapped_with_next_step": bool(runner.overlap)}
    if runner.classes is not None:
        info["second_collective"] = {"op": "all_gather_into_tensor of the per-line maxima (each rank classifies 1 / N of the line list), between the "
                                           "classification launch and the rest of the step", "bytes_per_rank": int(runner.classes.per * 8)}
    if dist.get_backend() == "nccl":
        try:
            info["nccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:  # noqa: BLE001
            pass
    return info


def s_c5_block(device, steps, check):
    """BASELINE configs[4]: the full solar spectrum synthesised with the fp32-mixed tolerance path, then F_lambda, the instrumental
    LSF and the rotational kernel on the device (postprocess.DeviceSpectrum) — step + chain timed, parity of the mixed spectrum
    against the fp64 one in the line."""
    from stardis_amd import _lib, postprocess, synth
    from stardis_amd import constants as K
    from stardis_amd.engine import SpectralSynthesizer

    tag = "S-c5"
    cfg = synth.WORKLOADS[tag]
    w = synth.make_workload(tag)
    atm, nus = w["atm"], w["nus"]
    fwhm_pix = cfg["R"] / cfg["lsf_resolution"]
    sigma_pix, vel_per_pix = fwhm_pix / 2.355, K.C_KMS / cfg["lsf_resolution"] / fwhm_pix
    res = {}
    for mode in ((0, 1) if check else (1,)):
        ctx = _lib.Context(device)
        ctx.set_option("mixed_precision", mode)
        syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                                  track_evaluations=False, keep_line=False, keep_total=False)
        syn.capture()
        spec = postprocess.DeviceSpectrum(syn)

        def chain():
            syn.step()
            return spec.broadened(sigma_pix=sigma_pix, velocity_per_pix=vel_per_pix, v_rot=cfg["v_rot_kms"])

        for _ in range(3):
            out = chain()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            syn.step()
        ctx.synchronize()
        t_step = (time.perf_counter() - t0) / steps
        t0 = time.perf_counter()
        for _ in range(steps):
            out = chain()
        ctx.synchronize()
        t_chain = (time.perf_counter() - t0) / steps
        res[mode] = dict(step_ms=t_step * 1e3, chain_ms=t_chain * 1e3, F=syn.F_nu()[-1], broad=out.numpy())
        syn.close()
        ctx.close()
    m = res[1]
    nd = atm["temperatures"].size
    out = {"workload": synth_desc(tag).replace("fp64", "fp32-mixed line opacity (stated tolerance 1e-4 on the flux), fp64 continuum and formal solution")
           + f"; then F_lambda, Gaussian LSF (R = {cfg['lsf_resolution']:.0f}) and rotation (v sin i = {cfg['v_rot_kms']:.0f} km/s) on the device",
           "n_nu": int(nus.size), "steps": steps, "ms_per_step_synthesis": m["step_ms"], "ms_per_step_with_postprocessing": m["chain_ms"],
           "spectral_points_per_s": nus.size * nd / (m["chain_ms"] * 1e-3)}
    if 0 in res:
        f = res[0]
        out["fp64_ms_per_step_synthesis"] = f["step_ms"]
        out["mixed_vs_fp64"] = {"emergent_flux_max_rel_err": float(np.max(np.abs(m["F"] - f["F"]) / np.abs(f["F"]))),
                                "broadened_spectrum_max_rel_err": float(np.max(np.abs(m["broad"] - f["broad"]) / np.abs(f["broad"]))),
                                "stated_tolerance": 1e-4, "speedup_of_the_step": f["step_ms"] / m["step_ms"]}
    return out


def linelist_block(tag, device, steps):
    """SURVEY §8 f1 at the size it exists for: the line list as ~100 B of scalars per line, alpha / gamma / Doppler width generated
    in the pre-pass, beside the dense-input step of the same workload (secondary[tag])."""
    from stardis_amd import _lib
    from stardis_amd.engine import SpectralSynthesizer

    w = build_workload(tag, 1, "linelist")
    atm, nus = w["atm"], w["nus"]
    ctx = _lib.Context(device)
    syn = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                              track_evaluations=False, keep_line=False)
    syn.step()
    ctx.synchronize()
    kern = kernel_times(ctx, syn, 5)
    syn.capture()
    for _ in range(2):
        syn.step()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        syn.step()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    nd = atm["temperatures"].size
    dense_bytes = 8 * syn.n_lines * (1 + 2 * nd + syn.gamma_cols)
    list_bytes = syn.n_lines * syn.linelist.host.bytes_per_line() + 8 * syn.linelist.host.pop.size
    out = {"workload": synth_desc(tag) + ", line list as per-line scalars (parameters generated on the device)", "n_lines": int(syn.n_lines),
           "steps": steps, "ms_per_step": ms, "spectral_points_per_s": nus.size * nd / (ms * 1e-3), "avg_kernel_ms": kern,
           "line_list_bytes": int(list_bytes), "dense_tables_bytes": int(dense_bytes), "hbm_bytes_saved": int(dense_bytes - list_bytes),
           "algorithmic_bytes": int(syn.algorithmic_bytes())}
    syn.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default=None, help="default: S-c2 (BASELINE configs[1]) on one GPU, S-c3 (configs[2]) on several")
    ap.add_argument("--inputs", choices=("dense", "linelist"), default="dense",
                    help="line list as the reference's dense (N_l, N_d) tables, or as per-line scalars expanded on the device")
    ap.add_argument("--scaling", choices=("weak", "strong"), default=None,
                    help="what `value` measures at N > 1. strong (default): the workload's grid split across the GPUs in shards of equal "
                         "estimated work (stardis_amd.parallel.balanced_shards); weak: fixed grid points per GPU (N x the resolving power)")
    ap.add_argument("--graph-steps", type=int, default=GRAPH_STEPS,
                    help="one GPU: at most this many steps per hipGraph launch of the timed loop (default 10; the largest divisor of --steps is taken; "
                         "1: one launch per step, as rounds 1-5 timed it)")
    ap.add_argument("--in-flight", type=int, choices=(1, 2), default=None,
                    help="2: every rank keeps two syntheses in flight (two contexts, stepped alternately) — throughput of a queue of independent "
                         "syntheses instead of one step after the other; `value` then counts both, and on several GPUs one synthesis's collectives "
                         "run under the other's kernels.  Default: 2 for strong scaling on several GPUs, 1 otherwise (serial steps)")
    ap.add_argument("--two-collectives", action="store_true",
                    help="N > 1, strong scaling (the default there): every rank classifies 1 / N of the line list and the per-line maxima are "
                         "all-gathered (a second collective of 8 N_l bytes per step) instead of every rank streaming the whole list")
    ap.add_argument("--one-collective", action="store_true",
                    help="N > 1, strong scaling: every rank classifies the whole line list itself; the flux gather is the only collective")
    ap.add_argument("--no-graph", action="store_true", help="plain launches (the default on ONE GPU since round 6, see --graph)")
    ap.add_argument("--graph", action="store_true",
                    help="one GPU: replay the step as a hipGraph (the default on several GPUs).  Round 6 measured successive graph launches "
                         "8.5-9 us apart on this runtime while plain launches of the same three kernels follow each other closely and cost the "
                         "host 10 us per step: S-c2 86-88 us per step with plain launches, 91-93 as graph replays")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure also measure and check everything else: cold timing, per-kernel times and rooflines, "
                         "the CPU baseline and parity against the oracle, two syntheses in flight, the secondary and drop-in blocks (one GPU), "
                         "per-rank times and the one-GPU run of the same workload (several GPUs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip every leg that runs the CPU oracle (baseline and parity checks)")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the S-c3 / S-c4m / S-c5 / drop-in blocks")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.workload is None:
        args.workload = "S-c2" if args.gpus == 1 else "S-c3"
    if args.scaling is None:
        args.scaling = "weak" if args.gpus == 1 else "strong"

    strong_many = args.gpus > 1 and args.scaling == "strong"
    if args.in_flight is None:
        args.in_flight = 2 if strong_many else 1
    args.two_collectives = (args.two_collectives or strong_many) and not args.one_collective

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args, sys.argv[1:]))

    import torch

    from stardis_amd import _lib, parallel

    # test hooks: SDX_BENCH_BACKEND=gloo and SDX_BENCH_SINGLE_DEVICE=1 let the N > 1 path run on a 1-GPU box
    rank, world, local = parallel.init_from_env(os.environ.get("SDX_BENCH_BACKEND", "nccl"))
    if os.environ.get("SDX_BENCH_SINGLE_DEVICE") == "1":
        local = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    import torch.distributed as dist

    check = not args.no_cpu_baseline
    w = build_workload(args.workload, world, args.inputs, args.scaling)
    nus, atm = w["nus"], w["atm"]
    nd = atm["temperatures"].size

    # the library enqueues on torch's current (non-default, capturable) stream, so the RCCL gather is
    # stream-ordered behind the kernels without a host sync
    stream = torch.cuda.Stream(device=local)
    torch.cuda.set_stream(stream)
    ctx = _lib.Context(local, stream=stream.cuda_stream)
    # N > 1: two flux buffers alternate so that the all-gather of step k (RCCL, its own stream) overlaps the kernels
    # of step k+1; a buffer is reused only after its gather has been waited for.  SDX_BENCH_SYNC_GATHER=1: blocking gather.
    overlap = os.environ.get("SDX_BENCH_SYNC_GATHER") != "1"
    # several GPUs: hipGraph replays.  One GPU: --graph / --no-graph as asked; by default the graph is captured, the run starts with plain
    # launches and the settling phase times both kinds of launch and keeps the faster (Runner.calibrate)
    auto_mode = world == 1 and not args.graph and not args.no_graph and args.in_flight == 1
    use_graph = (args.graph or world > 1 or auto_mode) and not args.no_graph
    runner = Runner(w, world, rank, local, ctx, args.scaling, use_graph, overlap, args.two_collectives, args.in_flight, args.graph_steps, args.steps)
    if auto_mode:
        runner.replay = False   # (the cold figure — K steps right after the W warm-up steps — is taken with plain launches)
        # ... and the settling phase that short runs have anyway decides (timed(): calibrate); a run of >= 200 steps has no settling
        # phase and stays with plain launches, the faster kind in every comparison of round 6 (86 - 88 us against 89 - 91 in batched replays)
        runner.auto_mode = args.steps < 200
    # a run of >= 200 timed steps is long enough for the clocks to have settled within its first few percent: the W warm-up steps
    # the driver asked for are then ALL that precedes the timed region; shorter runs get ~0.5 s of untimed settling (disclosed)
    tm = timed(runner, args.steps, args.warmup, world, local, settle_s=0.0 if args.steps >= 200 else 0.5, cold=args.full and args.steps < 200)
    elapsed, settle = tm["elapsed"], tm["settle"]
    syn, flux, count, evals = runner.syn, runner.flux, runner.count, runner.evals
    outputs = runner.last_outputs()
    spectrum = outputs.get("spectrum")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs)
    # everything below that is not the headline figure runs under --full only
    if args.full:
        kern = kernel_times(ctx, syn, 20)
        rt_variant = PROFILED_PASS[id(ctx)]["k_raytrace_is"]

    # N > 1: what every rank did (shard, its own time for the timed steps, per-kernel times), gathered on rank 0, and the
    # one-GPU step of the same workload on rank 0's GPU
    per_rank, n1 = None, None
    if world > 1 and args.full:
        mine = {"rank": rank, "device": local, "shard": [int(runner.begin), int(runner.count)], "ms_per_step_own": tm["local"] / args.steps * 1e3,
                "avg_kernel_ms": kern}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
        if rank == 0 and args.scaling == "strong":
            n1 = n1_same_workload(w, local, max(5, min(args.steps, 40)), use_graph, runner.in_flight)
        torch.cuda.synchronize()
        dist.barrier()

    # secondary figure (not `value`): two independent syntheses in flight on two streams — what a parameter grid
    # of stars would use; each is still a full pass, they only overlap on the device
    pipelined = None
    if world == 1 and args.full and not args.no_secondary:
        from stardis_amd.engine import SpectralSynthesizer

        ctx_b = _lib.Context(local)
        syn_b = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], w["thetas"], w["weights"], w["lines"], w["cont"],
                                    ctx=ctx_b, track_evaluations=False, keep_line=False)
        if use_graph:
            syn_b.capture()
        for _ in range(max(2, args.warmup // 2)):
            syn.step()
            syn_b.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            (syn if k % 2 == 0 else syn_b).step()
        torch.cuda.synchronize()
        pipelined = nus.size * nd * args.steps / (time.perf_counter() - t0)
        syn_b.close()
        ctx_b.close()

    if rank == 0:
        pts_total = nus.size * nd
        ms_per_step = elapsed / args.steps * 1e3
        value = pts_total * args.steps / elapsed
        n_l, g_cols = syn.n_lines, syn.gamma_cols
        scaling_text = {"weak": "weak (fixed points per GPU: N x the resolving power on the same window)",
                        "strong": "strong (BASELINE's fixed grid split N ways in shards of equal estimated work)"}[args.scaling]
        out = {
            "metric": "spectral points/sec (N_nu x N_depth)",
            "value": value,
            "unit": "spectral points/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "ms_per_step_cold": (tm["cold"] / args.steps * 1e3) if tm["cold"] is not None else None,
            "value_cold": (pts_total * args.steps / tm["cold"]) if tm["cold"] else None,
            "untimed_settle_steps_after_warmup": settle,
            "timed_region": ("the K steps follow the W warm-up steps directly" if settle == 0 else
                             f"K steps after W warm-up steps + {settle} untimed settling steps (~0.5 s: clocks; runs of >= 200 steps skip it); "
                             + ("ms_per_step_cold = the same K steps timed right after the W warm-up steps" if tm["cold"] is not None else
                                "ms_per_step_cold is measured with --full")),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": synth_desc(args.workload),
                "scaling": scaling_text if world > 1 else "one GPU",
                "n_nu_global": int(nus.size),
                "n_nu_per_gpu": int(count),
                "n_depth": int(nd),
                "n_lines": int(n_l),
                "n_theta": int(len(w["thetas"])),
                "voigt_evaluations_global": int(evals) if evals is not None else None,
                "parallelism": f"nu-shard x{world}" + (", 1 all-gather of F_nu[-1] per step" + (" overlapped with the next step" if runner.overlap else "") if world > 1 else ""),
                "hip_graph": bool(runner.replay),
                "launch_mode": (tm.get("launch") or {"mode": "hipGraph replay" if runner.replay else "plain launches",
                                                    "chosen": "by flag" if (args.graph or args.no_graph) else ("default of one-GPU runs of >= 200 steps" if world == 1 and not runner.replay else "default (several GPUs, --in-flight 2)")}),
                "graph_steps_per_launch": runner.batch if runner.replay else 1,
                "syntheses_in_flight_per_gpu": runner.in_flight,
                # how `value` was timed (the driver keeps `config`): `value` / `ms_per_step` are the K steps after the W warm-up steps and,
                # for runs of fewer than 200 steps, this many further untimed steps (~0.5 s: the clocks ramp); *_cold are the same K steps
                # timed right after the W warm-up steps — the figure that honours the command line to the letter
                "untimed_settle_steps_after_warmup": settle,
                "ms_per_step_cold": (tm["cold"] / args.steps * 1e3) if tm["cold"] is not None else None,
                "value_cold": (pts_total * args.steps / tm["cold"]) if tm["cold"] else None,
                "line_inputs": args.inputs,
                "outputs": "F_nu and total_alphas (N_d, N_nu); the optional alpha_line plane is not written",
            },
        }
        if args.full:
            dom = max(kern, key=kern.get)
            alg_bytes = {
                # SURVEY §8d per-stage figures, for the columns this rank produced
                "k_line_all": 8 * (n_l * (1 + 2 * nd + g_cols) + nus.size + nd * count),
                "k_raytrace": 16 * nd * count,
            }.get(dom, syn.algorithmic_bytes())
            achieved = alg_bytes / (kern[dom] * 1e-3) / 1e9
            copy_gbps = measured_copy_bandwidth(local) if world == 1 else None
            dom_traffic = profiled_traffic(args.workload, dom) if world == 1 else None
            line_ms = kern.get("k_line_all", 0.0) + kern.get("k_line_wide", 0.0) + kern.get("k_line_narrow", 0.0)
            far_on = "far" in (PROFILED_PASS.get(id(ctx)) or {}).get("k_line_all_is", "") or bool(kern.get("k_line_far"))
            out["counters_from"] = ("instruction counts (roofline_fp64_valu) and HBM traffic (roofline.traffic, hbm_traffic) are read from the "
                                    "committed rocprofv3 PMC passes under profiles/ (newest round), not counted in this run; every time in this "
                                    "line is measured in this run; a figure is refused when the committed pass does not hold exactly the kernels that ran")
            out["roofline"] = {
                "bound": "hbm",
                "kernel": rt_variant if dom == "k_raytrace" else dom,
                "stage": dom,
                "achieved": achieved,
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBPS,
                "peak_measured_copy": copy_gbps,
                "frac_of_measured_copy": (achieved / copy_gbps) if copy_gbps else None,
                "traffic": dom_traffic,
                "traffic_over_algorithmic": (dom_traffic / alg_bytes) if dom_traffic else None,
                "algorithmic_bytes_per_launch": int(alg_bytes),
                "avg_kernel_ms": kern,
                "profiled_pass": PROFILED_PASS.get(id(ctx)),
                "whole_step": {"algorithmic_bytes": int(syn.algorithmic_bytes()), "achieved": syn.algorithmic_bytes() / (ms_per_step * 1e-3) / 1e9,
                               "frac": syn.algorithmic_bytes() / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBPS},
                "per_kernel_traffic": traffic_table(args.workload, kern, {"k_line_all": 8 * (n_l * (1 + 2 * nd + g_cols) + nus.size + nd * count),
                                                                            "k_raytrace": 16 * nd * count, "step": syn.algorithmic_bytes()}) if world == 1 else None,
                "note": "path is fp64-VALU bound (Faddeeva evaluations), not HBM bound: see DESIGN.md and roofline_fp64_valu; peak = the data sheet's 8 TB/s, "
                        "peak_measured_copy = a device-to-device copy timed in this run (read + write)",
                "voigt_evaluations_per_s": (evals / world) / (line_ms * 1e-3) if (line_ms and evals is not None) else None,
                "voigt_evaluations_per_s_is": "the reference's window points (sum of hi - lo) per second of the line kernel: nominal where the far "
                                              "field is on (see voigt_evaluations_performed)",
                "voigt_evaluations_performed": performed_evaluations(w, far_on) if world == 1 else None,
            }
        if world > 1:
            out["collective"] = collective_info(world, runner)
            if spectrum is not None:
                out["gathered_spectrum_sha256_16"] = sha16(spectrum)
                if n1 is not None:
                    out["gathered_spectrum_equals_n1_bit_for_bit"] = bool(n1.get("spectrum_sha256_16") == sha16(spectrum))
                    ref = n1.pop("_spectrum", None)
                    if ref is not None and ref.shape == np.shape(spectrum):  # (0.0 where the bits agree; the north star asks for 1e-10)
                        out["max_rel_dev_vs_n1"] = float(np.max(np.abs(np.asarray(spectrum, dtype=np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)))
            if n1 is not None:
                n1.pop("_spectrum", None)
            if per_rank is not None:
                out["per_rank"] = per_rank
            out["config"]["shards"] = [[int(b), int(c)] for b, c in (runner.shards or [])] or "equal blocks of ceil(N_nu / N)"
            if n1 is not None:
                out["n1_same_workload"] = n1
                out["speedup_vs_n1"] = n1["ms_per_step"] / ms_per_step
                # the denominator a driver needs for scaling efficiency: `value` at N = 1 is a DIFFERENT workload (S-c2, the 1-GPU
                # config); this is the N = 1 value of THIS line's workload, measured in this run
                out["value_n1_same_workload"] = n1["value"]
        valu = profiled_valu(args.workload, kern) if world == 1 and args.full else None
        if valu is not None:
            out["roofline_fp64_valu"] = valu
        if world == 1 and args.full and check:
            base, F_cpu = cpu_baseline(w)
            out["cpu_baseline"] = base
            F_gpu = flux.cpu().numpy()
            out["parity_vs_cpu_oracle"] = {
                "emergent_flux_max_rel_err": float(np.max(np.abs(F_gpu[-1] - F_cpu[-1]) / np.abs(F_cpu[-1]))),
                "F_nu_max_rel_err": float(np.max(np.abs(F_gpu[1:] - F_cpu[1:]) / np.abs(F_cpu[1:]))),
            }
            out["speedup_vs_cpu_baseline"] = value / base["value"]
        if pipelined is not None:
            out["throughput_two_syntheses_in_flight"] = pipelined
        if world == 1 and args.full and not args.no_secondary:
            runner.close()
            out["secondary"] = {tag: secondary_block(tag, local, 10, check) for tag in ("S-c3", "S-c4m")}
            out["secondary"]["S-c5"] = s_c5_block(local, 10, check)
            out["secondary"]["S-c4m-linelist"] = linelist_block("S-c4m", local, 10)
            out["dropin"] = dropin_block(local, check)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
