"""A/B of two builds of the library in ONE session, every measurement in a child process of its own (STARDIS_AMD_LIB), the builds
alternated round by round (clocks drift between sessions and within one):

  python scripts/lib_ab.py kernels OLD.so NEW.so [TAG] [ROUNDS] [OPTION=VALUE ...]
      event-timed kernels of the fused step (200 profiled eager steps after 0.5 s of settling) and the wall time of 500 plain
      steps; OPTION=VALUE adds a third leg: the NEW library with that context option set (e.g. wide_list=0)
  python scripts/lib_ab.py bench OLD.so NEW.so [RUNS]
      `python bench.py` at its defaults, RUNS times per build, interleaved, the first of each discarded; then one
      `--steps 20 --warmup 5` pair

Prints mean, max - min, min and max per leg.  The other build: a copy of csrc/ at the other revision, `make -C` there."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_prepass_continuum", "k_line_all", "k_raytrace")


def child(tag, options):
    from stardis_amd import _lib, synth
    from stardis_amd.engine import SpectralSynthesizer

    w = synth.make_workload(tag)
    ctx = _lib.Context(0)
    for o in options:
        name, value = o.split("=")
        ctx.set_option(name, int(value))
    syn = SpectralSynthesizer(w["nus"], w["atm"]["temperatures"], w["atm"]["dist"], w["thetas"], w["weights"], w["lines"], w["cont"], ctx=ctx,
                              track_evaluations=False, keep_line=False)
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:
        for _ in range(10):
            syn.enqueue()
        ctx.synchronize()
    ctx.call("sdx_profile_enable", 1)
    ctx.call("sdx_profile_reset")
    n = 200
    for _ in range(n):
        syn.enqueue()
    ctx.synchronize()
    out = {k: ctx.profile(k)[1] / n * 1e3 for k in KERNELS}
    ctx.call("sdx_profile_enable", 0)
    ctx.call("sdx_profile_reset")
    for _ in range(50):
        syn.enqueue()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(500):
        syn.enqueue()
    ctx.synchronize()
    out["step_us"] = (time.perf_counter() - t0) / 500 * 1e6
    print(json.dumps(out))


def spawn(lib, argv, timeout):
    p = subprocess.run([sys.executable] + argv, env=dict(os.environ, STARDIS_AMD_LIB=os.path.abspath(lib)), capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    if p.returncode != 0:  # (a failed leg ends the session: nothing more is started on the device)
        print("FAILED", lib, p.returncode, p.stdout[-1500:], p.stderr[-1500:])
        sys.exit(1)
    return json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])


def summary(label, rows, unit, scale=1.0, drop_first=False):
    for k in rows[0]:
        v = [r[k] * scale for r in rows]
        u = v[1:] if drop_first and len(v) > 2 else v
        print(f"{label:14s} {k:20s} mean {sum(u) / len(u):8.2f} {unit}  max - min {max(u) - min(u):5.2f}  min {min(u):8.2f}  max {max(u):8.2f}   all {[round(x, 2) for x in v]}")


def main():
    mode = sys.argv[1]
    if mode == "child":
        child(sys.argv[2], sys.argv[3:])
        return
    old, new = sys.argv[2], sys.argv[3]
    if mode == "kernels":
        rest = sys.argv[4:]
        options = [a for a in rest if "=" in a]
        rest = [a for a in rest if "=" not in a]
        tag = rest[0] if rest else "S-c2"
        rounds = int(rest[1]) if len(rest) > 1 else 7
        legs = [("old", old, []), ("new", new, [])] + ([("new " + " ".join(options), new, options)] if options else [])
        res = {name: [] for name, _, _ in legs}
        for r in range(rounds):
            for name, lib, opts in legs:
                res[name].append(spawn(lib, [os.path.abspath(__file__), "child", tag] + opts, 180))
                print(r, name, res[name][-1], flush=True)
        for name, rows in res.items():
            summary(f"{tag} {name}", rows, "us")
    elif mode == "bench":
        runs = int(sys.argv[4]) if len(sys.argv) > 4 else 6
        res = {"old": [], "new": [], "old 20 after 5": [], "new 20 after 5": []}
        for r in range(runs):
            for name, lib in (("old", old), ("new", new)):
                j = spawn(lib, [os.path.join(ROOT, "bench.py")], 600)
                res[name].append({"ms_per_step": j["ms_per_step"]})
                print(r, name, j["ms_per_step"], flush=True)
        for name, lib in (("old", old), ("new", new)):
            j = spawn(lib, [os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5"], 600)
            res[name + " 20 after 5"].append({"ms_per_step": j["ms_per_step"]})
        for name, rows in res.items():
            summary(name, rows, "us", 1e3, drop_first=True)
    else:
        print(__doc__)


if __name__ == "__main__":
    main()
