"""A/B of two builds of the library in ONE session, every measurement in a child process of its own (STARDIS_AMD_LIB), the builds
alternated round by round (clocks drift between sessions and within one):

  python scripts/lib_ab.py kernels OLD.so NEW.so [TAG] [ROUNDS] [OPTION=VALUE ...]
      event-timed kernels of the fused step (200 profiled eager steps after 0.5 s of settling) and the wall time of 500 plain
      steps; OPTION=VALUE adds a third leg: the NEW library with that context option set (e.g. wide_list=0)
  python scripts/lib_ab.py bench OLD.so NEW.so [RUNS]
      `python bench.py` at its defaults, RUNS times per build, interleaved, the first of each discarded; then one
      `--steps 20 --warmup 5` pair

  python scripts/lib_ab.py stages OLD.so NEW.so [ROUNDS] [OUT.json]
      the broadening stages (rotation, cell-integrated rotation, macroturbulence; forward with every output, adjoint with nus and
      reference).  Bits: SHA-256 of every output on seeded small grids (n = 2, 3, 8, 9, 17 around the group of eight; a non-uniform
      grid whose expected window crosses the threshold between the eight-lane mapping and a wave per point; V = 0 and zeta = 0, the copy;
      with and without a reference; every window at an end of a grid is truncated) and one S-c2-sized call, device entries and
      host-buffer twins — every hash must agree.  Time: per stage name (sdx_profile_get) the six kernels at S-c2 with V = 2, 10, 100
      km/s and at S-c3 with V = 10, and the wall time of one forward and one adjoint host-buffer twin, ROUNDS children per build,
      alternated.  The bar: the new median within the old leg's own max - min of the old median.

  python scripts/lib_ab.py adjoints OLD.so NEW.so [ROUNDS] [OUT.json]
      the line adjoints (sdx_line_adjoint_dev, sdx_line_param_adjoint_dev) and the line tangent's host entry.  Bits: SHA-256 of every output
      on the six seeded models of tests/line_adjoint_truth.py (every class of item, gamma_cols = 1, tiled windows and the wing shortcut,
      partial last tiles), each entry in the forms that differ in storage (out_line, out_line_depth, both; all six outputs, one per
      line, one per depth; a strength direction, four directions per depth), the three host-buffer twins, the tests' shards, both
      adjoints of the tiled models at adjoint_partials = 1, 100, 160 and 1 << 22, and one S-c2 call per stage through
      SpectralSynthesizer — every hash must agree, also among the children of one build (the item lists' order depends on the run,
      the sums do not).  Time: per stage name the median of 31 single profiled calls at S-c2 and S-c3, per line and per depth
      (k_line_tangent: an unchanged control), and the wall time of sdx_line_param_adjoint_f64 at S-c2.  The bar as for `stages`.

  python scripts/lib_ab.py columns OLD.so NEW.so [ROUNDS] [OUT.json]
      the products of the formal solution over the grid's columns (contribution, emergent intensity, response, response_angles, mean
      intensity, scatter source, mean-intensity adjoint, scatter response: device entry and host-buffer twin each, and
      sdx_raytrace_f64).  Bits: SHA-256 of every output of the calls of tests/test_gpu_column_entries.py — 2, 3, 9 depths x 1, 3, 20, 64
      angles x 1, 7 frequencies, every form — and of one call each at S-c2's size; every hash must agree.  Time, host code only: 500
      enqueues of each device entry at 7 frequencies, and one call of each twin at S-c2's size.  The bar as for `stages`.

  python scripts/lib_ab.py engine OLD_TREE NEW_TREE [ROUNDS] [OUT.json]
      two trees of the PYTHON package on the one built library (the refactors of stardis_amd/engine.py and radiation_field/fused.py): each
      child puts its tree in front of sys.path.  Bits: SHA-256 of every output of SpectralSynthesizer on the small workload of
      tests/test_gpu_engine.py — dense sorted (with and without the plan), dense unsorted and a LineList, each with the continuum flux
      and as a shard of the middle third; eager, captured, capture(batch=3), a step after close(); the two-collective mode, eager and captured, on the long-list shard
      of tests/test_gpu_round5.py (the library refuses it on anything smaller); then
      everything asked on demand behind a step with every kept plane and a rotating, macroturbulent instrument (contribution,
      responses, sensitivities for every wrt, tangents, the instrument's transposes and Jacobian, the chi-square calls with
      curvature) — and of one drop-in run per branch fused.py's step call had.  Time at S-c2, constructed as bench.py constructs it,
      with the plan and with grid_plan=False: 500 eager enqueue() to one synchronize (`step_us`), the host time of that loop alone, 500
      captured step().  The bar as for `stages`.

Prints mean, max - min, min and max per leg.  The other build: a copy of csrc/ at the other revision, `make -C` there."""
import hashlib
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


STAGES = ("k_rotate", "k_rotate_adjoint", "k_rotate_integrated", "k_rotate_integrated_adjoint", "k_macroturbulence", "k_macroturbulence_adjoint")
STAGE_TIMES = {"S-c2": (2.0, 10.0, 100.0), "S-c3": (10.0,)}


def stage_calls(ctx, lam, f, g, u, ur, nus, V, eps, zeta):
    """every stage entry on device buffers -> {entry: ([outputs], stage name, call)}; g = None: no reference"""
    import numpy as np

    n = lam.size
    d = {k: (None if a is None else ctx.upload(a)) for k, a in dict(lam=lam, f=f, g=g, u=u, ur=ur, nus=nus).items()}
    rot, mac = ctx.upload(np.array([V, eps])), ctx.upload(np.array([zeta]))
    ptr = lambda a: None if a is None else a.ptr  # noqa: E731
    outs = lambda k: [ctx.empty((n,)) if g is not None or i % 2 == 0 else None for i in range(k)]  # noqa: E731
    res = {}
    for entry, stage, scalars, k in (("sdx_rotate_dev", "k_rotate", rot, 2), ("sdx_rotate_tangent_dev", "k_rotate_tangent", rot, 4),
                                     ("sdx_rotate_integrated_dev", "k_rotate_integrated", rot, 6), ("sdx_macroturbulence_dev", "k_macroturbulence", mac, 4)):
        o = outs(k)
        res[entry] = (o, stage, lambda entry=entry, scalars=scalars, o=o: ctx.call(
            entry, n, d["lam"].ptr, d["f"].ptr, ptr(d["g"]), scalars.ptr, *map(ptr, o)))
    for name, scalars in (("rotate", rot), ("rotate_integrated", rot), ("macroturbulence", mac)):
        o = outs(2)
        res[f"sdx_{name}_adjoint_dev"] = (o, f"k_{name}_adjoint", lambda name=name, scalars=scalars, o=o: ctx.call(
            f"sdx_{name}_adjoint_dev", n, d["lam"].ptr, scalars.ptr, d["u"].ptr, ptr(d["ur"] if g is not None else None), d["nus"].ptr, *map(ptr, o)))
    return res


def stage_twins(ctx, lam, f, g, u, ur, nus, V, eps, zeta):
    """the host-buffer twins -> {entry: ([outputs], call)}"""
    import numpy as np

    n = lam.size
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    outs = lambda k: [np.empty(n) if g is not None or i % 2 == 0 else None for i in range(k)]  # noqa: E731
    res = {}
    for entry, scalars, k in (("sdx_rotate_f64", (V, eps), 2), ("sdx_rotate_tangent_f64", (V, eps), 4), ("sdx_rotate_integrated_f64", (V, eps), 6),
                              ("sdx_macroturbulence_f64", (zeta,), 4)):
        o = outs(k)
        res[entry] = (o, lambda entry=entry, scalars=scalars, o=o: ctx.call(entry, n, ptr(lam), ptr(f), ptr(g), *scalars, *map(ptr, o)))
    for name, scalars in (("rotate", (V, eps)), ("rotate_integrated", (V, eps)), ("macroturbulence", (zeta,))):
        o = outs(2)
        res[f"sdx_{name}_adjoint_f64"] = (o, lambda name=name, scalars=scalars, o=o: ctx.call(
            f"sdx_{name}_adjoint_f64", n, ptr(lam), *scalars, ptr(u), ptr(ur if g is not None else None), ptr(nus), *map(ptr, o)))
    return res


def stage_inputs(lam, seed):
    import numpy as np
    from stardis_amd import constants as K

    rng = np.random.default_rng(seed)
    draw = lambda: rng.uniform(0.2, 1.0, lam.size)  # noqa: E731
    return dict(lam=lam, f=draw(), g=1.0 + 0.1 * draw(), u=draw() - 0.6, ur=draw() - 0.6, nus=K.C_CGS * 1.0e8 / lam)


def workload_lambdas(tag):
    import numpy as np
    from stardis_amd import constants as K
    from stardis_amd import synth

    w = synth.WORKLOADS[tag]
    return np.ascontiguousarray(K.nu_to_angstrom(synth.tracing_grid(w["lam0"], w["lam1"], R=w["R"])))


def stages_child():
    import numpy as np
    from stardis_amd import _lib
    from stardis_amd import constants as K

    ctx = _lib.Context(0)
    rng = np.random.default_rng(20250926)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    # ---- bits
    grids = {f"n={n}": 6000.0 + np.cumsum(rng.uniform(0.02, 0.08, n)) for n in (2, 3, 8, 9, 17)}
    lam = 5000.0 + np.cumsum(rng.uniform(0.2, 1.8, 400) * (1250.0 / 400))
    # the expected window (2 beta lam (n - 1) / span points) is kObsShort = 32 at the grid's median: groups on both sides of the threshold
    V_cross = 32.0 * (lam[-1] - lam[0]) / (2.0 * np.median(lam) * (lam.size - 1)) * K.C_KMS
    grids["non-uniform 400"] = lam
    grids["S-c2"] = workload_lambdas("S-c2")
    hashes = {}
    for name, lam in grids.items():
        settings = {"V=25": (25.0, 25.0 / 6)} if name != "non-uniform 400" else {"threshold": (V_cross, V_cross / 6), "V=40": (40.0, 40.0 / 6)}
        if name in ("n=9", "non-uniform 400"):
            settings["copy"] = (0.0, 0.0)
        for label, (V, zeta) in settings.items():
            for normal in (False, True):
                a = stage_inputs(lam, 7)
                if not normal:
                    a["g"] = None
                case = {}
                for entry, (outs, _, call) in stage_calls(ctx, V=V, eps=0.6, zeta=zeta, **a).items():
                    call()
                    ctx.synchronize()
                    case[entry] = [None if o is None else sha(o.numpy()) for o in outs]
                if name != "S-c2" or normal:
                    for entry, (outs, call) in stage_twins(ctx, V=V, eps=0.6, zeta=zeta, **a).items():
                        call()
                        case[entry] = [None if o is None else sha(o) for o in outs]
                hashes[f"{name}, {label}, {'with' if normal else 'no'} reference"] = case
    # ---- time: the median over 31 single profiled calls per stage, then the twins' wall time (each call ends in a synchronize)
    times = {}
    for tag, velocities in STAGE_TIMES.items():
        a = stage_inputs(workload_lambdas(tag), 11)
        for V in velocities:
            calls = stage_calls(ctx, V=V, eps=0.6, zeta=V / 6.0, **a)
            ctx.call("sdx_profile_enable", 1)
            for entry, (_, stage, call) in calls.items():
                if stage not in STAGES:
                    continue
                for _ in range(3):
                    call()
                us = []
                for _ in range(31):
                    ctx.call("sdx_profile_reset")
                    call()
                    ctx.synchronize()
                    us.append(ctx.profile(stage)[1] * 1e3)
                times[f"{tag} V={V:g} {stage}"] = float(np.median(us))
            ctx.call("sdx_profile_enable", 0)
            if tag == "S-c2" and V == 10.0:
                twins = stage_twins(ctx, V=V, eps=0.6, zeta=V / 6.0, **a)
                for entry in ("sdx_rotate_f64", "sdx_rotate_adjoint_f64"):
                    call = twins[entry][1]
                    for _ in range(5):
                        call()
                    ts = []
                    for _ in range(30):
                        t0 = time.perf_counter()
                        call()
                        ts.append((time.perf_counter() - t0) * 1e6)
                    times[f"{tag} V={V:g} {entry} wall"] = float(np.median(ts))
    print(json.dumps({"hashes": hashes, "us": times}))


ADJ_STAGES = ("k_line_adjoint", "k_line_param_adjoint", "k_line_tangent")
ADJ_MODELS = ("tiny", "odd", "small", "ragged", "long", "inner")  # tests/line_adjoint_truth.py: every class, gamma_cols = 1, tiled windows
ADJ_SHARDS = (("small", (0, 100)), ("small", (100, 120)), ("small", (220, 80)), ("long", (1500, 6000)), ("inner", (3000, 6000)), ("inner", (5000, 7001)))
ADJ_PARTIALS = (1, 100, 160, 1 << 22)  # `long`, `inner`: one supertile, two, three, every tile a supertile of its own
ADJ_PARAMS = ("damping", "doppler", "centre")


def adjoint_calls(ctx, m, shard=None):
    """the forms of the three device entries on a model of tests/line_adjoint_truth.py -> {form: [host outputs]}"""
    import numpy as np
    from stardis_amd import ops

    b, n = (0, m.n_nu) if shard is None else shard
    nl, nd, L = m.n_lines, m.n_depth, m.lines
    ptr = lambda a: None if a is None else a.ptr  # noqa: E731
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], m.W[:, b:b + n])]
    head = (nd, m.n_nu, d[0].ptr, b, n, nl, d[1].ptr, d[2].ptr, d[3].ptr, L["gammas"].shape[1], d[4].ptr, d[5].ptr, n)
    res = {}
    for form, want in (("out_line", (1, 0)), ("out_line_depth", (0, 1)), ("both", (1, 1))):  # (sld: scratch, the caller's buffer, the caller's)
        o = [ctx.zeros(s) if w else None for s, w in zip(((nl,), (nl, nd)), want)]
        ctx.call("sdx_line_adjoint_dev", *head, *map(ptr, o))
        res[f"sdx_line_adjoint_dev {form}"] = o
    for form, want in (("all six", (1,) * 6), ("damping per line", (1, 0, 0, 0, 0, 0)), ("centre per depth", (0, 0, 0, 0, 0, 1))):
        o = [ctx.zeros((nl,) if k < 3 else (nl, nd)) if w else None for k, w in enumerate(want)]
        ctx.call("sdx_line_param_adjoint_dev", *head, *map(ptr, o))
        res[f"sdx_line_param_adjoint_dev {form}"] = o
    rng = np.random.default_rng(3)
    for form, dirs in (("strength", dict(strength=rng.standard_normal(nl))),
                       ("four per depth", {k: rng.standard_normal((nl, nd)) * (1.0 if k != "centre" else 1e9) for k in ops.LINE_DIRECTIONS})):
        res[f"sdx_line_tangent_dev {form}"] = [ops.line_tangent(nd, m.nus, L["line_nus"], L["doppler_widths"], L["gammas"], L["alphas"], ctx=ctx, device=True,
                                                                shard=shard, **dirs)]
    ctx.synchronize()
    return {k: [None if o is None else np.array(o.numpy()) for o in outs] for k, outs in res.items()}


def adjoint_twins(ctx, nd, nus, L, W):
    """the three host-buffer twins -> {entry: ([outputs], call)}"""
    import numpy as np

    nl = L["line_nus"].size
    tables = [np.ascontiguousarray(L[k]) for k in ("line_nus", "doppler_widths", "gammas", "alphas")]
    head = (nd, nus.size, nus.ctypes.data, nl, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, tables[2].shape[1], tables[3].ctypes.data)
    order = np.argsort(tables[0], kind="stable")  # (the tangent wants an ascending list)
    asc = [np.ascontiguousarray(t[order]) for t in tables]
    dirs = [np.ascontiguousarray(np.random.default_rng(5).standard_normal((nl, nd)) * s) for s in (1.0, 1.0, 1.0, 1e9)]
    res = {}
    o1 = [np.zeros(nl), np.zeros((nl, nd))]
    res["sdx_line_adjoint_f64"] = (o1, lambda: ctx.call("sdx_line_adjoint_f64", *head, W.ctypes.data, *(o.ctypes.data for o in o1)))
    o2 = [np.zeros(nl) for _ in range(3)] + [np.zeros((nl, nd)) for _ in range(3)]
    res["sdx_line_param_adjoint_f64"] = (o2, lambda: ctx.call("sdx_line_param_adjoint_f64", *head, W.ctypes.data, *(o.ctypes.data for o in o2)))
    o3 = [np.zeros((nd, nus.size))]
    res["sdx_line_tangent_f64"] = (o3, lambda: ctx.call("sdx_line_tangent_f64", nd, nus.size, nus.ctypes.data, nl, *(t.ctypes.data for t in asc[:3]),
                                                        asc[2].shape[1], asc[3].ctypes.data, *(v.ctypes.data for v in dirs), nd, o3[0].ctypes.data))
    return res


def adjoints_child():
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import line_adjoint_truth as A
    from stardis_amd import _lib, synth
    from stardis_amd.engine import SpectralSynthesizer

    ctx = _lib.Context(0)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    digest = lambda forms: {k: [None if o is None else sha(o) for o in outs] for k, outs in forms.items()}  # noqa: E731
    # ---- bits
    hashes = {}
    for name in ADJ_MODELS:
        m = A.model(name)
        case = digest(adjoint_calls(ctx, m))
        for entry, (outs, call) in adjoint_twins(ctx, m.n_depth, m.nus, m.lines, m.W).items():
            call()
            case[entry] = [sha(o) for o in outs]
        hashes[name] = case
    for name, shard in ADJ_SHARDS:
        hashes[f"{name}, shard {shard}"] = digest(adjoint_calls(ctx, A.model(name), shard))
    try:
        for name in ("long", "inner"):
            for partials in ADJ_PARTIALS:
                ctx.set_option("adjoint_partials", partials)
                forms = adjoint_calls(ctx, A.model(name))
                hashes[f"{name}, adjoint_partials = {partials}"] = digest({k: v for k, v in forms.items() if "tangent" not in k})
    finally:
        ctx.set_option("adjoint_partials", 1 << 22)
    # ---- the engine at S-c2 (bits and time) and S-c3 (time), driven as scripts/line_param_sensitivity_cost.py drives it: the median
    # of 31 single profiled calls per stage name
    times = {}
    for tag in ("S-c2", "S-c3"):
        w = synth.make_workload(tag)
        atm, L = w["atm"], w["lines"]
        nd, nl = int(atm["temperatures"].size), int(L["line_nus"].size)
        syn = SpectralSynthesizer(w["nus"], atm["temperatures"], atm["dist"], w["thetas"], w["weights"], L, w["cont"], ctx=ctx, track_evaluations=False,
                                  keep_line=False, keep_response=True)
        d_weights = ctx.upload(np.random.default_rng(1).standard_normal(w["nus"].size))
        syn.step()
        ctx.synchronize()
        rng = np.random.default_rng(2)
        for per_depth in (False, True):
            dirs = [rng.standard_normal((nl, nd) if per_depth else (nl,)) * s for s in (1.0, 1.0, 1.0, 1e9)]
            calls = {"k_line_adjoint": lambda: syn.line_sensitivities(d_weights, per_depth=per_depth),
                     "k_line_param_adjoint": lambda: syn.line_sensitivities(d_weights, per_depth=per_depth, wrt=ADJ_PARAMS),
                     "k_line_tangent": lambda: syn.line_tangent(*dirs)}
            label = f"{tag} per {'depth' if per_depth else 'line'}"
            if tag == "S-c2":
                case = {}
                for stage, call in calls.items():
                    out = call()
                    ctx.synchronize()
                    case[stage] = [sha(o.numpy()) for o in (out.values() if isinstance(out, dict) else [out])]
                hashes[f"engine, {label}"] = case
            ctx.call("sdx_profile_enable", 1)
            for stage, call in calls.items():
                for _ in range(3):
                    call()
                us = []
                for _ in range(31):
                    ctx.call("sdx_profile_reset")
                    call()
                    ctx.synchronize()
                    us.append(ctx.profile(stage)[1] * 1e3)
                times[f"{label} {stage}"] = float(np.median(us))
            ctx.call("sdx_profile_enable", 0)
        if tag == "S-c2":  # the wall time of a host-buffer twin (each call ends in a synchronize)
            W = np.random.default_rng(4).standard_normal((nd, w["nus"].size))
            call = adjoint_twins(ctx, nd, np.ascontiguousarray(w["nus"]), L, W)["sdx_line_param_adjoint_f64"][1]
            for _ in range(5):
                call()
            ts = []
            for _ in range(30):
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e6)
            times[f"{tag} sdx_line_param_adjoint_f64 wall"] = float(np.median(ts))
        syn.close()
    print(json.dumps({"hashes": hashes, "us": times}))


def columns_child():
    """one leg of `columns`: the calls of tests/test_gpu_column_entries.py, hashed and timed"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_column_entries as T
    from stardis_amd import _lib, synth

    ctx = _lib.Context(0)
    w = synth.WORKLOADS["S-c2"]
    big = T.Problem(ctx, int(synth.solar_atmosphere()["temperatures"].size), synth.N_THETAS, int(synth.tracing_grid(w["lam0"], w["lam1"], R=w["R"]).size))
    shapes = [(f"{nd} depths, {nt} angles, {nn} frequencies", T.Problem(ctx, nd, nt, nn)) for nd in T.DEPTHS for nt in T.ANGLES for nn in T.FREQUENCIES]
    hashes = {}
    for label, p in shapes + [("S-c2 size", big)]:
        case = {}
        for entry in T.DEVICE:
            for twin in (False, True):  # one hash per entry: every output of every form, in order
                h = hashlib.sha256()
                for form in (T.forms(entry) if p is not big else [{}]):
                    for name, a in p.run(entry, twin, form).items():
                        h.update(name.encode() + (b"-" if a is None else np.ascontiguousarray(a).tobytes()))
                case[f"sdx_{entry}_{'f64' if twin else 'dev'}"] = h.hexdigest()
        hashes[label] = case
    times = {}
    small = T.Problem(ctx, 9, synth.N_THETAS, 7)
    for entry in T.PRODUCTS:  # the host cost of a device entry: 500 enqueues at 7 frequencies, then one synchronize
        outs = small.outputs(entry, False, {})
        args = small.arguments(entry, False, {}, outs)
        for _ in range(50):
            ctx.call(f"sdx_{entry}_dev", *args)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            ctx.call(f"sdx_{entry}_dev", *args)
        times[f"sdx_{entry}_dev enqueue"] = (time.perf_counter() - t0) / 500 * 1e6
        ctx.synchronize()
    for entry in T.DEVICE:  # one twin call at S-c2 size (each ends in a synchronize): the median of seven
        outs = big.outputs(entry, True, {})
        args = big.arguments(entry, True, {}, outs)
        ts = []
        for k in range(9):
            t0 = time.perf_counter()
            ctx.call(f"sdx_{entry}_f64", *args)
            ts.append((time.perf_counter() - t0) * 1e6)
        times[f"S-c2 sdx_{entry}_f64 wall"] = float(np.median(ts[2:]))
    print(json.dumps({"hashes": hashes, "us": times}))


ENGINE_WRT = ("strength", "damping", "doppler", "centre")


def engine_child(tree):
    """one leg of `engine`: the Python tree `tree` in front of sys.path, the library STARDIS_AMD_LIB names"""
    sys.path.insert(0, os.path.abspath(tree))
    import struct
    import types

    import numpy as np
    import stardis_amd
    from stardis_amd import _lib, synth
    from stardis_amd import constants as K
    from stardis_amd.engine import SpectralSynthesizer
    from stardis_amd.instrument import Instrument

    assert os.path.abspath(stardis_amd.__file__).startswith(os.path.abspath(tree) + os.sep), stardis_amd.__file__
    ctx = _lib.Context(0)

    def sha(a):
        if a is None or isinstance(a, str):
            return a
        if isinstance(a, dict):
            return {k: sha(v) for k, v in a.items()}
        if isinstance(a, (tuple, list)):
            return [sha(v) for v in a]
        if isinstance(a, float):
            return hashlib.sha256(struct.pack("<d", a)).hexdigest()
        if isinstance(a, int):
            return a
        return hashlib.sha256(np.ascontiguousarray(a.numpy() if hasattr(a, "ptr") else a).tobytes()).hexdigest()

    # ---- bits: the workload of tests/test_gpu_engine.py::small_workload (300 lines, ~500 frequencies, 56 depths, 8 angles)
    atm = synth.solar_atmosphere()
    nus = synth.tracing_grid(6560.0, 6570.0, step=0.02)
    dense = synth.synth_lines(nus, atm, 300, seed=11, mix=(0.8, 0.15, 0.05))
    perm = np.random.default_rng(3).permutation(300)
    lists = {"dense sorted": dense, "dense unsorted": {k: np.ascontiguousarray(v[perm]) for k, v in dense.items()},
             "line list": synth.synth_linelist(nus, atm, 300, seed=11)}
    cont = synth.synth_continuum_state(atm)
    th, w = synth.thetas_and_weights(8)
    make = lambda lines, **kw: SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, **kw)  # noqa: E731

    def planes(syn):
        out = dict(F_nu=syn.F_nu(), alpha_line=syn.alpha_line(), total_alphas=syn.total_alphas(), evaluations=syn.evaluations())
        if syn.keep_continuum_flux:
            out["F_nu_continuum"] = syn.F_nu_continuum
        return sha(out)

    hashes = {}
    third = nus.size // 3
    for name, lines in lists.items():
        variants = {"": {}, ", continuum": dict(keep_continuum_flux=True), ", shard": dict(shard=(third, third))}
        if name == "dense sorted":
            variants[", grid_plan=False"] = dict(grid_plan=False)
            variants[", grid_plan=False, continuum"] = dict(grid_plan=False, keep_continuum_flux=True)
        for label, kw in variants.items():
            syn = make(lines, **kw)
            case = {}
            syn.enqueue()
            case["eager"] = planes(syn)
            syn.capture(batch=3)
            for mode, step in (("captured", syn.step), ("batch of 3", syn.step_batch)):
                syn.d_F.zero()
                step()
                case[mode] = planes(syn)
            syn.close()
            syn.d_F.zero()
            syn.step()
            case["after close()"] = planes(syn)
            hashes[name + label] = case
    # the two-collective mode, the whole list as the share.  The library takes it on frequency shards of long lists alone: the case of
    # tests/test_gpu_round5.py (9000 lines, the second quarter of 20000 frequencies)
    long_nus = synth.tracing_grid(5000.0, 5000.0 * (1.0 + 1.02 * 20000 / 1.0e5), R=1.0e5)[:20000]
    long_lines = synth.synth_lines(long_nus, atm, 9000, seed=3, mix=(0.85, 0.12, 0.03))
    for label, kw in (("", {}), (", continuum", dict(keep_continuum_flux=True))):
        syn = SpectralSynthesizer(long_nus, atm["temperatures"], atm["dist"], th, w, long_lines, cont, ctx=ctx, shard=(5000, 5000), track_evaluations=False,
                                  classify_share=(0, 9000), m_max=ctx.zeros((9000,)), **kw)
        case = {}
        syn.enqueue_classify()
        syn.enqueue()
        case["eager"] = planes(syn)
        syn.capture()
        syn.d_F.zero()
        syn.step_classify()
        syn.step()
        case["captured"] = planes(syn)
        syn.close()
        hashes["two-collective" + label] = case

    # ---- bits: everything that is asked on demand, behind a step with every kept plane and a broadening instrument
    edges = np.r_[6560.75, 6561.2, np.linspace(6562.0, 6568.0, 25), 6571.0]  # (tests/test_gpu_macroturbulence.py: edge-affected and NaN pixels)
    rng = np.random.default_rng(7)
    col_w, pix_c, xi = rng.standard_normal(nus.size), rng.standard_normal(edges.size - 1), 1.5e5
    direction, dF, dFc = rng.standard_normal(300), rng.standard_normal(nus.size), rng.standard_normal(nus.size)
    noise, ivar = rng.standard_normal(edges.size - 1), rng.uniform(0.5, 2.0, edges.size - 1)
    ivar[5] = 0.0
    for name, lines in lists.items():
        inst = Instrument(edges, sigma=0.05, ctx=ctx, v_rot=10.0, v_mac=3.0)
        inst.set_radial_velocity(12.0)
        syn = make(lines, keep_continuum_flux=True, keep_contribution=True, keep_response=True, instrument=inst)
        case = {}
        for mode, step in (("eager", syn.enqueue), ("unfused", syn.enqueue_unfused), ("captured", lambda: syn.capture().step())):
            syn.d_F.zero()
            step()
            case[mode] = sha(dict(planes=planes(syn), contribution=syn.contribution, response_opacity=syn.response_opacity,
                                  response_source=syn.response_source, observed=syn.observed, observed_normalized=syn.observed_normalized))
        part = syn.alpha_line()
        case["formation_mean"] = sha([syn.formation_mean(atm["temperatures"]), syn.formation_mean(ctx.upload(np.asarray(atm["temperatures"], dtype=np.float64)))])
        case["flux_derivative"] = sha([syn.flux_derivative(part), syn.flux_derivative(ctx.upload(part))])
        for per_depth in (False, True):
            for wrt in ENGINE_WRT + (ENGINE_WRT,):
                case[f"line_sensitivities {wrt} per_depth={per_depth}"] = sha([syn.line_sensitivities(col_w, per_depth, wrt), syn.line_sensitivities(None, per_depth, wrt)])
        case["line_sensitivities device weights"] = sha(syn.line_sensitivities(ctx.upload(col_w)))
        case["line_tangent"] = sha([syn.line_tangent(strength=direction), syn.line_tangent(damping=0.5, centre=direction * 1e8)])
        case["flux_tangent"] = sha(syn.flux_tangent(doppler=direction))
        case["microturbulence"] = sha([syn.microturbulence_sensitivity(xi, col_w), syn.microturbulence_sensitivity(xi), syn.microturbulence_tangent(xi)])
        for normalized in (False, True):
            tag = f" normalized={normalized}"
            case["pixel_weights_to_grid" + tag] = sha([syn.pixel_weights_to_grid(pix_c, normalized), syn.pixel_weights_to_grid(ctx.upload(pix_c), normalized, True)])
            case["observed_tangent" + tag] = sha([syn.observed_tangent(dF, dFc if normalized else None, normalized), syn.observed_tangent(ctx.upload(dF), None, normalized)])
            case["observed_jacobian" + tag] = sha(syn.observed_jacobian(None, normalized))
            case["observed_line_sensitivities" + tag] = sha(syn.observed_line_sensitivities(pix_c, normalized, wrt=ENGINE_WRT))
            case["observed_macroturbulence_derivative" + tag] = sha(syn.observed_macroturbulence_derivative(pix_c, normalized))
            obs = (syn.observed_normalized if normalized else syn.observed).numpy()
            data = np.nan_to_num(obs) * (1.0 + 0.01 * noise)
            directions = {"gf": dict(strength=(direction > 0).astype(np.float64)), "xi": {"microturbulence": xi}}
            case["chi2_line_gradient" + tag] = sha(syn.chi2_line_gradient(data, ivar, normalized, wrt=ENGINE_WRT))
            case["chi2_macroturbulence_gradient" + tag] = sha(syn.chi2_macroturbulence_gradient(data, ivar, normalized))
            case["chi2_instrument_gradient" + tag] = sha(syn.chi2_instrument_gradient(data, ivar, None, normalized, curvature=True))
            case["chi2_joint_gradient" + tag] = sha([syn.chi2_joint_gradient(data, ivar, ("v_rad", "v_mac"), directions, normalized, curvature=True),
                                                     syn.chi2_joint_gradient(data, ivar, (), directions, normalized, curvature=True),
                                                     syn.chi2_joint_gradient(data, ivar, None, None, normalized, curvature=True)])
        syn.close()
        hashes["on demand, " + name] = case

    # ---- bits: the drop-in, one run per branch its step call had
    import stardis_amd.radiation_field.base as rf
    from stardis_amd.radiation_field import fused
    from stardis_amd.radiation_field.source_functions.blackbody import blackbody_flux_at_nu

    NS = types.SimpleNamespace
    for variant in ("plain", "tracked", "source", "spherical", "line list", "molecules"):
        plasma, model, config, _ = synth.fake_plasma(nus, atm, 300, seed=41, n_molecule_lines=200 if variant == "molecules" else 0)
        config.no_of_thetas = 8
        config.result_options = NS(return_radiation_field=variant in ("tracked", "spherical"))
        if variant == "molecules":
            config.opacity.line.include_molecules = True
        if variant == "line list":
            plasma.alpha_line_from_linelist = None
        if variant == "spherical":
            model.spherical = True
            r = 7.0e10 + np.concatenate([[0.0], np.cumsum(np.asarray(model.geometry.dist_to_next_depth_point))])
            model.geometry = NS(dist_to_next_depth_point=model.geometry.dist_to_next_depth_point, r=r, reference_r=r[-12])
        source = (lambda nu, t: 1.0e-13 * t**4 * (nu / nu[0]) ** 2) if variant == "source" else blackbody_flux_at_nu
        for continuum in (False, True):
            field = fused.try_fused(rf.RadiationField, nus.copy(), model, plasma, config, source, continuum=continuum)
            assert field is not None, variant
            case = dict(F_nu=field.F_nu, total_alphas=field.opacities.total_alphas)
            if continuum:
                case["F_nu_continuum"] = field.F_nu_continuum
            if config.result_options.return_radiation_field:
                case["I_nus"] = field.I_nus
            hashes[f"drop-in {variant}, continuum={continuum}"] = sha(case)

    # ---- time at S-c2, constructed as bench.py constructs it: 500 eager enqueue() and their host time alone, 500 captured step()
    wl = synth.make_workload("S-c2")
    times = {}
    for label, kw in (("", {}), (" grid_plan=False", dict(grid_plan=False))):
        syn = SpectralSynthesizer(wl["nus"], wl["atm"]["temperatures"], wl["atm"]["dist"], wl["thetas"], wl["weights"], wl["lines"], wl["cont"], ctx=ctx,
                                  track_evaluations=False, keep_line=False, **kw)
        for step in (syn.enqueue, syn.capture().step):
            t_end = time.perf_counter() + 0.5
            while time.perf_counter() < t_end:
                for _ in range(10):
                    step()
                ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(500):
                step()
            t1 = time.perf_counter()
            ctx.synchronize()
            t2 = time.perf_counter()
            if step == syn.enqueue:
                times["step_us" + label], times["enqueue_host_us" + label] = (t2 - t0) / 500 * 1e6, (t1 - t0) / 500 * 1e6
            else:
                times["captured_step_us" + label] = (t2 - t0) / 500 * 1e6
        syn.close()
    print(json.dumps({"hashes": hashes, "us": times}))


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
    if mode == "stages-child":
        stages_child()
        return
    if mode == "adjoints-child":
        adjoints_child()
        return
    if mode == "columns-child":
        columns_child()
        return
    if mode == "engine-child":
        engine_child(sys.argv[2])
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
    elif mode in ("stages", "adjoints", "columns", "engine"):
        rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
        res = {"old": [], "new": []}
        built = os.environ.get("STARDIS_AMD_LIB") or os.path.join(ROOT, "stardis_amd", "lib", "libstardis_hip.so")
        for r in range(rounds):
            for name, leg in (("old", old), ("new", new)):
                # (engine: the legs are two Python trees on the one built library)
                lib, argv = (built, ["engine-child", os.path.abspath(leg)]) if mode == "engine" else (leg, [mode + "-child"])
                res[name].append(spawn(lib, [os.path.abspath(__file__)] + argv, 300))
                print(r, name, {k: round(v, 2) for k, v in res[name][-1]["us"].items()}, flush=True)
        hashes = [r["hashes"] for rows in res.values() for r in rows]
        differing = sorted({f"{case}: {entry}" for h in hashes[1:] for case in h for entry in h[case] if h[case][entry] != hashes[0][case][entry]})
        count = lambda v: sum(map(count, v.values() if isinstance(v, dict) else v)) if isinstance(v, (dict, list)) else int(isinstance(v, str))  # noqa: E731
        n_hashes = count(hashes[0])
        print(f"{n_hashes} hashes per child, {len(hashes)} children: {'ALL EQUAL' if not differing else 'DIFFERENT: ' + '; '.join(differing)}")
        within = {name: all(r["hashes"] == rows[0]["hashes"] for r in rows) for name, rows in res.items()}  # (the item lists' order depends on the run)
        print("children of the same build agree among themselves:", within)
        summary("old", [r["us"] for r in res["old"]], "us")
        summary("new", [r["us"] for r in res["new"]], "us")
        table, missed = {}, []
        for k in res["old"][0]["us"]:
            o, n = sorted(r["us"][k] for r in res["old"]), sorted(r["us"][k] for r in res["new"])
            row = dict(old_median=o[len(o) // 2], old_spread=o[-1] - o[0], new_median=n[len(n) // 2], new_spread=n[-1] - n[0], old=o, new=n)
            row["within"] = abs(row["new_median"] - row["old_median"]) <= row["old_spread"]
            table[k] = row
            if not row["within"]:
                missed.append(f"{k} ({'slower' if row['new_median'] > row['old_median'] else 'faster'})")
        print("time bar (new median within old max - min of the old median):", "MET" if not missed else "MISSED by " + "; ".join(missed))
        if len(sys.argv) > 5:
            with open(sys.argv[5], "w") as fh:
                json.dump(dict(rounds=rounds, hashes_per_child=n_hashes, hashes_equal=not differing, equal_within_build=within, differing=differing, hashes=hashes[0],
                               us=table, time_bar_missed=missed), fh, indent=1)
    else:
        print(__doc__)


if __name__ == "__main__":
    main()
