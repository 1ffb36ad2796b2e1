"""Golden fixture of the flux contribution function, from the reference's own formal solution (THIS container only).

    /opt/conda/bin/python3.9 tests/golden/make_golden_contribution.py            write tests/golden/g15_contribution.npz
    /opt/conda/bin/python3.9 tests/golden/make_golden_contribution.py --verify   regenerate into a temporary directory and compare

Inputs: those of g7_raytrace.npz (200 frequencies, 56 depths, N_theta in {1, 4, 20}).  For every angle the reference's
single_theta_trace_parallel runs un-jitted (tests/golden/ref_loader.py; the reference is imported at run time, none of its
text is copied) and gives I (N_d, N_nu).  The step of a gap is the affine map I[g+1] = c[g] I[g] + e[g] with c = 1 - w0, w0 from
the reference's calc_weights on the optical depths of radiation_field_solvers/base.py:121-129 (c = 1 where tau == 0, :203-206 and
:253-254); so e[g] = I[g+1] - c[g] I[g].  With T[N_d-1] = 1, T[k] = T[k+1] c[k] the contribution of the layer below row k to the
emergent flux is

    C[0] = 0,    C[k] = sum_theta w_theta (T[k] e[k-1]),    sum_k C[k] = F_nu[N_d-1] up to rounding

(theta summed in two ascending halves, the lower added to the upper).  Stored: C_1, C_4, C_20, the emergent flux of the same run F_last_1, _4, _20 (sum_theta w_theta I[N_d-1]) and, for x = log10(1 .. N_d), the
formation mean  <x> = (sum_{k>=1} C[k] m_k) / (sum_{k>=1} C[k]),  m_k = (x[k-1] + x[k]) 0.5,  both sums over ascending k.
Columns 7 (opacity 0 everywhere: C = 0, mean NaN) and 11 (opacity 0 at the surface row: the reference's F_nu is NaN) are kept as
the reference gives them.

The two transcendental functions the reference's trace calls, np.exp and np.log, are pinned to their correctly rounded values while
it runs (tests/contribution_reference.py: exact_exp, exact_log; the name `np` in the reference's module is a proxy that forwards
everything else to numpy), and its source function returns g7's stored blackbody plane.  Left to numpy, their last bit depends on the
numpy build and the CPU; the scheme amplifies it (log(alpha) ~ -30; w2 = 2 w1 - tau^2 exp(-tau) cancels six digits in a thin gap)
to 7e-12 of the flux, so a golden made that way could be reproduced to better than 1e-11 only on the machine that made it.  With
the unique correctly rounded values the fixture — every other operation being one IEEE operation — is the same wherever it is made,
and differs from the run on numpy 1.26.4's own functions by 7.0 / 4.4 / 3.1e-12 of F_nu[-1] at 1 / 4 / 20 angles (printed by this
script).
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
NAME = "g15_contribution.npz"


def formation_mean(C, x):
    """The definition, one correctly rounded operation at a time, ascending k."""
    num, den = np.zeros(C.shape[1]), np.zeros(C.shape[1])
    for k in range(1, C.shape[0]):
        m = (x[k - 1] + x[k]) * 0.5
        num = num + C[k] * m
        den = den + C[k]
    with np.errstate(all="ignore"):
        return num / den


class _PinnedNumpy:
    """numpy with exp and log correctly rounded: what the reference's module sees as `np` while the golden is made"""

    def __init__(self):
        import contribution_reference as cref

        self.exp, self.log = cref.exact_exp, cref.exact_log

    def __getattr__(self, name):
        return getattr(np, name)


def contribution(R, g, n_theta, source):
    """C (N_d, N_nu) from the reference's trace of every angle, per the definition above."""
    nus, total, temps, dist = g["nus"], g["total_alphas"].copy(), g["temperatures"], g["dist"]
    n_depth = temps.size
    thetas, weights = g[f"thetas_{n_theta}"], g[f"weights_{n_theta}"]
    terms, flux = [], np.zeros(nus.size)
    for theta, w in zip(thetas, weights):
        rd = dist / np.cos(theta)
        inten = R.rt.single_theta_trace_parallel(rd, temps.reshape(-1, 1), total, nus, source)
        taus = R.rt.np.exp((R.rt.np.log(total[1:]) + R.rt.np.log(total[:-1])) * 0.5) * rd.reshape(-1, 1)  # :121-129
        w0 = R.rt.calc_weights(taus)[0]
        c = np.where(taus == 0, 1.0, 1 - w0)
        flux = flux + w * inten[-1]  # the emergent flux of this run, summed as :324-338 sum it
        e = inten[1:] - c * inten[:-1]
        trans = np.ones((n_depth, nus.size))
        for k in range(n_depth - 2, -1, -1):
            trans[k] = trans[k + 1] * c[k]
        terms.append((trans[1:] * e) * w)
    half = (n_theta + 1) >> 1
    lower, upper = np.zeros_like(terms[0]), np.zeros_like(terms[0])
    for t in terms[:half]:
        lower = lower + t
    for t in terms[half:]:
        upper = upper + t
    C = np.zeros((n_depth, nus.size))
    C[1:] = lower + upper
    return C, flux


def generate(out_dir, compare=False):
    import ref_loader

    R = ref_loader.load()
    g = np.load(os.path.join(HERE, "g7_raytrace.npz"), allow_pickle=False)
    n_depth = g["temperatures"].size
    x = np.log10(np.arange(1, n_depth + 1.0))
    out = dict(x_log10=x)
    blackbody = g["blackbody"]  # the reference's own Planck plane for these inputs, as g7 recorded it
    source = lambda nus, temps: blackbody  # noqa: E731
    plain = R.rt.np
    with np.errstate(all="ignore"):
        for n_theta in (1, 4, 20):
            R.rt.np = _PinnedNumpy()
            try:
                C, flux = contribution(R, g, n_theta, source)
            finally:
                R.rt.np = plain
            out[f"C_{n_theta}"] = C
            out[f"F_last_{n_theta}"] = flux
            out[f"mean_log10_{n_theta}"] = formation_mean(C, x)
            if compare:  # the same run on this numpy's own exp and log
                own = contribution(R, g, n_theta, source)[0]
                F = g[f"F_nu_{n_theta}"][-1]
                ok = np.isfinite(F) & (F != 0)
                print(f"N_theta={n_theta}: pinned exp/log against numpy {np.__version__}'s own: "
                      f"{np.max(np.abs(C[:, ok] - own[:, ok]) / F[ok]):.2e} of F_nu[-1]; sum_k C against this run's emergent flux "
                      f"{np.max(np.abs(C[:, ok].sum(axis=0) - flux[ok]) / F[ok]):.2e}, against g7's F_nu[-1] "
                      f"{np.max(np.abs(C[:, ok].sum(axis=0) - F[ok]) / F[ok]):.2e}")
    np.savez_compressed(os.path.join(out_dir, NAME), **out)


def verify():
    with tempfile.TemporaryDirectory(prefix="golden_verify_") as tmp:
        generate(tmp)
        new, old = np.load(os.path.join(tmp, NAME), allow_pickle=False), np.load(os.path.join(HERE, NAME), allow_pickle=False)
        diffs = [k for k in sorted(set(new.files) | set(old.files))
                 if k not in new.files or k not in old.files or new[k].dtype != old[k].dtype or new[k].shape != old[k].shape
                 or not np.array_equal(new[k], old[k], equal_nan=True)]
    print(f"VERIFY {NAME}: " + ("identical" if not diffs else f"DIFFERS in {diffs[:6]}"))
    return len(diffs)


if __name__ == "__main__":
    if "--verify" in sys.argv[1:]:
        raise SystemExit(1 if verify() else 0)
    generate(HERE, compare=True)
