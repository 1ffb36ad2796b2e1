"""What tests/test_gpu_line_params_truth.py rests on, checked without a GPU: the fp64 oracle alone is within A 2^-53 of the 80-bit truth
on every hostile line list (the same zeros, NaNs and infinities), every class holds what it claims — each branch of each decision of
stardis_amd/csrc/sdx_broadening.h is taken, each boundary has its three items — what a relative bound cannot hold stays out, the bound
on well-conditioned values is below the standing tolerances, and the constants restated in tests/line_params_truth.py are the source's."""
import os
import re

import numpy as np
import pytest

import line_params_truth as T
from conftest import ROOT

pytestmark = pytest.mark.skipif(not T.EXTENDED, reason="numpy.longdouble is not an extended type here")

TABLES = ("gamma", "dw", "alpha", "alpha_short")
SUBNORMAL_CLASSES = {"alpha_exp", "alpha_stim", "modes_2_3"}  # exp's own subnormals; a subnormal population; a subnormal A_ul (inputs)


@pytest.mark.parametrize("n_depth", T.N_DEPTHS)
@pytest.mark.parametrize("cls", T.CLASSES)
def test_oracle_alone_meets_the_criterion(cls, n_depth):
    c = T.case(cls, n_depth)
    for v in c.variants + ((T.Variant(T.GAMMA_VALD, 15, 1e5, False),) if cls in ("waals", "stark") else ()):
        for what in TABLES:
            share = T.judge(c, v, what, T.oracle_tables(c, v)[what], record=None, oracle_alone=True)
            print(f"{c.name:20s} {tuple(v)} {what:11s} oracle at {share:.3f} of A x 2^-53")


def test_the_list_is_of_the_size_asked_for():
    n = sum(c.n_lines for c in T.hostile_line_lists())
    assert 300 <= n <= 700, n
    for c in T.hostile_line_lists():
        assert 3 <= c.n_lines <= 160, c.name
        assert np.all(np.diff(c.nu) >= 0) and c.nu[0] > T.grid()[-1] and c.nu[-1] < T.grid()[0]  # route C: ascending, inside the exact grid


def test_what_a_relative_bound_cannot_hold_stays_out():
    huge = np.finfo(np.float64).max
    for n_depth in T.N_DEPTHS:
        for c in T.hostile_line_lists(n_depth):
            assert not np.isnan(c.waals).any() and np.all(c.mass > 0), c.name
            for v in c.variants:
                for what, t in T.truth(c, v).items():
                    a = np.abs(t[np.isfinite(t) & (t != 0)])
                    if a.size:
                        assert a.max() <= 0.5 * huge, (c.name, v, what)
                        assert a.min() >= T.TINY or c.cls in SUBNORMAL_CLASSES, (c.name, v, what, float(a.min()))


@pytest.mark.parametrize("n_depth", T.N_DEPTHS)
def test_the_standing_tolerances_bound_the_bound(n_depth):
    c = T.case("well_conditioned", n_depth)
    v = c.variants[0]
    for what in TABLES:
        assert T.well_conditioned(c, v)[what].all(), what  # every amplification at most 1 at every point of the class
        rel = T.bound(c, v, what)
        ceiling = T.CEILING["alpha" if what == "alpha_short" else what]
        ops = T.n_ops(c, v)[what].max() * T.U
        print(f"{what:11s} bound {rel.max():.3e}  A x 2^-53 {ops:.3e}  ceiling {ceiling:g}")
        assert rel.max() <= ceiling and ops <= ceiling, (what, rel.max(), ops)
    assert set(np.unique(T.vald_vdw(c, c.temps, c.n_h)[2])) == {0, 3}  # the log form and ABO


def test_waals_branches_and_boundaries():
    c = T.case("waals")
    branch = T.vald_vdw(c, c.temps, c.n_h)[2]
    assert set(branch) == {0, 1, 2, 3}
    for triple in c.notes["boundaries"].values():
        for w in triple:
            assert np.count_nonzero((c.waals == w) & (np.signbit(c.waals) == np.signbit(w))) >= 2, w
    lo, on, hi = c.notes["boundaries"]["20"]
    assert np.nextafter(on, 0) == lo and np.nextafter(on, np.inf) == hi and on == T.VDW_ABO
    assert set(branch[c.waals == lo]) == {2} and set(branch[c.waals == on]) == {3} and set(branch[c.waals == hi]) == {3}
    lo, on, hi = c.notes["boundaries"]["0"]
    assert set(branch[c.waals == lo]) == {0} and set(branch[(c.waals == on) & ~np.signbit(c.waals)]) == {1}
    assert set(branch[np.signbit(c.waals) & (c.waals == 0)]) == {1}  # -0.0 takes the zero branch
    assert set(branch[c.waals == hi]) == {2}
    g = T.truth(c, c.variants[0])["gamma"]
    rest = T.truth(c, T.Variant(T.GAMMA_VALD, 11))["gamma"]  # without the van der Waals term
    assert np.all(g[c.waals == 0] == rest[c.waals == 0]) and np.all(g[c.waals == -330.0] == rest[c.waals == -330.0])  # the term is exactly zero
    term = T.vald_vdw(c, c.temps, c.n_h)[0]
    assert np.all(term[c.waals == -300.0] > 0) and np.all(term[c.waals == -330.0] == 0) and np.all(term[c.waals == 0] == 0)
    for w, alpha in ((21.0, 0.0), (20.0, 0.0)):
        assert np.all(c.waals[c.waals == w] - np.trunc(w) == alpha)
    assert 0 < 1 - (20.999 - 20) < 2e-3 and 0 < 1 - (899.9999 - 899) < 2e-4
    for w in T.WAALS_VALUES:
        assert np.any(c.waals == w)
    assert set(c.ion) == {1, 2}


def test_unsoeld_class():
    c = T.case("unsoeld")
    assert set(T.vald_vdw(c, c.temps, c.n_h)[2]) == {2} and set(c.ion) == {1, 2, 3, 26}
    assert np.all(np.isfinite(T.truth(c, c.variants[0])["gamma"]))


def test_stark_sign_test_branches():
    for n_depth in (3, 65):
        c = T.case("stark", n_depth)
        with np.errstate(all="ignore"):
            p = c.n_e[None, :] * c.stark[:, None]
        assert np.any(p < 0) and np.any(p > 0) and np.any((p == 0) & np.signbit(p)) and np.any((p == 0) & ~np.signbit(p))
        assert np.any(c.n_e == 0)
        under = (c.stark[:, None] == -5e-324) & (c.n_e[None, :] == 1e-300)  # the product underflows to -0.0: the term is dropped
        assert under.any() and np.all(p[under] == 0) and np.all(np.signbit(p[under]))
        kept = (c.stark[:, None] == -5e-324) & (c.n_e[None, :] >= 1.0)
        term, _ = T.vald_stark(c.n_e, c.stark, c.temps)
        assert kept.any() and np.all(term[under] == 0) and np.all(term[kept] > 0)
        assert np.all(term[c.stark == -400.0] == 0) and np.all(term[c.stark == 1.0] == 0)
        for s in T.STARK_VALUES:
            assert np.any((c.stark == s) & (np.signbit(c.stark) == np.signbit(s)))
    assert set(T.DEPTH_NE) <= set(T.case("stark", 65).n_e)


def test_linear_flags_class():
    c = T.case("linear_flags")
    assert {(v.mode, v.flags) for v in c.variants} == {(m, f) for m in (0, 1) for f in range(16)}
    assert set(c.z) == {1, 2}
    for v in c.variants:
        with_lin = T.truth(c, v)["gamma"]
        without = T.truth(c, v._replace(flags=v.flags & ~T.FLAG_LINEAR))["gamma"]
        changed = np.any(with_lin != without, axis=1)
        assert np.array_equal(changed, (c.z == 1) & bool(v.flags & T.FLAG_LINEAR)), v  # the term is hydrogen's alone, under its flag alone


def test_stark_switch_class():
    c = T.case("stark_switch")
    f_up, f_lo = (T.n_effective(c.ion, c.e_ion, e)[0] for e in (c.e_up, c.e_lo))
    d = f_up - f_lo
    assert len(c.notes["triples"]) >= 3 and len(c.notes["exact"]) >= 1
    for below, on, above in c.notes["triples"]:
        assert c.e_up[below] == np.nextafter(c.e_up[on], -np.inf) and c.e_up[above] == np.nextafter(c.e_up[on], np.inf)
        assert d[below] < T.STARK_SWITCH <= d[on] <= d[above]
    for k in c.notes["exact"]:
        assert d[c.notes["triples"][k][1]] == T.STARK_SWITCH  # ON the boundary: 1.5 is not < 1.5
    near = np.array(c.notes["near_degenerate"])
    assert np.all((d[near] > 0) & (d[near] < 1e-4 * f_lo[near]))
    inv = np.array(c.notes["inverted"])
    assert np.all(c.e_up[inv] < c.e_lo[inv])
    classic, lin_only = T.truth(c, T.Variant(T.GAMMA_CLASSIC))["gamma"], T.truth(c, T.Variant(T.GAMMA_CLASSIC, 1))["gamma"]
    assert np.all(np.isnan(classic[inv])) and np.all(np.isfinite(lin_only[inv])) and np.all(lin_only[inv] < 0)
    vald = T.truth(c, T.Variant(T.GAMMA_VALD))["gamma"]
    assert np.all(np.isnan(vald[inv[:2]])) and np.all(np.isfinite(vald[inv[2:]]))  # the Unsoeld width of an inverted pair; the log form
    rest = np.setdiff1d(np.arange(c.n_lines), inv)
    assert np.all(np.isfinite(classic[rest])) and np.all(classic[rest] > 0)


def test_ionisation_class():
    c = T.case("ionisation")
    f_up, f_lo = (T.n_effective(c.ion, c.e_ion, e)[0] for e in (c.e_up, c.e_lo))
    inf, nan = np.array(c.notes["inf"]), np.array(c.notes["nan"])
    assert np.all(np.isinf(f_up[inf]) | np.isinf(f_lo[inf])) and np.all(np.isnan(f_up[nan]) | np.isnan(f_lo[nan]))
    for base in (0, 6):
        assert np.isinf(f_up[base]) and np.isfinite(f_lo[base]) and np.isfinite(f_up[base + 1]) and np.isinf(f_lo[base + 1])
        assert np.isinf(f_up[base + 2]) and np.isinf(f_lo[base + 2])
        assert np.isnan(f_up[base + 3]) and np.isfinite(f_lo[base + 3]) and np.isfinite(f_up[base + 4]) and np.isnan(f_lo[base + 4])
        assert np.isnan(f_up[base + 5]) and np.isnan(f_lo[base + 5])
    for v in c.variants:
        g = T.truth(c, v)["gamma"]
        assert np.all(np.isnan(g[nan])), v
        assert np.all(np.isposinf(g[[0, 6]])) and not np.any(np.isfinite(g[[1, 7]])) and np.all(np.isnan(g[[2, 8]])), v  # (pow(-inf, 2/3) is +inf)


def test_modes_and_depth_states():
    c = T.case("modes_2_3", 64)
    assert {v.mode for v in c.variants} == {T.GAMMA_RADIATION_ONLY, T.GAMMA_ZERO}
    for v in c.variants:
        g = T.truth(c, v)["gamma"]
        assert g.shape == (c.n_lines, 1) and (np.all(g[:, 0] == c.a_ul) if v.mode == T.GAMMA_RADIATION_ONLY else not g.any())
    c = T.case("depth_states", 65)
    assert set(c.temps) == set(T.DEPTH_T) and set(c.n_e) == set(T.DEPTH_NE) and set(c.n_h) == set(T.DEPTH_NH)
    assert np.any(c.temps / 1e4 == 1.0)
    line = c.notes["overflow_line"]
    g = T.truth(c, T.Variant(T.GAMMA_VALD))["gamma"][line]
    assert np.all(np.isposinf(g[c.n_h == 1e300])) and np.all(np.isfinite(g[c.n_h < 1e300]))
    assert set(T.vald_vdw(c, c.temps, c.n_h)[2]) == {0, 2, 3} and np.any(c.z == 1)
    for n_depth in (1, 3):
        assert np.isfinite(T.case("depth_states", n_depth).temps).all()


def test_density_overflow_class():
    c = T.case("density_overflow", 65)
    assert {(bool(np.isinf(a)), bool(np.isinf(b))) for a, b in zip(c.n_e, c.n_h)} == {(False, False), (True, False), (False, True), (True, True)}
    other = c.z != 1
    lin_only = T.truth(c, T.Variant(T.GAMMA_VALD, 9))["gamma"]  # radiation and the linear Stark term: hydrogen's alone
    assert np.all(np.isfinite(lin_only[other])) and np.all(np.isposinf(lin_only[~other][:, np.isinf(c.n_e)]))
    g = T.truth(c, T.Variant(T.GAMMA_VALD))["gamma"]
    assert np.all(np.isnan(g[c.waals == 0][:, np.isinf(c.n_h)]))  # the reference's own 0 x inf (:1006)
    no_vdw = T.truth(c, T.Variant(T.GAMMA_VALD, 11))["gamma"]
    assert np.all(np.isfinite(no_vdw[c.stark > 0])) and np.all(np.isposinf(no_vdw[(c.stark < 0) & other][:, np.isinf(c.n_e)]))
    assert np.all(np.isposinf(no_vdw[c.stark == 0][:, np.isinf(c.n_e)]))  # inf x 0 >= 0 is false: the reference keeps the infinite width (:886)


def test_doppler_classes():
    c = T.case("doppler_xi", 65)
    assert [v.xi for v in c.variants] == list(T.XI_VALUES) and set(c.temps) == set(T.DEPTH_T)
    assert np.isclose(c.mass.min(), 1.008 * T.AMU_CGS) and np.isclose(c.mass.max(), 238.02891 * T.AMU_CGS)
    thermal = 2.0 * T.K_B_CGS * c.temps[None, :] / c.mass[:, None]
    assert np.all(1e12 ** 2 > 1e6 * thermal)  # xi^2 dominates
    for v in c.variants:
        dw = T.truth(c, v)["dw"]
        assert np.all(np.isposinf(dw)) if v.xi == 1e160 else np.all(np.isfinite(dw) & (dw > 0))
    c = T.case("doppler_packed", 64)
    assert c.n_lines == 64 and np.unique(c.temps).size >= 48 and np.unique(c.mass).size == 64 and c.notes["hit"] >= 48
    for a in (c.mass, 2.0 * T.K_B_CGS * c.temps):
        m = np.frexp(a)[0] * 2  # mantissa in [1, 2)
        assert np.count_nonzero(m - 1 < 2.0 ** -45) >= 12 and np.count_nonzero(2 - m < 2.0 ** -45) >= 12


def test_alpha_classes():
    c = T.case("alpha_exp")
    x = T.exp_argument(c.e_low_ev[:, None], c.temps[None, :])
    for (below, on, above), target in zip(c.notes["triples"], T.EXP_TARGETS):
        assert c.e_low_ev[below] == np.nextafter(c.e_low_ev[on], -np.inf) and c.e_low_ev[above] == np.nextafter(c.e_low_ev[on], np.inf)
        assert np.all(x[below] >= target) and np.all(x[on] < target) and np.all(x[above] < target)
    a = T.truth(c, c.variants[0])["alpha"]
    lower = x < 0
    assert np.all(a[lower & (x < T.EXP_ZERO_BELOW - 1e-9)] == 0) and np.all(a[lower & (x > T.EXP_ZERO_BELOW + 4)] > 0)  # (the coefficient, 0.027, on top)
    sub = lower & (x < T.EXP_SUBNORMAL_BELOW - 1e-6) & (x > T.EXP_ZERO_BELOW + 1e-9)
    assert sub.any() and np.all(a[sub] < T.TINY) and np.any(lower & (a >= T.TINY))
    assert np.any(lower & (x > T.EXP_LOW_CUT) & (x < T.EXP_ZERO_BELOW))  # zero by rounding, before exp_inline's cut
    upper = x[np.array(c.notes["upper"])]
    au = a[np.array(c.notes["upper"])]
    assert np.all(np.isposinf(au[upper > T.EXP_INF_ABOVE])) and np.all(np.isfinite(au[upper < T.EXP_INF_ABOVE]))
    assert np.any(upper > T.EXP_HIGH_CUT) and np.any((upper < T.EXP_HIGH_CUT) & (upper > T.EXP_INF_ABOVE)) and np.any(upper < T.EXP_INF_ABOVE)
    c = T.case("alpha_stim", 65)
    y = T.H_SI * c.nu[:, None] / (T.K_B_SI * c.temps[None, :])
    for target in T.STIM_TARGETS:
        assert np.any(np.abs(y / target - 1) < 1e-3), target
    assert set(c.pop_row) >= {0, c.pop.shape[0] - 1} and np.all(c.pop[0] == 0) and np.all((c.pop[1] > 0) & (c.pop[1] < T.TINY)) and np.all(c.pop[2] == 1e300)
    assert np.any(c.strength == 0) and np.any(np.signbit(c.e_low_ev) & (c.e_low_ev == 0)) and np.any(~np.signbit(c.e_low_ev) & (c.e_low_ev == 0))
    a = T.truth(c, c.variants[0])["alpha"]
    assert np.all(a[c.pop_row == 0] == 0) and np.all(a[c.strength == 0] == 0) and np.all(np.isfinite(a))


def test_restated_constants_are_the_sources():
    with open(os.path.join(ROOT, "stardis_amd", "csrc", "sdx_broadening.h")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "stardis_amd", "csrc", "sdx_kernels.h")) as f:
        kernels = f.read()
    a1 = re.findall(r"\(sub_rn\(nu_, nl_\) < ([0-9.]+)\) \? ([0-9.]+) : 1\.0", src)
    assert a1 == [("1.5", "0.642")] * 2 and (float(a1[0][0]), float(a1[0][1])) == (T.STARK_SWITCH, T.A1_CLOSE)  # the direct form and gen_line
    assert len(re.findall(r"else if \(vdw < 20\)", src)) == 2 and "vdw > 0.0 && vdw < 20" in src and "else if (vdw >= 20)" in src and T.VDW_ABO == 20
    assert len(re.findall(r"if \(vdw < 0\)", src)) == 3 and len(re.findall(r"else if \(vdw == 0\.0\)", src)) == 2
    cut = re.search(r"return x < (-[0-9.]+) \? 0\.0 : \(x > ([0-9.]+) \? INFINITY : r\);", src)
    assert (float(cut.group(1)), float(cut.group(2))) == (T.EXP_LOW_CUT, T.EXP_HIGH_CUT)
    ln = re.search(r"constexpr double kLn1e6 = (0x[0-9a-fp.+]+);", src).group(1)
    assert float.fromhex(ln) == T.LN_1E6 == np.log(1e6)
    assert "// 1 linear Stark, 2 quadratic Stark, 4 van der Waals, 8 radiation" in src
    assert (T.FLAG_LINEAR, T.FLAG_QUADRATIC, T.FLAG_VDW, T.FLAG_RADIATION) == (1, 2, 4, 8)
    for bit in (1, 2, 4, 8):
        assert f"p.flags & {bit}" in src and f"flags & {bit}" in kernels
    assert f"(flags & {T.FLAG_NO_HALVING}) ? g : g / 2" in kernels
    assert len(re.findall(r"mul_rn\(ne, stark\) >= 0|mul_rn\(D\.ne, L\.stark\) >= 0", src)) == 2
    assert "// 0 calc_gamma, 1 calc_vald_gamma, 2 A_ul only (molecules, one column), 3 zero" in src
    assert (T.GAMMA_CLASSIC, T.GAMMA_VALD, T.GAMMA_RADIATION_ONLY, T.GAMMA_ZERO) == (0, 1, 2, 3)
    from stardis_amd import constants as K

    for name in ("H_CGS", "C_CGS", "K_B_CGS", "M_P_CGS", "AMU_CGS", "E_ESU", "BOHR_RADIUS", "RYDBERG_ENERGY", "PI", "ALPHA_COEFFICIENT"):
        assert getattr(T, name) == getattr(K, name), name
    consts = dict(re.findall(r"constexpr double (kKBsi|kHsi|kEvJ) = ([0-9.e+-]+);", src))
    assert (float(consts["kKBsi"]), float(consts["kHsi"]), float(consts["kEvJ"])) == (T.K_B_SI, T.H_SI, T.EV_J)
    assert T.EXP_ZERO_BELOW == float(np.log(np.longdouble(2.0) ** -1075)) and T.EXP_INF_ABOVE == float(np.log(np.longdouble(2.0) ** 1024))
    assert T.EXP_SUBNORMAL_BELOW == float(np.log(np.longdouble(2.0) ** -1022))


def test_route_c_takes_the_classes_it_can():
    """finite, dw > 0, gamma >= 0, alpha >= 0: decided from the truth, at every depth count"""
    for cls in T.CLASSES:
        takes = [any(T.case(cls, nd).on_grid(v) for v in T.case(cls, nd).variants) for nd in T.N_DEPTHS]
        assert all(takes) == (cls in T.GRID_CLASSES), (cls, takes)
    for nd in T.N_DEPTHS:
        c = T.combined(nd)
        assert 150 <= c.n_lines <= 250 and np.all(np.diff(c.nu) >= 0) and all(c.on_grid(v) for v in c.variants)
        for k in T.BLOCK_LINE_COUNTS:
            part = T.combined(nd, k)
            assert part.n_lines == k and np.array_equal(part.nu, c.nu[:k]) and all(part.on_grid(v) for v in part.variants)
            for v in part.variants:  # the same lines give the same truth
                assert np.array_equal(T.truth(part, v)["gamma"], T.truth(c, v)["gamma"][:k])
    assert {16, 32, 48} < {k + d for k in T.BLOCK_LINE_COUNTS for d in (-1, 0, 1)}
