"""The line parameters (gamma, Doppler width, alpha_line per line and depth) on hostile line lists, judged against an
extended-precision evaluation of the reference's own formulas.

truth() walks what the reference tabulates before its line sum: calc_doppler_width (opacities_solvers/broadening.py:32-66),
calc_n_effective (:114-137), the three classic widths (:193-229, :281-343, :420-473) and their sum calc_gamma (:550-656), the VALD
widths (:880-1006) and their sum calc_vald_gamma (:1009-1085), and alpha_line of a VALD list (plasma/base.py:243-289).  Every DECISION is
taken in fp64 exactly as the reference takes it — vdW < 0, == 0, < 20, >= 20; int(vdW) and vdW - int(vdW); n_e stark >= 0; atomic_number
== 1; n_up - n_lo < 1.5 on the fp64 effective quantum numbers (IEEE subtract, divide, square root and multiply: the same bits on any
IEEE machine); whether an fp64 value has left the fp64 range (it is infinity from that step on, and zero below half the smallest
subnormal) — and every ARITHMETIC step in numpy longdouble in the reference's order.  Gamma((4 - alpha) / 2) of the ABO width comes
from mpmath at 30 digits (numpy has no long-double gamma).

hostile_line_lists() builds the classes; each sits on one decision of stardis_amd/csrc/sdx_broadening.h.  A boundary that depends on a
computed value (n_up - n_lo = 1.5; the argument of an exponential at one of exp_inline's cuts) is dialled by bisecting the fp64 rule over
the fp64 inputs, and has three items: the first input on the far side, and the adjacent fp64 inputs either side of it.

A route is held to bound(): FACTOR times the fp64 oracle's own distance from the truth plus A 2^-53 |truth|, point by point.  A counts
the rounded operations on the value's chain (n_ops(), beside the kernel lines it counts), each weighted by its amplification onto the
output, evaluated in longdouble from the truth's own intermediates: the exponent for a power, |x| for a rounding in the argument of
exp(x), e^-x / (1 - e^-x) for the stimulated-emission factor, (a + b) / |a - b| for the three differences of squares, 1 elsewhere (every
other sum is of non-negative terms; gamma's own sum weighs each term by its share, so it holds for a negative term too).  A library call
counts LIB roundings: 1 for exp (tests/test_gpu_linelist.py: "two exp() of <= 1 ulp each"), and LIB = 16 for pow, log and tgamma — no
table of the device library's bounds ships with the toolchain, so this is the figure tests/macroturbulence_reference.py already assumes
for the device's erfc and exp; ASSUMED, not measured (scripts/line_params_truth_table.py records the distances it could be tightened
from).  Where the truth is exactly 0, an infinity or NaN, so is the route (-0.0 and +0.0 count as equal); where |truth| is below the
smallest normal the comparison is absolute: 2 x 2^-1074 plus FACTOR oracle distances.

The standing tolerances bound this bound: on a value whose chain has no amplification above 1 (well_conditioned()) the allowance is at
most CEILING — 1e-13 on gamma, 1e-15 on the Doppler width, 3e-15 on alpha, what test_broadening_golden and tests/test_gpu_linelist.py
allow against the oracle.  A 2^-53 alone is below the ceiling there (the CPU test asserts it), so the cap trims only the FACTOR term:
the oracle's Doppler width is up to 2.9 x 2^-53 from the truth, and four times that plus A = 4.5 would be 1.8e-15.

Left out by construction (tests/test_line_params_truth_cpu.py checks that they stay out): a product that underflows into the subnormals
from normal factors (other than the exponential classes, judged absolutely), a value within a rounding of the end of the fp64 range, a
NaN vdW (the reference's astype(int) of it is undefined), mass <= 0 (LineList refuses it).

Used by tests/test_line_params_truth_cpu.py, tests/test_gpu_line_params_truth.py and scripts/line_params_truth_table.py.
"""
from collections import namedtuple

import numpy as np

L = np.longdouble
EXTENDED = bool(np.finfo(L).eps <= 1e-18)  # a host without an extended long double has no truth to offer: the GPU tests skip

FACTOR = 4.0  # tests/formal_solution_truth.py FACTOR
U = 2.0 ** -53
LIB = 16  # pow, log, tgamma of the device library: assumed (docstring)
LIB_SOURCE = "assumed: tests/macroturbulence_reference.py's 16 ulp for device library calls; no table of bounds under the toolchain"
EXP_LIB = 1  # exp, exp_inline: tests/test_gpu_linelist.py

# the standing tolerances a bound on well-conditioned values may not exceed (test_broadening_golden, tests/test_gpu_linelist.py)
CEILING = dict(gamma=1e-13, dw=1e-15, alpha=3e-15)

# stardis_amd/constants.py, restated as the reference evaluates them (broadening.py:16-26, plasma/base.py:35)
H_CGS, C_CGS, K_B_CGS = 6.62607015e-27, 29979245800.0, 1.380649e-16
M_P_CGS, AMU_CGS = 1.67262192369e-24, 1.6605390666e-24
E_ESU, BOHR_RADIUS, RYDBERG_ENERGY = 4.803204712570263e-10, 5.2917721090299995e-09, 2.1798723611035848e-11
PI = 3.141592653589793
EPS0 = 1.0 / (4.0 * PI)
ALPHA_COEFFICIENT = 0.026540088545744744
K_B_SI, H_SI, EV_J = 1.380649e-23, 6.62607015e-34, 1.602176634e-19

# the decisions of sdx_broadening.h, restated (the CPU test holds them to the source text)
STARK_SWITCH, A1_CLOSE = 1.5, 0.642
VDW_ABO = 20.0
EXP_LOW_CUT, EXP_HIGH_CUT = -745.2, 709.8
LN_1E6 = float.fromhex("0x1.ba18a998fffa0p+3")
FLAG_LINEAR, FLAG_QUADRATIC, FLAG_VDW, FLAG_RADIATION, FLAG_NO_HALVING = 1, 2, 4, 8, 16
EXP_ZERO_BELOW = -745.1332191019412  # log(2^-1075): below it exp rounds to zero in fp64
EXP_SUBNORMAL_BELOW = -708.3964185322641  # log(2^-1022)
EXP_INF_ABOVE = 709.782712893384  # log(2^1024)

TINY = float(np.finfo(np.float64).tiny)
SUBNORMAL = 2.0 ** -1074

D = 2.0 ** 30  # tests/line_opacity_truth.py: grid spacing [Hz] and first grid frequency K0 D
K0 = 600000
N_GRID = 384

GAMMA_CLASSIC, GAMMA_VALD, GAMMA_RADIATION_ONLY, GAMMA_ZERO = range(4)

Variant = namedtuple("Variant", "mode flags xi halve", defaults=(GAMMA_VALD, 15, 1.0e5, True))


def grid(n=N_GRID):
    """descending, exact: nus[i] = (K0 - i) 2^30 Hz"""
    return (K0 - np.arange(n, dtype=np.float64)) * D


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def first_true(pred, lo, hi):
    """the smallest fp64 x in (lo, hi] with pred(x), for a predicate that is monotone (false at lo, true at hi) over the positive
    doubles: bisection on the integer that an fp64 of one sign is"""
    a, b = (int(np.float64(v).view(np.int64)) for v in (lo, hi))
    assert 0 < a < b and not pred(lo) and pred(hi), (lo, hi)
    while b - a > 1:
        m = (a + b) // 2
        if pred(float(np.int64(m).view(np.float64))):
            b = m
        else:
            a = m
    return float(np.int64(b).view(np.float64))


# ---- the truth -------------------------------------------------------------------------------------------------------------------
_F64_END = L(2.0) ** 1024 * (L(1) - L(2.0) ** -54)  # from here on fp64 rounds to infinity
_F64_ZERO = L(2.0) ** -1075  # up to here fp64 rounds to zero


def _r(x):
    """an fp64 value that has left the fp64 range is infinity (or zero) from that step on"""
    x = np.asarray(x, dtype=L)
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        x = np.where(ax >= _F64_END, np.copysign(L(np.inf), x), x)
        x = np.where(ax <= _F64_ZERO, np.copysign(L(0), x), x)
    return x


def _lgamma_function(x):
    """Gamma(x) of longdouble x through mpmath at 30 digits"""
    import mpmath

    out = np.empty(x.shape, dtype=L)
    with mpmath.workdps(30):
        for i, v in np.ndenumerate(x):
            hi = float(v)
            g = mpmath.gamma(mpmath.mpf(hi) + mpmath.mpf(float(v - L(hi))))
            ghi = float(g)
            out[i] = L(ghi) + L(float(g - mpmath.mpf(ghi)))
    return out


def n_effective(ion, e_ion, e_lev):
    """:137 -> (fp64 value, for the decisions; longdouble value; roundings of the fp64 chain: sub_rn, /, sqrt halves the two, mul_rn)"""
    with np.errstate(all="ignore"):
        f = np.sqrt(RYDBERG_ENERGY / (e_ion - e_lev)) * ion
        v = np.sqrt(L(RYDBERG_ENERGY) / (e_ion.astype(L) - e_lev.astype(L))) * ion.astype(L)
    return f, v, 0.5 * 2 + 1 + 1


def _pow(x, e):
    """x ** e, e an fp64 constant of the reference; a negative base is NaN as in C's pow for a non-integer exponent"""
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x, dtype=L), L(e))


def _diff_of_squares(a, b):
    """-> (a - b, (a + b) / |a - b|) for a, b the two squares (non-negative)"""
    with np.errstate(all="ignore"):
        d = a - b
        return d, (a + b) / np.abs(d)


class _Sum:
    """gamma's sum: g = g + t in fp64 range, the budget sum A_t |t| and one rounding per add of two non-zero operands"""

    def __init__(self, shape):
        self.g, self.e, self.adds = np.zeros(shape, dtype=L), np.zeros(shape, dtype=L), np.zeros(shape)

    def add(self, t, a):
        with np.errstate(all="ignore"):
            t = np.broadcast_to(np.asarray(t, dtype=L), self.g.shape)
            self.adds = self.adds + ((self.g != 0) & (t != 0))
            self.g = _r(self.g + t)
            self.e = self.e + np.where(np.isfinite(t) & (t != 0), np.broadcast_to(a, t.shape) * np.abs(t), 0)

    def result(self, scale=1.0):
        with np.errstate(all="ignore"):
            a = self.e / np.abs(self.g) + self.adds
        return _r(self.g * L(scale)), np.where(np.isfinite(a), a, 0.0).astype(np.float64)


def linear_stark(nf_up, nf_lo, n_up, n_lo, a_n, ne):
    """:193-229 (gamma_linear_stark; gen_line's L.lin times gen_depth's D.ne23) -> (term (N_l, N_d), A)"""
    with np.errstate(all="ignore"):
        a1 = np.where(nf_up - nf_lo < STARK_SWITCH, A1_CLOSE, 1.0)  # the decision, in fp64
        sq, amp = _diff_of_squares(n_up * n_up, n_lo * n_lo)
        lin = L(0.60) * a1.astype(L) * sq
        t = _r(lin[:, None] * _pow(ne, 2.0 / 3.0)[None, :])
    # n_ops: 0.60 a1 (1); the squares (2 a_n + 1 each) through the difference (amp) and its rounding (1); pow (LIB); two products (2)
    a = 1 + amp * (2 * a_n + 1) + 1 + LIB + 2
    return t, a[:, None]


_C4_PRE_OPS = 4 + 6 + 1  # e e a0 a0 a0 (4), 36 h eps0 z z z z (6), the division


def quadratic_stark(ion, n_up, n_lo, a_n, ne, t):
    """:281-343 (gamma_quadratic_stark; L.c4p, D.qd, D.t16)"""
    with np.errstate(all="ignore"):
        zi = ion.astype(L)
        pre = (L(E_ESU) * L(E_ESU) * L(BOHR_RADIUS) * L(BOHR_RADIUS) * L(BOHR_RADIUS)) / (L(36.0) * L(H_CGS) * L(EPS0) * zi * zi * zi * zi)
        t1 = n_up * ((L(5.0) * n_up * n_up) + 1)
        t2 = n_lo * ((L(5.0) * n_lo * n_lo) + 1)
        d, amp = _diff_of_squares(t1 * t1, t2 * t2)
        c4 = pre * d
        out = _r(_r(L(1e19) * L(K_B_CGS) * ne.astype(L))[None, :] * _pow(c4, 2.0 / 3.0)[:, None]) * _pow(t, 1.0 / 6.0)[None, :]
    # n_ops: t1 = n (5 n n + 1): 3 a_n + 4; its square 6 a_n + 9, through the difference and its rounding; pre and the product; the power
    # takes 2/3 of that and LIB; 1e19 k (1) n_e (1) c4p (1); T ** (1/6) (LIB) and its product (1)
    a_c4 = amp * (6 * a_n + 9) + 1 + _C4_PRE_OPS + 1
    a = (2.0 / 3.0) * a_c4 + LIB + 3 + LIB + 1
    return _r(out), a[:, None]


def van_der_waals(ion, n_up, n_lo, a_n, t, nh):
    """:420-473 (gamma_van_der_waals; L.c6p, D.vw)"""
    with np.errstate(all="ignore"):
        u2, l2 = n_up * n_up, n_lo * n_lo
        d, amp = _diff_of_squares(L(5) * u2 * u2 + u2, L(5) * l2 * l2 + l2)
        c6 = L(6.46e-34) * d / (L(2) * ion.astype(L) * ion.astype(L))
        vw = L(17) * _pow(L(8) * L(K_B_CGS) * t.astype(L) / (L(PI) * L(M_P_CGS)), 0.3)
        out = _r(_r(vw[None, :] * _pow(c6, 0.4)[:, None]) * nh.astype(L)[None, :])
    # n_ops: n^2 (2 a_n + 1), n^4 as (n^2)^2 (4 a_n + 3), 5 x (1), + n^2 (1), through the difference and its rounding; 6.46e-34 x (1), / (1);
    # the power takes 0.4 of that and LIB; 8 k T / (pi m_p): 4, the power 0.3 of them and LIB, 17 x (1); two products
    a_c6 = amp * (4 * a_n + 5) + 1 + 2
    a = 0.4 * a_c6 + LIB + 0.3 * 4 + LIB + 1 + 2
    return out, a[:, None]


def vald_stark(ne, stark, t):
    """:880-890 (vald_stark; L.p10s, D.t16 and the sign test in gen_gamma)"""
    with np.errstate(all="ignore"):
        g = _r(_r(ne.astype(L)[None, :] * _r(L(10.0) ** stark.astype(L))[:, None]) * _pow(t.astype(L) / L(1e4), 1.0 / 6)[None, :])
        drop = ne[None, :] * stark[:, None] >= 0  # the decision, in fp64
    # n_ops: 10 ** stark (LIB), n_e x (1); T / 1e4 (1/6 of 1), its power (LIB), the product (1)
    return np.where(drop, L(0), g), np.full((stark.size, 1), LIB + 1 + 1.0 / 6 + LIB + 1)


def vald_vdw(c, t, nh):
    """:893-1006 (vald_vdw; gen_line's p10w / c6p / ab, oma, lmu and gen_gamma's four branches) -> (term, A, branch per line)"""
    vdw = c.waals
    nl, nd = vdw.size, t.size
    branch = np.where(vdw < 0, 0, np.where(vdw == 0.0, 1, np.where(vdw < VDW_ABO, 2, 3)))  # the decisions, in fp64
    g = np.zeros((nl, nd), dtype=L)
    a = np.zeros((nl, nd))
    tl = t.astype(L)
    with np.errstate(all="ignore"):
        m = branch == 0
        if m.any():  # :898: 10 ** vdW (LIB) x (T / 1e4) ** 0.38 (0.38 of 1, LIB), the product (1)
            g[m] = _r(_r(L(10.0) ** vdw[m].astype(L))[:, None] * _pow(tl / L(1e4), 0.38)[None, :])
            a[m] = LIB + 0.38 + LIB + 1
        m = branch == 2
        if m.any():  # :901-925: the classic width at n_H = 1 (exact), times the enhancement factor (1)
            ion = c.ion[m]
            _, n_up, a_n = n_effective(ion, c.e_ion[m], c.e_up[m])
            _, n_lo, _ = n_effective(ion, c.e_ion[m], c.e_lo[m])
            w, aw = van_der_waals(ion, n_up, n_lo, a_n, t, np.ones(nd))
            g[m] = _r(w * vdw[m].astype(L)[:, None])
            a[m] = aw - 1 + 1
        m = branch == 3
        if m.any():  # :928-948
            v = vdw[m]
            vi = np.trunc(v)  # astype(int)
            sigma = (vi.astype(L) * L(BOHR_RADIUS) * L(BOHR_RADIUS))[:, None]
            alpha = (v - vi).astype(L)[:, None]  # exact in fp64
            inv_mu = (L(1) / (L(1.008) * L(AMU_CGS)) + (L(1) / c.mass[m].astype(L)))[:, None]
            x = L(8) * L(K_B_CGS) * tl[None, :] / L(PI) * inv_mu
            vbar = np.sqrt(x)
            oma = L(1) - alpha
            g[m] = _r(L(2) * (L(4) / L(PI)) ** (alpha / 2) * _lgamma_function((L(4) - alpha) / 2) * L(1e6) * sigma * (vbar / L(1e6)) ** oma)
            # n_ops, the kernel's spelling (abo_speed_power): exp(oma (0.5 (lvb + lmu) - ln 1e6)).  lvb = log(8 k T / pi): 3 roundings in
            # its argument (absolute 3 on the logarithm) and LIB on |lvb|; lmu = log(1 / (1.008 amu) + 1 / m): 4 and LIB on |lmu|; their sum
            # (1 on |lvb + lmu|), halved; ln 1e6 rounded (1/2 on it), the difference (1 on it); all of it times |oma|; the product oma x
            # (1 on |exponent|); exp (EXP_LIB).  ab: 4 / pi (alpha / 2 of 1) and its power (LIB); 4 - alpha (1: x psi(x) < 1 on [1.5, 2]) and
            # tgamma (LIB); sigma (2); four products.  The last product with the speed power (1).
            lvb, lmu = np.log(L(8) * L(K_B_CGS) * tl / L(PI))[None, :], np.log(inv_mu)
            e = L(0.5) * (lvb + lmu) - L(LN_1E6)
            a_e = 0.5 * (3 + LIB * np.abs(lvb) + 4 + LIB * np.abs(lmu) + np.abs(lvb + lmu)) + 0.5 * LN_1E6 + np.abs(e)
            a_speed = np.abs(oma) * a_e + np.abs(oma * e) + EXP_LIB
            a_ab = 0.5 + LIB + 1 + LIB + 2 + 4
            a[m] = (a_ab + a_speed + 1).astype(np.float64)
        out = _r(g * nh.astype(L)[None, :])  # :1006 (1)
    return out, a + 1, branch


def gamma_truth(c, v):
    """-> (gamma, A): (N_l, N_d) longdouble and float64, (N_l, 1) for the modes with one column"""
    nl, nd = c.n_lines, c.n_depth
    if v.mode == GAMMA_RADIATION_ONLY:  # :799-801
        return c.a_ul.astype(L)[:, None], np.zeros((nl, 1))
    if v.mode == GAMMA_ZERO:
        return np.zeros((nl, 1), dtype=L), np.zeros((nl, 1))
    s = _Sum((nl, nd))
    is_h = c.z == 1  # the decision
    nf_up, n_up, a_n = n_effective(c.ion, c.e_ion, c.e_up)
    nf_lo, n_lo, _ = n_effective(c.ion, c.e_ion, c.e_lo)
    lin, a_lin = linear_stark(nf_up, nf_lo, n_up, n_lo, a_n, c.n_e)
    if v.mode == GAMMA_CLASSIC:  # :649-654, left to right (k_calc_gamma; gen_gamma's mode 0)
        if v.flags & FLAG_LINEAR:
            s.add(np.where(is_h[:, None], lin, L(0)), a_lin)
        if v.flags & FLAG_QUADRATIC:
            s.add(*quadratic_stark(c.ion, n_up, n_lo, a_n, c.n_e, c.temps))
        if v.flags & FLAG_VDW:
            s.add(*van_der_waals(c.ion, n_up, n_lo, a_n, c.temps, c.n_h))
        if v.flags & FLAG_RADIATION:
            s.add(c.a_ul.astype(L)[:, None], 0.0)
        return s.result()
    if v.flags & FLAG_RADIATION:  # :1043-1084 (k_calc_vald_gamma; gen_gamma's mode 1)
        s.add(c.a_ul.astype(L)[:, None], 0.0)
    if v.flags & FLAG_LINEAR:
        s.add(np.where(is_h[:, None], lin, L(0)), a_lin)
    if v.flags & FLAG_QUADRATIC:
        s.add(*vald_stark(c.n_e, c.stark, c.temps))
    if v.flags & FLAG_VDW:
        s.add(*vald_vdw(c, c.temps, c.n_h)[:2])
    return s.result(0.5 if v.halve else 1.0)  # :1084 (exact)


def doppler_truth(c, xi):
    """:57-66 (doppler_width; gen_doppler, whose 2 k T / m is the correctly rounded quotient) -> (dw, A)"""
    with np.errstate(all="ignore"):
        a = _r(L(2.0) * L(K_B_CGS) * c.temps.astype(L)[None, :] / c.mass.astype(L)[:, None])
        b = _r(L(xi) * L(xi))
        s = _r(a + b)
        dw = _r((c.nu.astype(L) / L(C_CGS))[:, None] * np.sqrt(s))
        share = np.where(np.isfinite(s) & (s > 0), a / s, 1.0)
    # n_ops: 2 k exact, x T (1), / m (1) on their share of the sum, xi xi (1) on its share, the sum (1); sqrt halves them (1); nu / c (1) and
    # the product (1)
    inside = np.maximum(2 * share, 1 - share) + 1
    return dw, (0.5 * inside + 1 + 2).astype(np.float64)


def alpha_truth(c, with_g_lo=True):
    """plasma/base.py:243-289 (gen_alpha) -> (alpha, A, x = -E / kT, y = -h nu / kT), all (N_l, N_d)"""
    with np.errstate(all="ignore"):
        tl = c.temps.astype(L)
        inv_kt = L(1) / (tl * L(K_B_SI))
        x = ((-c.e_low_ev.astype(L))[:, None] * inv_kt[None, :]) * L(EV_J)  # :243-247
        expo = _r(np.exp(x))
        n_lower = _r(expo * c.pop.astype(L)[c.pop_row])  # :256-259
        if with_g_lo:
            n_lower = _r(n_lower * c.g_lo.astype(L)[:, None])  # :260
        y = (L(-H_SI) / L(K_B_SI)) * (c.nu.astype(L)[:, None] * (L(1) / tl)[None, :])  # :271-280
        ey = np.exp(y)
        corr = L(1) - ey
        alpha = _r(_r(_r(L(c.alpha_coefficient) * n_lower) * c.strength.astype(L)[:, None]) * corr)  # :284-287
        stim = np.where(corr > 0, ey / corr, 0.0)
    # n_ops: T k (1), 1 / (1), -E x (1), x eV (1): four roundings in the argument of exp (|x| each) and exp (EXP_LIB); the population (1), g_lo
    # (1); h / k (1), 1 / T (1), nu x (1), the product (1): four in the argument of the second exp (|y| each) and exp, all through
    # e^y / (1 - e^y), and the difference (1); the coefficient, the strength and the correction (3)
    a = 4 * np.abs(x) + EXP_LIB + 1 + (1 if with_g_lo else 0) + (4 * np.abs(y) + EXP_LIB) * stim + 1 + 3
    return alpha, np.where(np.isfinite(a), a, 0.0).astype(np.float64), x, y


def well_conditioned(c, v):
    """-> dict like truth() of masks: the points on whose chain every amplification is at most 1 — no difference of squares in gamma
    (no linear Stark term of hydrogen, no classic quadratic Stark or van der Waals width, no Unsoeld width), |E / kT| <= 1 and
    e^-x / (1 - e^-x) <= 1 in alpha; the Doppler width has no amplification anywhere.  bound() is capped by CEILING there."""
    key = ("well", v)
    if key not in c._cache:
        nl, nd = c.n_lines, c.n_depth
        if v.mode >= GAMMA_RADIATION_ONLY:
            g = np.ones((nl, 1), dtype=bool)
        else:
            squares = ((v.flags & FLAG_LINEAR) != 0) & (c.z == 1)
            if v.mode == GAMMA_CLASSIC:
                squares = squares | bool(v.flags & (FLAG_QUADRATIC | FLAG_VDW))
            elif v.flags & FLAG_VDW:
                squares = squares | ((c.waals > 0) & (c.waals < VDW_ABO))
            g = np.repeat(~squares[:, None], nd, axis=1)
        _, _, x, y = alpha_truth(c, True)
        with np.errstate(all="ignore"):
            ey = np.exp(y)
            a = (np.abs(x) <= 1) & (ey <= (L(1) - ey))
        c._cache[key] = dict(gamma=g, dw=np.ones((nl, nd), dtype=bool), alpha=a, alpha_short=a)
    return c._cache[key]


def truth(c, v):
    """-> dict(gamma, dw, alpha, alpha_short) of longdouble tables for variant v of case c; alpha_short: g_lo null"""
    return {k: t for k, (t, _) in _walk(c, v).items()}


def n_ops(c, v):
    """-> dict like truth() of A, the weighted count of rounded operations on each value's chain (docstring)"""
    return {k: a for k, (_, a) in _walk(c, v).items()}


def _walk(c, v):
    key = ("walk", v)
    if key not in c._cache:
        dkey, akey = ("dw", v.xi), ("alpha",)
        if dkey not in c._cache:
            c._cache[dkey] = doppler_truth(c, v.xi)
        if akey not in c._cache:
            c._cache[akey] = (alpha_truth(c, True)[:2], alpha_truth(c, False)[:2])
        out = dict(gamma=gamma_truth(c, v), dw=c._cache[dkey], alpha=c._cache[akey][0], alpha_short=c._cache[akey][1])
        for t, a in out.values():
            t.setflags(write=False)
            a.setflags(write=False)
        c._cache[key] = out
    return c._cache[key]


def oracle_tables(c, v):
    """the fp64 oracle's tables -> dict like truth()"""
    import oracle

    key = ("oracle", v)
    if key not in c._cache:
        args = (c.z, c.ion, c.e_ion, c.e_up, c.e_lo, c.a_ul)
        with np.errstate(all="ignore"):
            if v.mode == GAMMA_VALD:
                g = oracle.calc_vald_gamma(*args, c.stark, c.waals, c.mass, c.n_e, c.temps, c.n_h, flags=v.flags | (0 if v.halve else FLAG_NO_HALVING))
            elif v.mode == GAMMA_CLASSIC:
                g = oracle.calc_gamma(*args, c.n_e, c.temps, c.n_h, flags=v.flags)
            else:  # (no arithmetic: the column of A_ul, or of zeros)
                g = (c.a_ul.copy() if v.mode == GAMMA_RADIATION_ONLY else np.zeros(c.n_lines))[:, None]
            dw = oracle.doppler_widths(c.nu, c.mass, c.temps, v.xi)
            al = [oracle.alpha_line_linelist(c.e_low_ev, g_lo, c.strength, c.nu, c.pop_row, c.pop, c.temps, c.alpha_coefficient) for g_lo in (c.g_lo, None)]
        out = dict(gamma=g, dw=dw, alpha=al[0], alpha_short=al[1])
        for t in out.values():
            t.setflags(write=False)
        c._cache[key] = out
    return c._cache[key]


# ---- the criterion ---------------------------------------------------------------------------------------------------------------
def same_special_values(got, ref):
    """zeros, NaNs and infinities (with their sign) at the same points; -0.0 and +0.0 count as equal"""
    got, ref = np.asarray(got), np.asarray(ref)
    return (np.array_equal(got == 0, ref == 0) and np.array_equal(np.isnan(got), np.isnan(ref))
            and np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)))


def distances(got, t):
    """-> (relative distance at the points where |t| is normal, absolute distance where it is subnormal, those two masks)"""
    got, t = np.asarray(got), np.asarray(t)
    at = np.abs(t)
    normal = np.isfinite(t) & (at >= TINY)
    sub = (at > 0) & (at < TINY)
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(L) - t)
        rel = np.where(normal, d / np.where(normal, at, 1), 0).astype(np.float64)
        ab = np.where(sub, d, 0).astype(np.float64)
    return rel, ab, normal, sub


RECORD = []  # what the GPU tests measured in this process: dicts, see judge(); scripts/line_params_truth_table.py writes them out


def _judge(tag, got, t, a, o, cap, ceiling, oracle_alone, record, fields):
    """the asserts of an fp64 table `got` against the truth t (A = a, the oracle's table o, the ceiling where `cap` holds): the zero /
    NaN / infinity pattern, then every other point within the bound -> the largest distance as a share of its allowance"""
    got = np.asarray(got)
    assert got.shape == t.shape and got.dtype == np.float64, (tag, got.shape, t.shape)
    odd = ((got == 0) != (t == 0)) | (np.isnan(got) != np.isnan(t)) | (np.isinf(got) != np.isinf(t))
    assert same_special_values(got, t), (tag, "zeros, NaNs or infinities differ from the truth", np.argwhere(odd)[:4].tolist())
    with np.errstate(all="ignore"):
        od = np.abs(o.astype(L) - t)
        od = np.where(np.isfinite(od), od, 0)
        at = np.abs(np.where(np.isfinite(t), t, 0))
        if oracle_alone:  # (a subnormal value carries the roundings of its chain too: the four in the argument of exp, |x| > 708 each)
            rel_ok = a * U * np.ones(t.shape)
            abs_ok = (2 * SUBNORMAL + rel_ok * at).astype(np.float64)
        else:
            rel_ok = np.where(at > 0, FACTOR * od / np.where(at > 0, at, 1) + a * U, 0).astype(np.float64)
            rel_ok = np.where(cap, np.minimum(rel_ok, ceiling), rel_ok)
            abs_ok = (2 * SUBNORMAL + FACTOR * od).astype(np.float64)
    rel, ab, normal, sub = distances(got, t)
    o_rel, o_ab, _, _ = distances(o, t)
    with np.errstate(all="ignore"):  # (an exact value, A = 0, at an exact distance of 0: no share)
        share = max(float(np.nanmax(rel[normal] / rel_ok[normal], initial=0.0)), float(np.max(ab[sub] / abs_ok[sub], initial=0.0)))
    if record is not None:
        record.append(dict(fields, kernel_ulp=float(rel.max(initial=0.0) / U), oracle_ulp=float(o_rel.max(initial=0.0) / U), share=share,
                           kernel_subnormal=float(ab.max(initial=0.0) / SUBNORMAL), oracle_subnormal=float(o_ab.max(initial=0.0) / SUBNORMAL),
                           largest_bound=float(rel_ok[normal].max(initial=0.0))))
    bad = (normal & (rel > rel_ok)) | (sub & (ab > abs_ok))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError((tag, "points outside the bound", int(bad.sum()), "first", i, "got", float(got[i]), "truth", float(t[i]), "distance",
                              float(rel[i] if normal[i] else ab[i]), "allowed", float(rel_ok[i] if normal[i] else abs_ok[i])))
    return share


def bound(c, v, what):
    """-> the relative allowance of every point where |truth| is normal: what a route's distance from the truth may be"""
    t, a, o = truth(c, v)[what], n_ops(c, v)[what], oracle_tables(c, v)[what]
    with np.errstate(all="ignore"):
        od = np.abs(o.astype(L) - t)
        rel = np.where(np.isfinite(t) & (t != 0), FACTOR * np.where(np.isfinite(od), od, 0) / np.abs(t) + a * U, 0).astype(np.float64)
    return np.where(well_conditioned(c, v)[what], np.minimum(rel, CEILING["alpha" if what == "alpha_short" else what]), rel)


def judge(c, v, what, got, route="", label="", record=RECORD, oracle_alone=False):
    """a route's table `what` of variant v of case c against truth() and bound() (oracle_alone: within A 2^-53, the FACTOR term being
    zero) -> the largest distance as a share of its allowance; one record per call"""
    fields = dict(route=route, label=label, what=what, cls=c.cls, case=c.name, variant=tuple(v), n_depth=c.n_depth)
    return _judge((c.name, tuple(v), route, label, what), got, truth(c, v)[what], n_ops(c, v)[what], oracle_tables(c, v)[what],
                  well_conditioned(c, v)[what], CEILING["alpha" if what == "alpha_short" else what], oracle_alone, record, fields)


TERMS = {"linear_stark": FLAG_LINEAR, "quadratic_stark": FLAG_QUADRATIC, "van_der_waals": FLAG_VDW}


def term_tables(c, term):
    """one classic width of EVERY line of case c (the linear Stark width too, whatever the atomic number), as the reference's element-wise
    functions give it from the fp64 effective quantum numbers -> (truth, A, oracle)"""
    import oracle

    key = ("term", term)
    if key not in c._cache:
        _, n_up, a_n = n_effective(c.ion, c.e_ion, c.e_up)
        _, n_lo, _ = n_effective(c.ion, c.e_ion, c.e_lo)
        if term == "linear_stark":
            nf_up, nf_lo = n_effective(c.ion, c.e_ion, c.e_up)[0], n_effective(c.ion, c.e_ion, c.e_lo)[0]
            t, a = linear_stark(nf_up, nf_lo, n_up, n_lo, a_n, c.n_e)
        elif term == "quadratic_stark":
            t, a = quadratic_stark(c.ion, n_up, n_lo, a_n, c.n_e, c.temps)
        else:
            t, a = van_der_waals(c.ion, n_up, n_lo, a_n, c.temps, c.n_h)
        with np.errstate(all="ignore"):  # (one term of calc_gamma's sum, the others exactly zero)
            o = oracle.calc_gamma(np.ones_like(c.z), c.ion, c.e_ion, c.e_up, c.e_lo, c.a_ul, c.n_e, c.temps, c.n_h, flags=TERMS[term])
        a = np.broadcast_to(np.where(np.isfinite(a), a, 0.0), t.shape).astype(np.float64)
        c._cache[key] = (t, a, o)
    return c._cache[key]


def judge_term(c, term, got, route="A", record=RECORD):
    t, a, o = term_tables(c, term)
    fields = dict(route=route, label=term, what="term", cls=c.cls, case=c.name, variant=(GAMMA_CLASSIC, TERMS[term], 0.0, True), n_depth=c.n_depth)
    return _judge((c.name, route, term), got, t, a, o, np.zeros(t.shape, dtype=bool), 0.0, False, record, fields)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
MASSES = {1: 1.008, 2: 4.0026, 6: 12.011, 12: 24.305, 20: 40.078, 26: 55.845, 56: 137.327, 92: 238.02891}  # H to U [amu]
EV = 1.602176634e-12


class Case:
    """one line list of a class with its per-depth state, in the layout stardis_amd.linelist.LineList takes it; `variants` the
    (gamma_mode, flags, microturbulence, halving) it is run with; notes: what the class claims, for the CPU test"""

    def __init__(self, cls, n_lines, n_depth, seed, variants=(Variant(),), name=None):
        self.cls, self.name, self.n_lines, self.n_depth = cls, name or cls, int(n_lines), int(n_depth)
        self.variants = tuple(variants)
        rng = self.rng = np.random.default_rng(seed)
        n, nd = self.n_lines, self.n_depth
        lo, hi = (K0 - N_GRID + 40) * D, (K0 - 40) * D
        self.nu = np.sort(rng.uniform(lo, hi, n))  # ascending, inside the exact grid
        self.z = rng.choice([6, 12, 20, 26], n).astype(np.int32)
        self.ion = rng.integers(1, 3, n).astype(np.int32)  # charge seen by the outer electron
        self.e_ion = np.where(self.ion == 1, 7.9, 16.2) * EV * (1 + 0.3 * rng.random(n))
        self.e_up = rng.uniform(0.5, 0.9, n) * self.e_ion
        self.e_lo = rng.uniform(0.1, 0.4, n) * self.e_ion
        self.a_ul = 10 ** rng.uniform(6, 9, n)
        self.stark = -rng.uniform(4.5, 6.5, n)
        self.waals = -rng.uniform(7, 8, n)
        self.set_masses()
        self.e_low_ev = rng.uniform(0.01, 0.1, n)
        self.g_lo = rng.integers(1, 11, n).astype(np.float64)
        self.strength = 10 ** rng.uniform(-6, 0.3, n) / self.g_lo
        self.pop_row = rng.integers(0, 3, n).astype(np.int32)
        self.temps = np.linspace(4000.0, 9000.0, nd) if nd > 1 else np.array([5777.0])
        self.n_e = 10 ** np.linspace(15, 12, nd)
        self.n_h = 10 ** np.linspace(17, 15, nd)
        self.pop = 10 ** rng.uniform(4, 12, (3, nd))
        self.alpha_coefficient = ALPHA_COEFFICIENT
        self.notes = {}
        self._cache = {}

    def set_masses(self):
        self.mass = np.array([MASSES[int(a)] for a in self.z]) * AMU_CGS

    def hydrogen(self, m, n_lo=2.0, n_up=3.0):
        """lines m become hydrogen lines between effective quantum numbers n_lo and n_up (n = sqrt(Ryd / (E_ion - E)))"""
        self.z[m], self.ion[m] = 1, 1
        self.e_ion[m] = 13.61 * EV  # (above the Rydberg energy: the ground level keeps a positive energy)
        self.e_up[m] = self.e_ion[m] - RYDBERG_ENERGY / np.asarray(n_up, dtype=np.float64) ** 2
        self.e_lo[m] = self.e_ion[m] - RYDBERG_ENERGY / np.asarray(n_lo, dtype=np.float64) ** 2
        self.set_masses()

    def depth_cycle(self, temps=None, n_e=None, n_h=None):
        """per-depth state from lists, every combination in turn (the first list fastest)"""
        lists = [np.atleast_1d(np.asarray(a, dtype=np.float64)) if a is not None else None for a in (temps, n_e, n_h)]
        k = np.arange(self.n_depth)
        for name, a in zip(("temps", "n_e", "n_h"), lists):
            if a is not None:
                setattr(self, name, a[k % a.size].copy())
                k = k // a.size
        return self

    def line_list(self, v, g_lo=True):
        from stardis_amd import linelist as LL

        return LL.LineList(self.nu, self.e_low_ev, self.strength, self.pop_row, self.pop, self.mass, self.temps, g_lo=self.g_lo if g_lo else None,
                           microturbulence=v.xi, gamma_mode=v.mode, flags=v.flags, atomic_number=self.z, ion_number=self.ion,
                           ionization_energy=self.e_ion, upper_energy=self.e_up, lower_energy=self.e_lo, A_ul=self.a_ul, stark=self.stark, waals=self.waals,
                           electron_density=self.n_e, h_density=self.n_h, alpha_coefficient=self.alpha_coefficient)

    def on_grid(self, v):
        """whether route C takes the case: every value of the three tables finite, dw > 0, gamma >= 0, alpha >= 0"""
        t = truth(self, v)
        return bool(all(np.all(np.isfinite(x)) for x in t.values()) and np.all(t["dw"] > 0) and np.all(t["gamma"] >= 0) and np.all(t["alpha"] >= 0))


BOTH = (Variant(GAMMA_CLASSIC), Variant(GAMMA_VALD))
WAALS_VALUES = (-0.0, 0.0, 5e-324, -5e-324, down(20.0), 20.0, up(20.0), 21.0, 20.999, 899.9999, -7.5, -300.0, -330.0, 350.25, down(21.0), 1.0, down(1.0))
STARK_VALUES = (-0.0, 0.0, 1.0, -5.0, -400.0, -5e-324, 5e-324)
DEPTH_T = (1000.0, 5777.0, 1e4, 1e5, 1e7)
DEPTH_NE = (0.0, 1e-300, 1.0, 1e14, 1e20)
DEPTH_NH = (0.0, 1e17, 1e300)
XI_VALUES = (0.0, 1e5, 1e12, 1e160)
STIM_TARGETS = (1e-12, 1e-3, 1.0, 40.0, 750.0)
EXP_TARGETS = (EXP_SUBNORMAL_BELOW, EXP_ZERO_BELOW, EXP_LOW_CUT)


def _well_conditioned(nd):
    """every amplification at most 1: no difference of squares (no hydrogen, no Unsoeld width), exponents |E / kT| < 0.3, h nu / kT > 3;
    the log-form and ABO van der Waals widths, the log-form Stark width.  The ceilings of the standing tolerances are asserted here."""
    c = Case("well_conditioned", 24, nd, 1)
    c.waals[::3] = c.rng.integers(150, 900, c.waals[::3].size) + c.rng.uniform(0.2, 0.35, c.waals[::3].size)
    return c


def _waals(nd):
    c = Case("waals", len(WAALS_VALUES) * 2, nd, 2)
    c.waals[:] = np.repeat(WAALS_VALUES, 2)
    c.ion[:] = np.tile([1, 2], len(WAALS_VALUES))
    c.notes["boundaries"] = {"0": (-5e-324, 0.0, 5e-324), "20": (down(20.0), 20.0, up(20.0))}
    return c


def _unsoeld(nd):
    """0 < vdW < 20: the enhancement factor on the classic width, with the charge the outer electron sees 1, 2, 3 and 26"""
    factors, charges = (0.5, 1.0, 2.5, 19.5), (1, 2, 3, 26)
    c = Case("unsoeld", 16, nd, 3)
    c.waals[:] = np.repeat(factors, 4)
    c.ion[:] = np.tile(charges, 4)
    c.e_ion[:] = 7.9 * EV * c.ion.astype(np.float64) ** 2 * (1 + 0.1 * c.rng.random(16))
    c.e_up, c.e_lo = c.rng.uniform(0.6, 0.9, 16) * c.e_ion, c.rng.uniform(0.1, 0.4, 16) * c.e_ion
    return c


def _stark(nd):
    c = Case("stark", len(STARK_VALUES) * 2, nd, 4)
    c.stark[:] = np.repeat(STARK_VALUES, 2)
    c.depth_cycle(n_e=DEPTH_NE)
    c.notes["boundaries"] = {"0": (-5e-324, 0.0, 5e-324)}
    return c


def _linear_flags(nd):
    """atomic number 1 and 2 under all 16 flag combinations in both modes that have a linear Stark term"""
    c = Case("linear_flags", 8, nd, 5, variants=[Variant(m, f) for m in (GAMMA_CLASSIC, GAMMA_VALD) for f in range(16)])
    c.hydrogen(np.arange(0, 8, 2), n_lo=[2.0, 2.0, 3.0, 1.0], n_up=[3.0, 5.0, 4.0, 2.0])
    c.z[1::2], c.ion[1::2] = 2, 1
    c.set_masses()
    c.waals[:4] = 350.25
    return c


def dial_stark_switch(c, l):
    """e_up of hydrogen line l so that n_up - n_lo >= 1.5 first holds in fp64 -> that e_up (the adjacent fp64 below is < 1.5)"""
    one = lambda a: np.array([a], dtype=np.float64)  # noqa: E731
    n_lo = n_effective(c.ion[l:l + 1], c.e_ion[l:l + 1], c.e_lo[l:l + 1])[0][0]
    pred = lambda e: bool(n_effective(c.ion[l:l + 1], c.e_ion[l:l + 1], one(e))[0][0] - n_lo >= STARK_SWITCH)  # noqa: E731
    return first_true(pred, float(c.e_lo[l]), float(c.e_ion[l] * (1 - 1e-6)))


def _stark_switch(nd):
    """hydrogen lines with n_up - n_lo on the switch of a1 and one fp64 step of e_up either side (three lower levels; notes["exact"]: the
    triples whose middle item has n_up - n_lo == 1.5 exactly), near-degenerate levels (n_up - n_lo of order 1e-6 n), and e_up < e_lo"""
    lows = np.concatenate([[1.0, 2.0, 3.0], 1.0 + 3.0 * np.random.default_rng(6).random(37)])
    n = 3 * lows.size + 6 + 4
    c = Case("stark_switch", n, nd, 6, variants=BOTH + (Variant(GAMMA_CLASSIC, 1), Variant(GAMMA_VALD, 1), Variant(GAMMA_CLASSIC, 7)))
    c.hydrogen(np.arange(n), n_lo=2.0, n_up=3.0)
    triples, exact = [], []
    for k, n_lo in enumerate(lows):
        i = 3 * k
        c.hydrogen(np.arange(i, i + 3), n_lo=n_lo, n_up=n_lo + 2)
        e = dial_stark_switch(c, i)
        c.e_up[i:i + 3] = down(e), e, up(e)
        triples.append((i, i + 1, i + 2))
        f = n_effective(c.ion[i + 1:i + 2], c.e_ion[i + 1:i + 2], c.e_up[i + 1:i + 2])[0] - n_effective(c.ion[i + 1:i + 2], c.e_ion[i + 1:i + 2], c.e_lo[i + 1:i + 2])[0]
        if f[0] == STARK_SWITCH:
            exact.append(k)
    i = 3 * lows.size
    for k, (n_lo, rel) in enumerate(((2.0, 1e-6), (3.0, 3e-6), (10.0, 1e-6), (2.0, 1e-9), (30.0, 1e-6), (1.0, 1e-6))):
        c.hydrogen(np.arange(i + k, i + k + 1), n_lo=n_lo, n_up=n_lo * (1 + rel))
    c.notes["near_degenerate"] = tuple(range(i, i + 6))
    i += 6
    c.hydrogen(np.arange(i, i + 4), n_lo=[3.0, 5.0, 2.5, 4.0], n_up=[2.0, 2.0, 2.0, 3.9])
    c.notes["inverted"] = tuple(range(i, i + 4))
    c.waals[i:i + 2] = 5.0  # the Unsoeld width of an inverted pair: c6 < 0
    c.notes["triples"], c.notes["exact"] = tuple(triples), tuple(exact)
    return c


def _ionisation(nd):
    """a level AT the ionisation energy (n_eff infinite) and ABOVE it (NaN): upper, lower, both; hydrogen and iron, the latter with an
    Unsoeld width so that the VALD mode reads n_eff too"""
    c = Case("ionisation", 12, nd, 7, variants=BOTH)
    c.hydrogen(np.arange(6))
    c.ion[6:] = 1
    c.e_ion[6:] = 7.9 * EV
    c.e_up[6:], c.e_lo[6:] = 0.8 * c.e_ion[6:], 0.3 * c.e_ion[6:]
    c.waals[6:] = 5.0
    for base in (0, 6):
        ei = c.e_ion[base]
        c.e_up[base + 0] = ei
        c.e_lo[base + 1] = ei
        c.e_up[base + 2] = c.e_lo[base + 2] = ei
        c.e_up[base + 3] = 1.1 * ei
        c.e_lo[base + 4] = 1.1 * ei
        c.e_up[base + 5] = c.e_lo[base + 5] = 1.2 * ei
    c.notes["inf"] = (0, 1, 2, 6, 7, 8)
    c.notes["nan"] = (3, 4, 5, 9, 10, 11)
    return c


def _modes(nd):
    c = Case("modes_2_3", 19, nd, 8, variants=(Variant(GAMMA_RADIATION_ONLY), Variant(GAMMA_ZERO), Variant(GAMMA_RADIATION_ONLY, 0)))
    c.a_ul[:3] = 0.0, 5e-324, 1e300
    return c


def _depth_states(nd):
    """T in DEPTH_T, n_e in DEPTH_NE and n_H in DEPTH_NH, every combination in turn, on hydrogen, log-form, Unsoeld and ABO lines; one line whose
    van der Waals width leaves the fp64 range at n_H = 1e300"""
    c = Case("depth_states", 18, nd, 9, variants=BOTH)
    c.depth_cycle(DEPTH_T, DEPTH_NE, DEPTH_NH)
    if nd >= 3:
        c.temps[:3], c.n_e[:3], c.n_h[:3] = (1e4, 1e7, 1000.0), (1e20, 0.0, 1e-300), (1e300, 0.0, 1e300)
    c.hydrogen(np.arange(0, 4), n_lo=[1.0, 2.0, 2.0, 3.0], n_up=[2.0, 3.0, 4.0, 4.0])
    c.waals[4:8] = 350.25, 899.3, 21.0, 20.0
    c.waals[8:10] = 2.5
    c.waals[11] = 9e18  # an ABO cross-section of 9e18 a0^2 (int64 holds it): the width is beyond the fp64 range at n_H = 1e300
    c.notes["overflow_line"] = 11
    return c


def _density_overflow(nd):
    """n_e and n_H beyond the fp64 range (infinite), alone and together: every width that holds the density is infinite, a width that
    is exactly zero (vdW = 0, stark >= 0) times it NaN, and a line without a term keeps a finite gamma — a term that is not the line's
    own must not be formed from a zero factor and the density"""
    c = Case("density_overflow", 8, nd, 14, variants=BOTH + (Variant(GAMMA_VALD, 9), Variant(GAMMA_VALD, 11), Variant(GAMMA_CLASSIC, 9)))
    c.hydrogen(np.arange(0, 2))
    c.waals[2:] = -7.5, 350.25, 0.0, 2.5, -7.5, 350.25
    c.stark[6:] = 0.0, 1.0
    c.depth_cycle(n_e=[1e14, np.inf], n_h=[1e17, np.inf])
    return c


def _doppler_xi(nd):
    """microturbulence 0, 1e5, 1e12 (xi^2 dominates) and 1e160 (xi^2 overflows); masses from H to U; the temperatures of DEPTH_T"""
    zs = sorted(MASSES)
    c = Case("doppler_xi", 2 * len(zs), nd, 10, variants=[Variant(GAMMA_ZERO, 15, xi) for xi in XI_VALUES])
    c.z[:] = np.tile(zs, 2)
    c.set_masses()
    c.depth_cycle(DEPTH_T)
    return c


def packed_mantissas(n=64):
    """n mantissas in [1, 2): packed against 1 from above, against 2 from below, and a few in between"""
    q = n // 4
    k = np.arange(q, dtype=np.float64)
    return np.concatenate([1.0 + k * 2.0 ** -52, 2.0 - (k + 1) * 2.0 ** -52, 1.0 + (2 * k + 1) * 2.0 ** -30, 1.5 + (k - q // 2) * 2.0 ** -52])


def _doppler_packed(nd):
    """64 masses x 64 values of 2 k T with mantissas packed against 1 and 2: gen_doppler's reciprocal and two FMAs against the division.
    T is chosen so that 2 k T, as the kernels round it, IS the packed value wherever an fp64 T gives it (notes["hit"] counts them)."""
    c = Case("doppler_packed", 64, nd, 11, variants=(Variant(GAMMA_ZERO, 15, 0.0),))
    c.mass = packed_mantissas() * 2.0 ** -77  # 6.6e-24 to 1.3e-23 g
    want = packed_mantissas() * 2.0 ** -40  # 2 k T, T from 3300 K to 6600 K
    t = want / (2.0 * K_B_CGS)
    for k in range(64):  # the fp64 T whose product is nearest the wanted mantissa
        cand = np.array([down(down(t[k])), down(t[k]), t[k], up(t[k]), up(up(t[k]))])
        t[k] = cand[np.argmin(np.abs(2.0 * K_B_CGS * cand - want[k]))]
    c.notes["hit"] = int(np.count_nonzero(2.0 * K_B_CGS * t == want))
    c.temps = t[np.arange(nd) % 64].copy()
    return c


def exp_argument(e_low_ev, t):
    """the argument gen_alpha hands exp_inline, in fp64: ((-E) (1 / (T k))) eV"""
    return ((-e_low_ev) * (1.0 / (t * K_B_SI))) * EV_J


def dial_exp_argument(target, t):
    """-> the smallest fp64 e_low [eV] whose fp64 exponent argument at temperature t is below `target` (< 0)"""
    guess = -target * t * K_B_SI / EV_J
    return first_true(lambda e: bool(exp_argument(e, t) < target), guess * (1 - 1e-9), guess * (1 + 1e-9))


def _alpha_exp(nd):
    """-E / kT on either side of -708.4 (the result turns subnormal), -745.13 (it rounds to zero) and -745.2 (exp_inline's cut): the
    first fp64 e_low beyond each and its neighbours, and arguments a thousandth away; population, weight and strength 1 (the products
    keep the subnormal's absolute error); all depths at one temperature.  And the upper end: negative e_low around 709.78 and 709.8."""
    t = 5777.0
    vals = []
    for target in EXP_TARGETS:
        e = dial_exp_argument(target, t)
        vals += [down(e), e, up(e), e * (1 - 1e-3), e * (1 + 1e-3)]
    vals += [0.5 * (vals[5] + vals[10]), 0.9 * vals[0], 0.5 * (vals[0] + vals[5])]
    hi = [-EXP_INF_ABOVE * t * K_B_SI / EV_J * f for f in (0.998, 1 + 1e-6, 1 + 1e-4)] + [-EXP_HIGH_CUT * t * K_B_SI / EV_J * f for f in (1 - 1e-9, 1 + 1e-9)]
    c = Case("alpha_exp", len(vals) + len(hi), nd, 12, variants=(Variant(GAMMA_ZERO),))
    c.temps[:] = t
    c.e_low_ev[:] = vals + hi
    c.g_lo[:], c.strength[:], c.pop[:] = 1.0, 1.0, 1.0
    c.pop_row[:] = 0
    c.strength[len(vals):] = 1e-300  # (the upper end: finite below the overflow)
    c.notes["triples"] = ((0, 1, 2), (5, 6, 7), (10, 11, 12))
    c.notes["upper"] = tuple(range(len(vals), len(vals) + len(hi)))
    return c


def _alpha_stim(nd):
    """h nu / kT of 1e-12 (1 - exp cancels), 1e-3, 1, 40 and 750 (exp underflows) by the temperature; populations 0, subnormal and 1e300;
    strength 0; the first and the last population row; e_low 0 and -0.0"""
    c = Case("alpha_stim", 16, nd, 13, variants=(Variant(GAMMA_ZERO),))
    nu0 = K0 * D
    c.depth_cycle(temps=[H_SI * nu0 / (K_B_SI * x) for x in STIM_TARGETS])
    c.pop = np.ones((4, nd))
    c.pop[0], c.pop[1], c.pop[2], c.pop[3] = 0.0, 1e-310, 1e300, 10 ** np.linspace(12, 4, nd)
    c.pop_row[:] = np.tile([0, 1, 2, 3], 4)
    c.e_low_ev[:8] = np.repeat([0.0, -0.0], 4)
    c.e_low_ev[8:] = 0.0
    c.g_lo[:8], c.strength[:8] = 1.0, 1.0
    c.strength[8:12] = 0.0
    c.notes["rows"] = (0, 3)
    return c


_BUILDERS = {"well_conditioned": _well_conditioned, "waals": _waals, "unsoeld": _unsoeld, "stark": _stark, "linear_flags": _linear_flags,
             "stark_switch": _stark_switch, "ionisation": _ionisation, "modes_2_3": _modes, "depth_states": _depth_states, "density_overflow": _density_overflow, "doppler_xi": _doppler_xi,
             "doppler_packed": _doppler_packed, "alpha_exp": _alpha_exp, "alpha_stim": _alpha_stim}
CLASSES = tuple(_BUILDERS)
N_DEPTHS = (1, 3, 64, 65)  # one pre-pass depth block, ragged, full, and two
_cases = {}


def case(cls, n_depth=3):
    """the Case of a class at a depth count, cached for the life of the process"""
    if (cls, n_depth) not in _cases:
        c = _BUILDERS[cls](n_depth)
        c.name = f"{cls}_{n_depth}"
        for k, a in vars(c).items():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cases[(cls, n_depth)] = c
    return _cases[(cls, n_depth)]


PER_LINE = ("nu", "z", "ion", "e_ion", "e_up", "e_lo", "a_ul", "stark", "waals", "mass", "e_low_ev", "g_lo", "strength", "pop_row")
# route C: the classes with a variant whose three tables are finite, dw > 0, gamma >= 0, alpha >= 0 at every depth count (the CPU test
# holds the list to Case.on_grid)
GRID_CLASSES = ("well_conditioned", "waals", "unsoeld", "stark", "linear_flags", "modes_2_3", "depth_states", "doppler_xi", "doppler_packed", "alpha_stim")
COMBINED = ("well_conditioned", "waals", "unsoeld", "linear_flags", "stark", "modes_2_3", "doppler_xi", "doppler_packed")
BLOCK_LINE_COUNTS = (15, 16, 17, 31, 32, 33, 47, 48, 49)  # both sides of the pre-pass's 16 and 32 lines per block, and of 48


def combined(n_depth, n_lines=None):
    """the lines of the COMBINED classes as one ascending list under the benign depth state (both gamma modes with every flag): the
    first n_lines of it, for line counts on both sides of the pre-pass's block sizes"""
    key = ("combined", n_depth, n_lines)
    if key not in _cases:
        parts = [case(k, n_depth) for k in COMBINED]
        total = sum(p.n_lines for p in parts)
        c = Case("combined", total, n_depth, 99, variants=BOTH, name=f"combined_{n_depth}_{n_lines or total}")
        order = np.argsort(np.concatenate([p.nu for p in parts]), kind="stable")[:n_lines]
        for name in PER_LINE:
            setattr(c, name, np.ascontiguousarray(np.concatenate([getattr(p, name) for p in parts])[order]))
        c.pop_row = np.ascontiguousarray(c.pop_row % c.pop.shape[0])
        c.n_lines = c.nu.size
        _cases[key] = c
    return _cases[key]


def hostile_line_lists(n_depth=3, classes=CLASSES):
    for cls in classes:
        yield case(cls, n_depth)
