"""The line-profile sensitivities restated on the CPU (no test in here; tests/test_line_param_truth_cpu.py checks the restatement,
tests/test_gpu_voigt_grad.py and tests/test_gpu_line_param_adjoint.py judge the kernels by it).

What is differentiated is the reference's Faddeeva formula in the Humlicek region it picks (voigt.py:39-84), the region chosen by the
reference's predicates on the fp64 x = delta_nu / doppler_width and y = (gamma / (sqrt(pi) pi)) / doppler_width (voigt.py:148), the
region boundaries held fixed.  Each region's w is analytic in z = x + i y:  K = Re w,  K_x = Re w',  K_y = -Im w'.

Two statements of the same four formulas and their z-derivatives:
  w_mp, dw_mp   mpmath at DPS = 50 digits, one point at a time: the truth of the point-wise tests;
  w_dw_ld       numpy's extended precision (64-bit mantissa), vectorised: the truth of the SUMS, which run over up to a million terms
                per model.  tests/test_line_param_truth_cpu.py holds it against the mpmath statement (both rounded to fp64: < 1e-15 of |w'|), three orders below
                the per-term allowance of the sums.

restated(name, W, shard) has the shape of line_adjoint_truth.restated, on the same models, windows and regimes (imported): per output
s_ld, s_l, the term counts and a SCALE BUILT FROM ABSOLUTE PIECES
    damping:  sum |W| amp y |w'|          doppler:  sum |W| amp (|K| + |x| |w'| + y |w'|)          centre:  sum |W| amp |w'| / doppler
— the Doppler derivative cancels to leading order in the Lorentz wing (the wing does not depend on the Doppler width), so a bound scaled by
the result itself would mean nothing there."""
import functools
import types

import mpmath
import numpy as np

import line_adjoint_truth as A
from line_adjoint_truth import SHAPES, bound, model, regimes, windows  # noqa: F401  (the same models: imported, not restated)

DPS = 50
SQRT_PI = float(np.sqrt(np.pi, dtype=float))  # voigt.py:12
PI = float(np.pi)
LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 2e-19, "numpy's long double is not the 64-bit-mantissa format on this machine"

P3 = (0.5642236, 3.778987, 11.96482, 20.20933, 16.4955)  # region III, descending powers of t (voigt.py:60)
Q3 = (1.0, 6.699398, 21.69274, 39.27121, 38.82363, 16.4955)  # (:62-63)
P4 = (0.56419, 1.320522, 35.7668, 219.031, 1540.787, 3321.99, 36183.31)  # region IV, descending powers of m = -u (:70-78)
Q4 = (1.0, 1.84144, 61.5704, 364.219, 2186.18, 9022.23, 24322.8, 32066.6)  # (:79-83)
C2 = 1.4104739589  # region II (:52)


def region(x, y):
    """voigt.py:35-44 on fp64 x, y -> 1 ... 4 (arrays or scalars)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = np.abs(x) + y
    return np.where(s > 15.0, 1, np.where(s > 5.5, 2, np.where(y >= 0.195 * np.abs(x) - 0.176, 3, 4)))


def _poly(coef, v, zero, one):
    """-> (p(v), p'(v)) by Horner, any number type"""
    p, dp = zero, zero
    for c in coef:
        dp = dp * v + p
        p = p * v + c * one
    return p, dp


def _formulas(reg, z, i, exp, const):
    """region `reg`'s w(z) and dw/dz for the number type whose imaginary unit is i, exponential exp and constants const(float)"""
    one = const(1.0)
    k = one / const(SQRT_PI)
    if reg == 1:  # w = i k z / (z^2 - 1/2)
        a = z * z - const(0.5)
        return i * k * z / a, -i * k * (z * z + const(0.5)) / (a * a)
    if reg == 2:  # w = i z (z^2 k - c) / (3/4 + z^2 (z^2 - 3))
        s = z * z
        n, dn = z * (s * k - const(C2)), const(3.0) * s * k - const(C2)
        q, dq = const(0.75) + s * (s - const(3.0)), const(2.0) * z * (const(2.0) * s - const(3.0))
        return i * n / q, i * (dn * q - n * dq) / (q * q)
    t = -i * z  # y - i x
    zero = z * const(0.0)
    if reg == 3:  # w = P(t) / Q(t),  dt/dz = -i
        p, dp = _poly([const(c) for c in P3], t, zero, one)
        q, dq = _poly([const(c) for c in Q3], t, zero, one)
        return p / q, -i * (dp * q - p * dq) / (q * q)
    # w = exp(u) - t P(m) / Q(m),  u = t^2 = -z^2,  m = -u = z^2
    m = z * z
    p, dp = _poly([const(c) for c in P4], m, zero, one)
    q, dq = _poly([const(c) for c in Q4], m, zero, one)
    f, df_dm = p / q, (dp * q - p * dq) / (q * q)
    e = exp(-m)
    return e - t * f, -const(2.0) * z * e + i * (f + const(2.0) * m * df_dm)  # d(t f)/dz = -i f + t df/dm 2 z = -i (f + 2 m df/dm)


def _digits():
    """at least DPS digits (never fewer than the caller works with: mpmath.diff raises the precision around its evaluations)"""
    return mpmath.workdps(max(mpmath.mp.dps, DPS))


def w_mp(reg, z):
    with _digits():
        return _formulas(reg, mpmath.mpc(z), mpmath.mpc(0, 1), mpmath.exp, mpmath.mpf)[0]


def dw_mp(reg, z):
    with _digits():
        return _formulas(reg, mpmath.mpc(z), mpmath.mpc(0, 1), mpmath.exp, mpmath.mpf)[1]


def truth_points(x, y):
    """fp64 arrays x, y -> (region, w, w') with w, w' complex128 arrays rounded from the mpmath values (the region from `region`)"""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    reg = region(x, y)
    w, dw = np.empty(x.size, dtype=np.complex128), np.empty(x.size, dtype=np.complex128)
    with mpmath.workdps(DPS):
        for j in range(x.size):
            a, b = _formulas(int(reg[j]), mpmath.mpc(float(x[j]), float(y[j])), mpmath.mpc(0, 1), mpmath.exp, mpmath.mpf)
            w[j], dw[j] = complex(a), complex(b)
    return reg, w, dw


def w_dw_ld(x, y):
    """fp64 arrays x, y -> (w, w') as extended-precision complex arrays, every point in the region `region` picks"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    reg = region(x, y)
    z = x.astype(LD) + CLD(1j) * y.astype(LD)
    w, dw = np.zeros(z.shape, dtype=CLD), np.zeros(z.shape, dtype=CLD)
    for r in (1, 2, 3, 4):
        sel = reg == r
        if sel.any():
            w[sel], dw[sel] = _formulas(r, z[sel], CLD(1j), np.exp, LD)
    return w, dw


def reference_order(x, y):
    """The yardstick of tests/test_gpu_voigt_grad.py: the same formulas and derivatives (_formulas: complex Horner steps, the quotient
    rule written out, complex division) in complex128, no extended precision and no FMA -> (region, w, w')"""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    reg = region(x, y)
    z = x + 1j * y
    w, dw = np.zeros(z.shape, dtype=np.complex128), np.zeros(z.shape, dtype=np.complex128)
    for r in (1, 2, 3, 4):
        sel = reg == r
        if sel.any():
            w[sel], dw[sel] = _formulas(r, z[sel], 1j, np.exp, np.float64)
    return reg, w, dw


@functools.lru_cache(maxsize=None)
def terms(name):
    """Per line of the model the terms of all its windows, flat and depth by depth: a list of namespaces with the half-open ranges
    `seg` (n_depth + 1 offsets), the grid columns `col`, and per term amp K, amp K_x, amp x K_x, amp K_y, amp |w'| in extended
    precision; with them y and doppler per depth."""
    m = model(name)
    L = m.lines
    lo, hi = windows(name)
    out = []
    for l in range(m.n_lines):
        cols, xs, ys, amps, seg = [], [], [], [], [0]
        y_d, dw_d = np.empty(m.n_depth), np.empty(m.n_depth)
        for d in range(m.n_depth):
            dw = L["doppler_widths"][l, d]
            g = L["gammas"][l, d if L["gammas"].shape[1] > 1 else 0]
            i = np.arange(lo[l, d], hi[l, d])
            y_d[d], dw_d[d] = (g / (SQRT_PI * PI)) / dw, dw  # voigt.py:148
            cols.append(i)
            xs.append((m.nus[i] - L["line_nus"][l]) / dw)
            ys.append(np.full(i.size, y_d[d]))
            amps.append(np.full(i.size, L["alphas"][l, d] / (SQRT_PI * dw)))  # voigt.py:149, base.py:627
            seg.append(seg[-1] + i.size)
        x, y, amp = np.concatenate(xs), np.concatenate(ys), np.concatenate(amps).astype(LD)
        w, dw_dz = w_dw_ld(x, y)
        kx = dw_dz.real
        out.append(types.SimpleNamespace(seg=np.array(seg), col=np.concatenate(cols), y=y_d, doppler=dw_d, k=amp * w.real, kx=amp * kx,
                                         xkx=amp * (x.astype(LD) * kx), ky=amp * -dw_dz.imag, absk=amp * np.abs(w.real),
                                         absx=amp * np.abs(x.astype(LD)) * np.abs(dw_dz), absd=amp * np.abs(dw_dz)))
    return out


def restated(name, W=None, shard=None):
    """-> namespace(damping, doppler, centre), each a namespace(s_ld, s_l, scale_ld, scale_l, terms_ld, terms_l) over the columns
    [begin, begin + count) of `shard` (default: all); W (n_depth, n_nu) on the whole grid (default: the model's)"""
    m = model(name)
    W = m.W if W is None else W
    b, n = (0, m.n_nu) if shard is None else shard
    Wc = np.zeros(W.shape, dtype=LD)
    Wc[:, b:b + n] = W[:, b:b + n]
    lo, hi = windows(name)
    n_terms = np.maximum(np.minimum(hi, b + n) - np.maximum(lo, b), 0)
    s = {k: np.zeros((m.n_lines, m.n_depth), dtype=LD) for k in ("damping", "doppler", "centre")}
    scale = {k: np.zeros((m.n_lines, m.n_depth), dtype=LD) for k in s}
    for l, t in enumerate(terms(name)):
        for d in range(m.n_depth):
            cut = slice(t.seg[d], t.seg[d + 1])
            wt = Wc[d, t.col[cut]]
            aw = np.abs(wt)
            y, dw = LD(t.y[d]), LD(t.doppler[d])
            s0, sx, sxx, sy = (wt * t.k[cut]).sum(), (wt * t.kx[cut]).sum(), (wt * t.xkx[cut]).sum(), (wt * t.ky[cut]).sum()
            a0, ax, ad = (aw * t.absk[cut]).sum(), (aw * t.absx[cut]).sum(), (aw * t.absd[cut]).sum()
            s["damping"][l, d], scale["damping"][l, d] = y * sy, y * ad
            s["doppler"][l, d], scale["doppler"][l, d] = -(s0 + sxx + y * sy), a0 + ax + y * ad
            s["centre"][l, d], scale["centre"][l, d] = -sx / dw, ad / dw
    out = {}
    for k in s:
        out[k] = types.SimpleNamespace(s_ld=s[k].astype(np.float64), s_l=s[k].sum(axis=1).astype(np.float64), scale_ld=scale[k].astype(np.float64),
                                       scale_l=scale[k].sum(axis=1).astype(np.float64), terms_ld=n_terms, terms_l=n_terms.sum(axis=1))
    return types.SimpleNamespace(**out)
