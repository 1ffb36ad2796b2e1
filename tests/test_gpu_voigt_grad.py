"""The term's partial derivatives on the device (sdx_voigt_grad_dev, ops.voigt_grad; sdx_math.h voigt_grad_x), judged point by point and
per Humlicek region on the (x, y) sets of the reference's own vectors G1 (voigt.py:17-86) and G2 (voigt.py:113-150) and on points 8 ulp
either side of every region boundary.

Truth: the reference's formula of the region and its z-derivative at 50 digits (tests/line_param_truth.py; the region by the reference's
predicates on the fp64 x, y).  Distance: |got - truth| / |w'_truth| for K_x = Re w' and for K_y = -Im w'.  Yardstick: the same derivative
formulas in complex128.  Allowed per region: max(4 x the yardstick's worst distance, 2e-13) — the margin of the project's 80-bit
criterion, and the forward routine's own pin (tests/test_gpu_hot_faddeeva.py) as the floor; in region IV 10 x instead of 4 x, the ratio
sdx_math.h documents between the forward routine's recurrence form and the complex Horner form there (1.3e-13 against 1.4e-14).  K of the
routine stays within the forward pin of the reference's Re w.  Doppler width 1 makes x = delta_nu * (1 / dw) exact, so every point — the
boundary-hugging ones included — is evaluated in the region the truth picks.

Every figure is printed before it is asserted; scripts/line_param_truth_table.py writes them to profiles/line_param_truth_classes.json."""
import functools

import numpy as np
import pytest

import line_param_truth as T
import oracle
from conftest import load_golden
from stardis_amd import ops

pytestmark = pytest.mark.gpu

FLOOR = 2e-13  # the forward routine's pin
MARGIN = {1: 4.0, 2: 4.0, 3: 4.0, 4: 10.0}
ULPS = 8


def _step(v, n, towards):
    for _ in range(n):
        v = np.nextafter(v, towards)
    return v


def boundary_points():
    """points ULPS ulp either side of s = |x| + y = 15, s = 5.5 (x stepped) and of y = 0.195 |x| - 0.176 below s = 5.5 (y stepped)"""
    xs, ys = [], []
    for s0 in (15.0, 5.5):
        y = np.concatenate([10.0 ** np.linspace(-6, np.log10(0.9 * s0), 40), [0.0]])
        for sign in (1.0, -1.0):
            for side in (np.inf, -np.inf):
                xs.append(sign * _step(s0 - y, ULPS, side))
                ys.append(y)
    x = np.concatenate([np.linspace(0.95, 4.7, 60), -np.linspace(0.95, 4.7, 60)])
    edge = 0.195 * np.abs(x) - 0.176
    for side in (np.inf, -np.inf):
        xs.append(x)
        ys.append(_step(edge, ULPS, side))
    return np.concatenate(xs), np.concatenate(ys)


@functools.lru_cache(maxsize=None)
def points(which):
    """-> (x, y, gamma) of a point set, the points kept whose y the pre-pass arithmetic returns bit for bit from gamma"""
    if which == "g1":
        g = load_golden("g1_faddeeva")
        x, y = g["z"].real.copy(), g["z"].imag.copy()
    elif which == "g2":
        g = load_golden("g2_voigt")
        x = g["delta_nu"] / g["doppler_width"]
        y = (g["gamma"] / (np.float64(T.SQRT_PI) * np.float64(T.PI))) / g["doppler_width"]
    else:
        x, y = boundary_points()
    gamma = y * (np.float64(T.SQRT_PI) * np.float64(T.PI))
    ok = (gamma / (np.float64(T.SQRT_PI) * np.float64(T.PI))) == y
    assert ok.mean() > 0.5
    return x[ok], y[ok], gamma[ok]


@functools.lru_cache(maxsize=None)
def truth(which):
    x, y, _ = points(which)
    return T.truth_points(x, y), T.reference_order(x, y)


def measure(which):
    """-> {region: dict(points, yardstick_kx, yardstick_ky, got_kx, got_ky, got_k, allowed)} of one point set"""
    x, y, gamma = points(which)
    (reg, w, dw), (reg_y, _, dw_y) = truth(which)
    assert np.array_equal(reg, reg_y)
    k, kx, ky = ops.voigt_grad(x, 1.0, gamma, alpha=T.SQRT_PI)  # amp = sqrt(pi) / (sqrt(pi) * 1) = 1
    ref_k = oracle.faddeeva(x + 1j * y).real
    scale = np.abs(dw)
    out = {}
    for r in (1, 2, 3, 4):
        sel = reg == r
        if not sel.any():
            continue
        yard = max(float((np.abs(dw_y.real - dw.real)[sel] / scale[sel]).max()), float((np.abs(dw_y.imag - dw.imag)[sel] / scale[sel]).max()))
        out[r] = dict(points=int(sel.sum()), yardstick=yard, allowed=max(MARGIN[r] * yard, FLOOR),
                      got_kx=float((np.abs(kx - dw.real)[sel] / scale[sel]).max()), got_ky=float((np.abs(ky + dw.imag)[sel] / scale[sel]).max()),
                      got_k=float((np.abs(k - ref_k)[sel] / np.where(ref_k[sel] != 0, np.abs(ref_k[sel]), 1.0)).max()))  # (absolute where Re w = 0: y = 0 in the wing)
    return out


@pytest.mark.parametrize("which", ["g1", "g2", "boundaries"])
def test_derivatives_point_by_point(ctx, which):
    table = measure(which)
    for r, v in table.items():
        print(f"{which}, region {r}: {v['points']} points; |dK_x| / |w'| {v['got_kx']:.3e}, |dK_y| / |w'| {v['got_ky']:.3e} (yardstick {v['yardstick']:.3e}, "
              f"allowed {v['allowed']:.3e}); K against the reference's Re w {v['got_k']:.3e}")
    assert set(table) == {1, 2, 3, 4}
    assert all(v["points"] >= (50 if which == "boundaries" else 100) for v in table.values()), {r: v["points"] for r, v in table.items()}
    for r, v in table.items():
        assert v["got_kx"] <= v["allowed"] and v["got_ky"] <= v["allowed"], (which, r, v)
        assert v["got_k"] <= FLOOR, (which, r, v)


def test_amplitude_and_doppler_width_scale_the_outputs(ctx):
    """ops.voigt_grad forms inv_dw, y and amp as the pre-pass does (voigt.py:148-149): with a Doppler width and a strength the outputs
    are amp (K, K_x, K_y) at x = delta_nu / dw, y = gamma / (sqrt(pi) pi dw); scalars come back as scalars"""
    rng = np.random.default_rng(3)
    n = 2000
    dw = 10.0 ** rng.uniform(8.5, 9.5, n)
    x, y = rng.uniform(-25, 25, n), 10.0 ** rng.uniform(-4, 1, n)
    s, edge = np.abs(x) + y, y - (0.195 * np.abs(x) - 0.176)
    keep = (np.abs(s - 15) > 1e-6) & (np.abs(s - 5.5) > 1e-6) & (np.abs(edge) > 1e-6)
    x, y, dw = x[keep], y[keep], dw[keep]
    alpha = 10.0 ** rng.uniform(-8, -4, x.size)
    delta_nu, gamma = x * dw, y * dw * (T.SQRT_PI * T.PI)
    xr, yr = delta_nu / dw, (gamma / (T.SQRT_PI * T.PI)) / dw
    reg, w, dwdz = T.truth_points(xr, yr)
    amp = alpha / (T.SQRT_PI * dw)
    k, kx, ky = ops.voigt_grad(delta_nu, dw, gamma, alpha)
    # x = delta_nu * (1 / dw) is within an ulp of the reference's x: the derivative moves by |x w''| 2^-52 ~ (2 + 2 x^2) 2^-52 |w'| at most
    allowed = (FLOOR + (2 + 2 * xr * xr) * 2.0**-52) * amp * np.abs(dwdz)
    worst = max(float((np.abs(kx - amp * dwdz.real) / allowed).max()), float((np.abs(ky + amp * dwdz.imag) / allowed).max()))
    print(f"{x.size} points with Doppler widths and strengths: worst |got - amp w'| / allowed {worst:.3e}")
    assert worst <= 1.0
    assert float((np.abs(k - amp * w.real) / (amp * np.abs(w))).max()) <= FLOOR + 60 * 2.0**-52
    one = ops.voigt_grad(float(delta_nu[0]), float(dw[0]), float(gamma[0]), float(alpha[0]))
    assert all(np.ndim(v) == 0 for v in one) and (float(one[0]), float(one[1]), float(one[2])) == (k[0], kx[0], ky[0])
