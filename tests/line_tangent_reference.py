"""The tangent of the line-opacity sum restated on the CPU (no test in here; tests/test_line_tangent_cpu.py checks the restatement,
tests/test_gpu_line_tangent.py judges the kernel by it).

For the directions a = d ln alpha, g = d ln gamma, b = d ln doppler and n = d nu_l (Hz) of every (line, depth) item the plane is
    d alpha[d][i] = sum over the items whose window covers i of  a T + g (amp y K_y) - b (T + amp x K_x + amp y K_y) - n (amp K_x / doppler)
at the reference's windows and regions: the extended-precision per-term pieces of line_param_truth.terms(name) — the very pieces
line_param_truth.restated sums per item — scattered into a plane instead.  With it come the SCALE BUILT FROM ABSOLUTE PIECES
    scale[d][i] = sum |a| |T| + |g| y amp |w'| + |b| (|T| + amp |x| |w'| + y amp |w'|) + |n| amp |w'| / doppler
(the Doppler derivative cancels to leading order in the Lorentz wing, as in line_param_truth) and the number of items that cover an
element, n_cover.  The criterion is the project's per-term rule, line_adjoint_truth.bound:
    |got - ref| <= (OPACITY_RTOL + n_cover 2^-53) scale,        and exactly 0.0 where scale == 0."""
import types

import numpy as np

import line_adjoint_truth as A
import line_param_truth as T
from line_adjoint_truth import SHAPES, bound, model  # noqa: F401  (the same models: imported, not restated)

LD = np.longdouble
NAMES = ("strength", "damping", "doppler", "centre")
ALL_MODELS = ("tiny", "odd", "small", "ragged", "long", "inner")


def directions(name, per_depth, which=NAMES, seed=101):
    """seeded normal directions of the model's lines -> dict name -> (n_lines,) or, per_depth, (n_lines, n_depth); the centre's in Hz,
    in units of the list's median Doppler width so that it weighs what the logarithmic ones weigh.  Every name draws the same numbers
    whatever `which` asks for."""
    m = model(name)
    rng = np.random.default_rng(seed)
    shape = (m.n_lines, m.n_depth) if per_depth else (m.n_lines,)
    drawn = {k: rng.standard_normal(shape) for k in NAMES}
    drawn["centre"] = drawn["centre"] * float(np.median(m.lines["doppler_widths"]))
    return {k: drawn[k] for k in which}


def species_mask(name):
    """a 0 / 1 mask over the model's lines: the lines whose windows are the 20-point floor at every depth (line_adjoint_truth.regimes),
    so that where the list has wider lines there are elements only unmasked lines cover; every third line where that picks none or all"""
    m = model(name)
    mask = np.zeros(m.n_lines)
    mask[A.regimes(name)[0]] = 1.0
    if mask.all() or not mask.any():
        mask = (np.arange(m.n_lines) % 3 == 0).astype(np.float64)
    return mask


def per_item(m, v):
    """a direction (None, scalar, (n_lines,) or (n_lines, n_depth)) -> (n_lines, n_depth)"""
    if v is None:
        return np.zeros((m.n_lines, m.n_depth))
    v = np.asarray(v, dtype=np.float64)
    return np.broadcast_to(v.reshape(m.n_lines, -1) if v.ndim else v, (m.n_lines, m.n_depth))


def plane(name, strength=None, damping=None, doppler=None, centre=None, lines=None):
    """-> namespace(value, scale, n_cover), each (n_depth, n_nu) fp64 / int: the tangent plane of the model along the directions;
    lines: only these lines (default: all)"""
    m = model(name)
    a, g, b, n = (per_item(m, v) for v in (strength, damping, doppler, centre))
    value, scale = np.zeros((m.n_depth, m.n_nu), dtype=LD), np.zeros((m.n_depth, m.n_nu), dtype=LD)
    n_cover = np.zeros((m.n_depth, m.n_nu), dtype=np.int64)
    terms = T.terms(name)
    for l in (range(m.n_lines) if lines is None else lines):
        t = terms[l]
        for d in range(m.n_depth):
            cut = slice(t.seg[d], t.seg[d + 1])
            col = t.col[cut]  # (an arange: no column twice)
            y, dw = LD(t.y[d]), LD(t.doppler[d])
            al, gl, bl, nl = (LD(v[l, d]) for v in (a, g, b, n))
            value[d, col] += al * t.k[cut] + gl * (y * t.ky[cut]) - bl * (t.k[cut] + t.xkx[cut] + y * t.ky[cut]) - nl * (t.kx[cut] / dw)
            scale[d, col] += (abs(al) * t.absk[cut] + abs(gl) * (y * t.absd[cut]) + abs(bl) * (t.absk[cut] + t.absx[cut] + y * t.absd[cut])
                              + abs(nl) * (t.absd[cut] / dw))
            n_cover[d, col] += 1
    return types.SimpleNamespace(value=value.astype(np.float64), scale=scale.astype(np.float64), n_cover=n_cover)


def worst_ratio(got, ref, factor=1.0):
    """-> the largest |got - ref.value| / bound over the elements with a scale (0.0 if there is none); asserts exact zeros elsewhere"""
    got = np.asarray(got)
    assert got.shape == ref.value.shape, (got.shape, ref.value.shape)
    dead = ref.scale == 0
    assert not got[dead].any(), "an element no direction reaches must be exactly 0.0"
    if dead.all():
        return 0.0
    b = bound(ref.scale[~dead], ref.n_cover[~dead], factor)
    return float((np.abs(got[~dead] - ref.value[~dead]) / b).max())


def sorted_tables(m):
    """-> (order, line_nus, doppler, gammas, alphas) of the model in ascending frequency (stable), as the raw entry point wants them"""
    L = m.lines
    order = np.argsort(L["line_nus"], kind="stable")
    return (order,) + tuple(np.ascontiguousarray(L[k][order]) for k in ("line_nus", "doppler_widths", "gammas", "alphas"))
