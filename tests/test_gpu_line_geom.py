"""The line launch with its geometry formed on the host (stardis_amd/csrc/sdx_line_geom.h), on the GPU: line opacity through the existing
entry points against the CPU oracle at the suite's tolerance (1e-12, evaluation counts equal), at the smallest shapes where a block index
decoded wrongly would show — a wrong index puts a frequency's sum into another column or row, or leaves a unit out, so the plane is then
grossly wrong and no tolerance of its own is needed.  tests/test_line_geom_cpu.py checks the decode itself over every block and wave."""
import functools

import numpy as np
import pytest

import oracle
from stardis_amd import _lib, ops, synth
from stardis_amd.engine import SpectralSynthesizer

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def atmosphere(n_depth):
    """the solar model's columns resampled to n_depth points (what synth_lines and the synthesizer read of it)"""
    atm = synth.solar_atmosphere()
    if n_depth == atm["temperatures"].size:
        return atm
    x = np.linspace(0.0, 1.0, atm["temperatures"].size)
    xi = np.linspace(0.0, 1.0, n_depth)
    out = dict(atm)
    for k in ("temperatures", "n_e", "n_h", "r"):
        out[k] = np.interp(xi, x, atm[k])
    out["dist"] = out["r"][1:] - out["r"][:-1]
    if np.ndim(atm["microturbulence"]):
        out["microturbulence"] = np.interp(xi, x, atm["microturbulence"])
    return out


def grid(n_points, lam0=6560.0):
    return synth.tracing_grid(lam0, lam0 * (1.0 + n_points / 3.0e5), n_override=n_points)


def line_args(n_depth, nus, lines):
    return (n_depth, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])


def against_oracle(ctx, n_depth, nus, lines, tol=1e-12, ref=None):
    args = line_args(n_depth, nus, lines)
    got, evals = ops.calc_alan_entries(*args, return_evaluations=True, ctx=ctx)
    ref, ref_evals = ref if ref is not None else oracle.calc_alan_entries(*args, return_evals=True)
    err = rel_err(got, ref)
    print(f"N_nu {nus.size} N_l {lines['line_nus'].size} N_d {n_depth}: rel err {err:.2e}, evaluations {evals} / {ref_evals}")
    assert np.all(np.isfinite(got)) and ref_evals > 0
    assert err < tol and evals == ref_evals


@pytest.mark.parametrize("n_points", [7, 65, 2051])
def test_small_grids_with_surplus_workgroups(ctx, n_points):
    """1, 1 and 9 tiles; the narrow role's last round of 32 workgroups is mostly surplus; 200 lines, some of them wide"""
    atm = atmosphere(56)
    nus = grid(n_points)
    lines = synth.synth_lines(nus, atm, 200, seed=31, mix=(0.8, 0.15, 0.05))
    against_oracle(ctx, 56, nus, lines)


@pytest.mark.parametrize("n_depth", [65, 129])
def test_two_and_three_depth_chunks(ctx, n_depth):
    """more than 64 depths: the narrow role's units carry a depth chunk, the one place where a wave still divides (by multiplication)"""
    atm = atmosphere(n_depth)
    nus = grid(2051)
    lines = synth.synth_lines(nus, atm, 200, seed=32, mix=(0.8, 0.15, 0.05))
    against_oracle(ctx, n_depth, nus, lines)


def shards_against_the_whole_grid(ctx, n_depth, nus, lines, shards):
    """alpha_line, total_alphas and F_nu of the shards, side by side, are the whole grid's bit for bit"""
    atm = atmosphere(n_depth)
    cont = synth.synth_continuum_state(atm)
    th, w = synth.thetas_and_weights(4)
    full = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx)
    full.step()
    parts_a, parts_t, parts_F = [], [], []
    for begin, count in shards:
        s = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, shard=(begin, count))
        s.step()
        parts_a.append(s.alpha_line()), parts_t.append(s.total_alphas()), parts_F.append(s.F_nu())
    assert np.array_equal(np.concatenate(parts_a, axis=1), full.alpha_line())
    assert np.array_equal(np.concatenate(parts_t, axis=1), full.total_alphas())
    assert np.array_equal(np.concatenate(parts_F, axis=1), full.F_nu())


def test_unequal_shards_with_an_odd_first_column_against_the_whole_grid(ctx):
    nus = grid(2051)
    lines = synth.synth_lines(nus, atmosphere(56), 200, seed=33, mix=(0.8, 0.15, 0.05))
    shards_against_the_whole_grid(ctx, 56, nus, lines, ((0, 777), (777, nus.size - 777)))


DENSE = [(16384, 8192), (32768, 16384), (2048, 8192)]


@functools.lru_cache(maxsize=None)
def dense_case(n_points, n_lines):
    """a dense list of narrow lines on nine depths (they keep the oracle quick), with the oracle's opacity and evaluation count: computed
    once per shape, read-only"""
    nus = grid(n_points)
    lines = synth.synth_lines(nus, atmosphere(9), n_lines, seed=34, mix=(1.0, 0.0, 0.0))
    ref, ref_evals = oracle.calc_alan_entries(*line_args(9, nus, lines), return_evals=True)
    ref.setflags(write=False)
    return nus, lines, (ref, ref_evals)


@pytest.mark.parametrize("n_points,n_lines", DENSE)
def test_dense_lists(ctx, n_points, n_lines):
    """16 384 x 8192: two frequencies per narrow wave; 32 768 x 16 384: four, and the far role merged into the launch; 2048 x 8192 (four
    lines per grid point): the subsets kernel."""
    nus, lines, ref = dense_case(n_points, n_lines)
    against_oracle(ctx, 9, nus, lines, ref=ref)


@pytest.mark.parametrize("n_points,n_lines", DENSE)
def test_dense_lists_in_the_mixed_precision_mode(ctx, n_points, n_lines):
    """the fp32 records' walk at two and four frequencies per wave and over line subsets (the small tests reach it at one frequency per
    wave only), at the mode's stated 1e-4 against the oracle"""
    nus, lines, (ref, _) = dense_case(n_points, n_lines)
    args = line_args(9, nus, lines)
    a64 = ops.calc_alan_entries(*args, ctx=ctx)
    try:
        ctx.set_option("mixed_precision", 1)
        a32 = ops.calc_alan_entries(*args, ctx=ctx)
    finally:
        ctx.set_option("mixed_precision", 0)
    print(f"N_nu {n_points} N_l {n_lines} mixed precision: rel err", rel_err(a32, ref))
    assert not np.array_equal(a32, a64)  # the mode really took the fp32 route
    assert rel_err(a32, ref) < 1e-4


@pytest.mark.parametrize("mixed", [0, 1], ids=["fp64", "mixed"])
@pytest.mark.parametrize("n_points,n_lines,cut", [(32768, 16384, 12001), (2048, 8192, 777)], ids=["grouped", "subsets"])
def test_the_narrow_sums_depend_neither_on_the_frequencies_per_wave_nor_on_the_shard(ctx, n_points, n_lines, cut, mixed):
    """What lets one narrow walk stand for all its forms.  32 768 x 16 384: the whole grid walks four frequencies per wave, the shard
    of 12 001 columns one and that of 20 767 two, and the boundary is a multiple of neither group size.  2048 x 8192: the subsets kernel,
    whose groups of four frequencies the boundary 777 cuts.  In the mixed-precision mode too, where the fp32 terms are folded into the
    fp64 sum per stretch of the LIST so that this holds."""
    nus = grid(n_points)
    lines = synth.synth_lines(nus, atmosphere(9), n_lines, seed=34, mix=(1.0, 0.0, 0.0))
    try:
        ctx.set_option("mixed_precision", mixed)
        shards_against_the_whole_grid(ctx, 9, nus, lines, ((0, cut), (cut, n_points - cut)))
    finally:
        ctx.set_option("mixed_precision", 0)


def test_mixed_precision_at_its_stated_tolerance(ctx):
    atm = atmosphere(56)
    nus = grid(2051)
    lines = synth.synth_lines(nus, atm, 400, seed=35, mix=(0.8, 0.15, 0.05))
    args = line_args(56, nus, lines)
    ref = oracle.calc_alan_entries(*args)
    a64 = ops.calc_alan_entries(*args, ctx=ctx)
    try:
        ctx.set_option("mixed_precision", 1)
        a32 = ops.calc_alan_entries(*args, ctx=ctx)
    finally:
        ctx.set_option("mixed_precision", 0)
    print("mixed precision: rel err", rel_err(a32, ref))
    assert not np.array_equal(a32, a64)  # the mode really took the fp32 route
    assert rel_err(a32, ref) < 1e-4
