"""The line launch with its geometry formed on the host (stardis_amd/csrc/sdx_line_geom.h), on the GPU: line opacity through the existing
entry points against the CPU oracle at the suite's tolerance (1e-12, evaluation counts equal), at the smallest shapes where a block index
decoded wrongly would show — a wrong index puts a frequency's sum into another column or row, or leaves a unit out, so the plane is then
grossly wrong and no tolerance of its own is needed.  tests/test_line_geom_cpu.py checks the decode itself over every block and wave."""
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
    """the solar model's columns resampled to n_depth points (what synth_lines reads of it)"""
    atm = synth.solar_atmosphere()
    if n_depth == atm["temperatures"].size:
        return atm
    x = np.linspace(0.0, 1.0, atm["temperatures"].size)
    xi = np.linspace(0.0, 1.0, n_depth)
    out = dict(atm)
    for k in ("temperatures", "n_e"):
        out[k] = np.interp(xi, x, atm[k])
    if np.ndim(atm["microturbulence"]):
        out["microturbulence"] = np.interp(xi, x, atm["microturbulence"])
    return out


def grid(n_points, lam0=6560.0):
    return synth.tracing_grid(lam0, lam0 * (1.0 + n_points / 3.0e5), n_override=n_points)


def against_oracle(ctx, n_depth, nus, lines, tol=1e-12):
    args = (n_depth, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])
    got, evals = ops.calc_alan_entries(*args, return_evaluations=True, ctx=ctx)
    ref, ref_evals = oracle.calc_alan_entries(*args, return_evals=True)
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


def test_unequal_shards_with_an_odd_first_column_against_the_whole_grid(ctx):
    atm = atmosphere(56)
    nus = grid(2051)
    lines = synth.synth_lines(nus, atm, 200, seed=33, mix=(0.8, 0.15, 0.05))
    cont = synth.synth_continuum_state(atm)
    th, w = synth.thetas_and_weights(4)
    full = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx)
    full.step()
    parts_a, parts_t, parts_F = [], [], []
    for begin, count in ((0, 777), (777, nus.size - 777)):
        s = SpectralSynthesizer(nus, atm["temperatures"], atm["dist"], th, w, lines, cont, ctx=ctx, shard=(begin, count))
        s.step()
        parts_a.append(s.alpha_line()), parts_t.append(s.total_alphas()), parts_F.append(s.F_nu())
    assert np.array_equal(np.concatenate(parts_a, axis=1), full.alpha_line())
    assert np.array_equal(np.concatenate(parts_t, axis=1), full.total_alphas())
    assert np.array_equal(np.concatenate(parts_F, axis=1), full.F_nu())


@pytest.mark.parametrize("n_points,n_lines", [(16384, 8192), (32768, 16384), (2048, 8192)])
def test_dense_lists(ctx, n_points, n_lines):
    """16 384 x 8192: two frequencies per narrow wave; 32 768 x 16 384: four, and the far role merged into the launch; 2048 x 8192 (four
    lines per grid point): the subsets kernel.  Nine depths keep the oracle quick."""
    atm = atmosphere(9)
    nus = grid(n_points)
    lines = synth.synth_lines(nus, atm, n_lines, seed=34, mix=(1.0, 0.0, 0.0))
    against_oracle(ctx, 9, nus, lines)


def test_mixed_precision_at_its_stated_tolerance(ctx):
    atm = atmosphere(56)
    nus = grid(2051)
    lines = synth.synth_lines(nus, atm, 400, seed=35, mix=(0.8, 0.15, 0.05))
    args = (56, nus, lines["line_nus"], lines["doppler_widths"], lines["gammas"], lines["alphas"])
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
