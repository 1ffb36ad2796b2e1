"""SpectralSynthesizer with keep_intensities=True and keep_response=True: the derivative chain through the disk integration —
disk_integrated_derivative, disk_weights_to_rays, ray_response, disk_line_sensitivities, observed_disk_line_sensitivities and
chi2_disk_gradient — on the small model of tests/test_gpu_response.py (12 depth points, 300 frequencies, 40 lines, 8 angles, the
gaps thickened as its difference-quotient tests need) with an instrument that has a macroturbulence and 200 pixels.

Margins.  d chi2 / dV against a Richardson quotient of chi2 over observed_disk_integrated (disk_adjoint_reference.richardson_lnv: the
quotient's own uncertainty), plus the rounding of the chi-squares it is made of: the disk integration holds 1e-11 of its scale
(rotation_reference.ROT_TOL), so a chi-square is uncertain by 1e-11 sum_j |c_j observed_j|, two of them per quotient, the
extrapolation's weights 5 / 3, over the step 2 (V h / 4).  disk_line_sensitivities at v = 0 against line_sensitivities(weights = u nu /
lambda): the two chains hold the same factors and differ by where the theta sum is rounded — per element of the response plane (n_theta
+ 4) 2^-52 of sum_theta |term| — after which the same weight plane and line adjoint run on inputs that differ in their last bits, each
run with a summation rounding of its own, n_terms 2^-53 of the absolute sum as tests/test_gpu_line_adjoint.py bounds it, n_terms <=
N_d N_nu: together ((n_theta + 4) + N_d N_nu) 2^-52 of the sum of the absolute terms, which the same chain gives from the per-angle
responses' absolute values.  At v > 0 against quotients of whole steps
with one line's strength scaled: the margin of tests/test_gpu_line_adjoint.py's engine test for the same comparison, per column |coarse -
fine| + FLUX_PARITY max |F| / H.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import disk_adjoint_reference as A
from rotation_reference import ROT_TOL
from stardis_amd import constants as K
from stardis_amd.instrument import Instrument
from test_gpu_response import FLUX_PARITY, H, profiled, small_model, synthesizer, thicken

pytestmark = pytest.mark.gpu

V0 = 24.0
STAGES = ("k_response", "k_emergent_intensity", "k_response_angles", "k_disk_integrate", "k_disk_integrate_adjoint", "k_response_weight",
          "k_line_adjoint", "k_line_param_adjoint")


@pytest.fixture(scope="module")
def m(ctx):
    return thicken(ctx, small_model())


def instrument(ctx, m, **kw):
    lam = K.nu_to_angstrom(m.nus)
    inst = Instrument(np.linspace(lam[40], lam[-40], 201), resolving_power=4.0e4, ctx=ctx, **kw)
    inst.set_radial_velocity(7.0)
    return inst


@pytest.fixture(scope="module")
def stepped(ctx, m):
    syn = synthesizer(ctx, m, keep_intensities=True, keep_response=True, instrument=instrument(ctx, m, v_mac=3.2))
    syn.step()
    ctx.synchronize()
    yield syn
    syn.close()


def chi2_data(syn):
    rng = np.random.default_rng(2)
    base = np.array(syn.observed_disk_integrated(20.0).numpy())
    data = base * (1.0 + 0.01 * rng.standard_normal(base.size))
    ivar = rng.uniform(0.5, 2.0, base.size) / np.nanmax(base) ** 2
    ivar[::17] = 0.0
    return data, ivar


def test_derivative_to_v_is_the_array_entrys_and_zero_raises(ctx, m, stepped):
    from stardis_amd import ops

    syn = stepped
    lam = K.nu_to_angstrom(m.nus)
    rings = np.array(syn.emergent_intensities.numpy()) * m.nus / lam
    F, dF = syn.disk_integrated_derivative(V0)
    F, dF = np.array(F.numpy()), np.array(dF.numpy())
    out, dlnv = ops.disk_integrate(lam, rings, np.sin(m.thetas), m.weights, V0, derivative=True, ctx=ctx)
    assert np.array_equal(F, out) and np.array_equal(dF, dlnv / V0) and np.array_equal(F, syn.disk_integrated(V0).numpy())
    assert np.all(np.isfinite(dF)) and np.abs(dF).max() > 0
    with pytest.raises(ValueError, match="v_rot > 0"):
        syn.disk_integrated_derivative(0.0)
    with pytest.raises(ValueError, match="v_rot > 0"):
        syn.chi2_disk_gradient(*chi2_data(syn), 0.0)


def test_chi2_gradient_to_v_against_a_richardson_quotient(ctx, m, stepped):
    syn = stepped
    data, ivar = chi2_data(syn)
    chi2, dchi2_dv, grad = syn.chi2_disk_gradient(data, ivar, V0)
    obs = np.array(syn.observed_disk_integrated(V0).numpy())
    use = ~np.isnan(obs) & (ivar != 0) & ~syn.instrument.edge_affected(syn.lambdas, v_rot=V0)
    assert 100 < use.sum() < use.size and syn.instrument.edge_affected(syn.lambdas, v_rot=V0).any()
    assert not np.array_equal(syn.instrument.edge_affected(syn.lambdas, v_rot=V0), syn.instrument.edge_affected(syn.lambdas))

    def chi2_at(v):
        o = np.array(syn.observed_disk_integrated(float(v)).numpy())
        r = np.where(use, data, 0.0) - np.where(use, o, 0.0)
        return A.LD(np.sum((np.where(use, ivar, 0.0) * r * r).astype(A.LD)))

    assert float(chi2_at(V0)) == pytest.approx(chi2, rel=1e-13)
    h = 2.0 ** -6
    quotient, unsure = A.richardson_lnv(chi2_at, V0, h)
    c = -2.0 * np.where(use, ivar, 0.0) * (np.where(use, data, 0.0) - np.where(use, obs, 0.0))
    rounding = ROT_TOL * float(np.sum(np.abs(c * np.where(use, obs, 0.0)))) * 2 * (5.0 / 3.0) / (2 * V0 * h / 4)
    allow = float(unsure) / V0 + rounding
    err = abs(dchi2_dv - float(quotient) / V0)
    print(f"d chi2 / dV = {dchi2_dv:.6e}, quotient {float(quotient) / V0:.6e}: |difference| {err:.3e}, allowance {allow:.3e} (the quotient's own "
          f"{float(unsure) / V0:.3e}, rounding {rounding:.3e}); |value| / allowance {abs(dchi2_dv) / allow:.1f}")
    assert err <= allow and abs(dchi2_dv) > 10 * allow
    # the line gradient is observed_disk_line_sensitivities of the same pixel weights
    again = syn.observed_disk_line_sensitivities(c, V0)
    assert np.array_equal(grad.numpy(), again.numpy()) and np.abs(grad.numpy()).max() > 0


def test_line_sensitivities_without_rotation_are_the_flux_chain(ctx, m, stepped):
    syn = stepped
    lam = K.nu_to_angstrom(m.nus)
    u = np.random.default_rng(4).standard_normal(300)
    weights = u * m.nus / lam
    W = np.array(syn.disk_weights_to_rays(u, 0.0).numpy())
    assert np.array_equal(W, m.weights[:, None] * u[None, :] * m.nus[None, :] / lam[None, :])
    got = np.array(syn.disk_line_sensitivities(u, 0.0).numpy())
    want = np.array(syn.line_sensitivities(weights).numpy())
    # the sum of the absolute terms, from the same chain: per-angle responses (one-hot cotangents), their absolute values weighted
    absR = np.zeros((12, 300))
    for th in range(8):
        cot = np.zeros((8, 300))
        cot[th] = m.weights[th]
        absR += np.abs(np.array(syn.ray_response(cot, want_source=False)[0].numpy()))
    terms = np.array(syn._sensitivities_of_response(ctx.upload(absR), ctx.upload(np.abs(weights)), ("strength",), True, False).numpy())
    allow = ((8 + 4) + 12 * 300) * 2.0 ** -52 * terms
    worst = float((np.abs(got - want) / allow).max())
    print(f"disk_line_sensitivities(u, 0) against line_sensitivities(u nu / lambda): worst / allowance {worst:.3e}; largest |value| / terms "
          f"{float((np.abs(want) / terms).max()):.3e}")
    assert worst <= 1.0 and np.all(terms > 0) and np.abs(want).max() > 0
    per_depth = np.array(syn.disk_line_sensitivities(u, 0.0, per_depth=True).numpy())
    assert per_depth.shape == (40, 12) and np.max(np.abs(per_depth.sum(axis=1) - got)) <= 64 * 2.0 ** -52 * terms.max()
    both = syn.disk_line_sensitivities(u, 0.0, wrt=("strength", "damping"))
    assert set(both) == {"strength", "damping"} and np.array_equal(both["strength"].numpy(), got)


def test_line_sensitivities_with_rotation_against_quotients_of_whole_steps(ctx, m, stepped):
    """one line's strength scaled by exp(+-H), exp(+-H / 2), a whole step each, disk_integrated(V0): the margin of
    tests/test_gpu_line_adjoint.py::test_engine_against_difference_quotients"""
    syn = stepped
    F0 = np.array(syn.disk_integrated(V0).numpy())
    worst = 0.0
    for line in m.x_lines[-3:]:
        flux = {}
        for h in (H, -H, H / 2, -H / 2):
            lines = {k: v.copy() for k, v in m.lines.items()}
            lines["alphas"][line] *= np.exp(h)
            other = synthesizer(ctx, m, lines, keep_intensities=True)
            other.step()
            flux[h] = np.array(other.disk_integrated(V0).numpy())
            other.close()
        coarse, fine = (flux[H] - flux[-H]) / (2 * H), (flux[H / 2] - flux[-H / 2]) / H
        extrapolated = (4 * fine - coarse) / 3
        columns = np.argsort(np.abs(extrapolated))[-20:]
        u = np.zeros(300)
        u[columns] = 1.0
        value = float(np.array(syn.disk_line_sensitivities(u, V0).numpy())[line])
        target = float(extrapolated[columns].sum())
        allowance = float((np.abs(coarse - fine)[columns] + FLUX_PARITY * np.abs(F0).max() / H).sum())
        print(f"line {line}: {value:.6e}, difference quotients {target:.6e}, |difference| {abs(value - target):.3e}, allowance {allowance:.3e}, "
              f"|value| / allowance {abs(value) / allowance:.1f}")
        worst = max(worst, abs(value - target) / allowance)
        assert abs(value - target) <= allowance
        assert abs(value) > 10 * allowance  # a zero cannot pass
    # rotation matters: the sensitivity at V0 is not the one without rotation
    assert not np.array_equal(syn.disk_line_sensitivities(u, V0).numpy(), syn.disk_line_sensitivities(u, 0.0).numpy())


def test_the_step_launches_what_it_launched_and_the_calls_launch_their_own(ctx, m, stepped):
    syn = stepped
    u = np.random.default_rng(6).standard_normal(300)
    counts = lambda: {name: ctx.profile(name)[0] for name in STAGES}  # noqa: E731
    none = dict.fromkeys(STAGES, 0)
    with profiled(ctx):
        syn.step()
        ctx.synchronize()
        assert counts() == dict(none, k_response=1, k_emergent_intensity=1)
    before = np.array(syn.line_sensitivities(u).numpy())
    with profiled(ctx):
        after = np.array(syn.line_sensitivities(u).numpy())
        assert counts() == dict(none, k_response_weight=1, k_line_adjoint=1)
    assert np.array_equal(before, after)
    with profiled(ctx):
        syn.disk_line_sensitivities(u, V0)
        ctx.synchronize()
        assert counts() == dict(none, k_disk_integrate_adjoint=1, k_response_angles=1, k_response_weight=1, k_line_adjoint=1)
    plain = synthesizer(ctx, m)
    try:
        with profiled(ctx):
            plain.step()
            ctx.synchronize()
            assert counts() == none
    finally:
        plain.close()


def test_without_the_options_the_methods_raise(ctx, m):
    u = np.zeros(300)
    cot = np.zeros((8, 300))
    bare = synthesizer(ctx, m, keep_response=True)
    try:
        bare.step()
        for call in (lambda: bare.disk_integrated_derivative(V0), lambda: bare.disk_weights_to_rays(u, V0), lambda: bare.ray_response(cot),
                     lambda: bare.disk_line_sensitivities(u, V0)):
            with pytest.raises(RuntimeError, match="keep_intensities=True"):
                call()
        assert bare._disk is None
    finally:
        bare.close()
    no_response = synthesizer(ctx, m, keep_intensities=True, instrument=instrument(ctx, m))
    try:
        no_response.step()
        assert no_response.disk_weights_to_rays(u, V0).shape == (8, 300)  # (these two need the intensities alone)
        assert no_response.ray_response(cot)[0].shape == (12, 300)
        for call in (lambda: no_response.disk_line_sensitivities(u, V0), lambda: no_response.observed_disk_line_sensitivities(np.zeros(200), V0),
                     lambda: no_response.chi2_disk_gradient(np.zeros(200), np.ones(200), V0)):
            with pytest.raises(RuntimeError, match="keep_response=True"):
                call()
        with pytest.raises(ValueError):
            no_response.disk_weights_to_rays(u[:-1], V0)
        with pytest.raises(ValueError):
            no_response.ray_response(cot[:, :-1])
    finally:
        no_response.close()
    no_instrument = synthesizer(ctx, m, keep_intensities=True, keep_response=True)
    try:
        no_instrument.step()
        with pytest.raises(RuntimeError, match="instrument"):
            no_instrument.chi2_disk_gradient(np.zeros(200), np.ones(200), V0)
    finally:
        no_instrument.close()
    rotating = synthesizer(ctx, m, keep_intensities=True, keep_response=True, instrument=instrument(ctx, m, v_rot=5.0))
    try:
        rotating.step()
        for call in (lambda: rotating.chi2_disk_gradient(np.zeros(200), np.ones(200), V0),
                     lambda: rotating.observed_disk_line_sensitivities(np.zeros(200), V0)):
            with pytest.raises(ValueError, match="rotation twice"):
                call()
    finally:
        rotating.close()
