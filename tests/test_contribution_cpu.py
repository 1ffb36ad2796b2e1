"""The numpy restatement of the flux contribution function (tests/contribution_reference.py: built from the source function and
the weights) against the golden fixture g15 (built from the reference's own traced intensities, tests/golden/
make_golden_contribution.py), on the inputs of g7: 200 frequencies, 56 depths, 1 / 4 / 20 angles.

Both sides take exp and log as correctly rounded functions (contribution_reference.exact_exp / exact_log; the golden's generator pins
them in the reference's module while it runs).  Left to numpy they differ in the last bit between builds (numpy 1.26.4 against 2.2.6:
2 364 of 11 200 logarithms, 4 % of the exponentials), and the scheme amplifies that bit — log(alpha) ~ -30, and w2 = 2 w1 -
tau^2 exp(-tau) cancels six digits in a thin surface gap — to 7.0 / 4.2 / 3.1e-12 of F_nu[-1]: a golden made on one numpy's own functions can be reproduced on
another only to that.  The same 7e-12 separate g15 from g7's recorded F_nu (made on numpy's functions), which is why the sum identity is
checked against the emergent flux of g15's own run.  Measured, max over the 198 ordinary columns of |C - C_g15| / F_nu[-1] at 1 / 4 / 20
angles: 2.6e-16 / 1.8e-16 / 8.6e-17, the same figures under numpy 2.2.6 and under numpy 1.26.4 (bound 1e-13); the restatement
on numpy 2.2.6's own exp and log: 2.1e-12 / 1.7e-12 / 4.7e-13."""
import numpy as np
import pytest

import contribution_reference as cref
from conftest import load_golden


def _inputs(n_theta):
    g7, g15 = load_golden("g7_raytrace"), load_golden("g15_contribution")
    ray = g7["dist"].reshape(-1, 1) / np.cos(g7[f"thetas_{n_theta}"])
    return g7, g15, ray


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_restatement_reproduces_the_golden(n_theta):
    g7, g15, ray = _inputs(n_theta)
    F = g7[f"F_nu_{n_theta}"][-1]
    C_ref = g15[f"C_{n_theta}"]
    C = cref.contribution_function(g7["nus"], g7["temperatures"], ray, g7[f"weights_{n_theta}"], g7["total_alphas"], source=g7["blackbody"], exact=True)
    ok = np.isfinite(F)
    assert np.flatnonzero(~ok).tolist() == [11]  # exactly one column is left out: the reference's own flux is NaN there
    assert F[7] == 0.0 and not C_ref[:, 7].any() and not C[:, 7].any()  # opacity 0 at all depths: exactly 0
    ordinary = ok.copy()
    ordinary[7] = False
    assert ordinary.sum() == 198
    err = np.max(np.abs(C[:, ordinary] - C_ref[:, ordinary]) / F[ordinary])
    print(f"n_theta={n_theta}: restatement vs golden {err:.2e} of F_nu[-1]")
    assert err <= 1e-13
    # the Planck function of the restatement itself (what the GPU tests use) gives the same within the same bound
    C_planck = cref.contribution_function(g7["nus"], g7["temperatures"], ray, g7[f"weights_{n_theta}"], g7["total_alphas"], exact=True)
    assert np.max(np.abs(C_planck[:, ordinary] - C_ref[:, ordinary]) / F[ordinary]) <= 1e-13
    assert not C_planck[:, 7].any()
    # numpy's own exp and log (what the restatement runs on at sizes where 10 us per value is too slow): within the flux tolerance
    C_numpy = cref.contribution_function(g7["nus"], g7["temperatures"], ray, g7[f"weights_{n_theta}"], g7["total_alphas"])
    err = np.max(np.abs(C_numpy[:, ordinary] - C_ref[:, ordinary]) / F[ordinary])
    print(f"n_theta={n_theta}: restatement on numpy's exp / log vs golden {err:.2e} of F_nu[-1]")
    assert err <= 1e-10


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_golden_sums_to_the_reference_flux_and_is_non_negative(n_theta):
    g7, g15, _ = _inputs(n_theta)
    F, F_run = g7[f"F_nu_{n_theta}"][-1], g15[f"F_last_{n_theta}"]
    C = g15[f"C_{n_theta}"]
    ok = np.isfinite(F) & (F != 0)
    assert ok.sum() == 198 and np.array_equal(np.isfinite(F_run) & (F_run != 0), ok)
    assert np.max(np.abs(C[:, ok].sum(axis=0) - F_run[ok]) / F_run[ok]) <= 1e-14  # the flux of g15's own run: rounding of a 55-term sum
    assert np.max(np.abs(C[:, ok].sum(axis=0) - F[ok]) / F[ok]) <= 1e-10          # g7's recorded flux (numpy's exp / log): the flux tolerance
    assert (C[:, ok] >= 0).all() and not C[0].any()  # (what the bound of the formation-mean test on the GPU rests on)


@pytest.mark.parametrize("n_theta", [1, 4, 20])
def test_formation_mean_of_the_golden(n_theta):
    g7, g15, _ = _inputs(n_theta)
    x = g15["x_log10"]
    assert np.allclose(x, np.log10(np.arange(1, 57.0)), rtol=1e-15, atol=0)  # (the stored values are used: log10 is not the same in every numpy)
    mean = cref.formation_mean(g15[f"C_{n_theta}"], x)
    assert np.array_equal(mean, g15[f"mean_log10_{n_theta}"], equal_nan=True)
    assert np.isnan(mean[7])  # 0 / 0
    ok = np.isfinite(g7[f"F_nu_{n_theta}"][-1])
    ok[7] = False
    assert (mean[ok] >= x[0]).all() and (mean[ok] <= x[-1]).all()
