"""Host checks of tests/psi_in_ref.py, the reference of the exact-Psi input messages (no GPU): gamma and Gamma against central
differences of the value (symmetric directions for Gamma), the S = 0 identities against the point restatement of the :in closure, the
summed energies against the theta objective, three injected faults, and the natural-gradient driver on the restatement."""
import numpy as np
import pytest

from tests import in_message_grad_ref as GR
from tests import psi_in_ref as R
from tests import psi_theta_ref as TR
from tests.test_psi_theta_host import problem

# the bound tests/test_psi_theta_host.py grants the same comparison (analytic derivative against central differences), element-wise
GRAD_RTOL, GRAD_ATOL = 5e-5, 1e-6


def assert_close(g, n, rtol=GRAD_RTOL, atol=GRAD_ATOL):
    np.testing.assert_allclose(g, n, rtol=rtol, atol=atol * np.abs(n).max())


@pytest.mark.parametrize("d_out", [1, 3])
@pytest.mark.parametrize("cov", ["full", "rank1", "zero", "none"])
def test_derivatives_match_central_differences(cov, d_out):
    p = problem(cov=cov, d_out=d_out)
    gamma, Gamma = R.analytic(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    n_gamma, n_Gamma = R.numeric(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    assert np.array_equal(Gamma, Gamma.transpose(0, 2, 1))
    for t in range(len(gamma)):
        assert_close(gamma[t], n_gamma[t])
        assert_close(Gamma[t], n_Gamma[t])


@pytest.mark.parametrize("fault", ["h_c1", "no_p2", "offdiag_once"])
def test_injected_faults_are_caught(fault):
    p = problem()
    n = R.stacked(*R.numeric(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"]))
    good = R.stacked(*R.analytic(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"]))
    bad = R.stacked(*R.analytic(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"], fault=fault))
    assert_close(good, n)
    with pytest.raises(AssertionError):
        assert_close(bad, n)


@pytest.mark.parametrize("cov", ["zero", "none"])
def test_zero_covariance_is_the_point_closure(cov):
    """U = -logpdf - 1/2 tr(W) sigma2, gamma = -grad, Gamma = -1/2 hess of sgp_in_message_grad's restatement at the point m_t"""
    p = problem(cov=cov)
    mean, S, Y, Rv, v, W, Xu = p["args"]
    T, D = mean.shape
    M = len(Xu)
    c = dict(M=M, D=D, W=W, ell=p["ell"], sigma2=p["sigma2"], jitter=p["jitter"], Xu=Xu, X=mean, Y=Y, family="se", mu_v=v,
             Sigma_v=Rv - np.outer(v, v), start=np.arange(T + 1))
    lp, grad, hess = GR.evaluate(c)
    U, gamma, Gamma = R.evaluate(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    scale = np.abs(lp).max()
    np.testing.assert_allclose(U, -lp - 0.5 * np.trace(W) * p["sigma2"], rtol=0, atol=1e-11 * scale)
    np.testing.assert_allclose(gamma, -grad, rtol=1e-9, atol=1e-11 * np.abs(grad).max())
    np.testing.assert_allclose(Gamma, -0.5 * hess, rtol=1e-9, atol=1e-11 * np.abs(hess).max())


@pytest.mark.parametrize("cov", ["full", "none"])
def test_energies_sum_to_the_theta_objective(cov):
    p = problem(cov=cov)
    W = p["args"][5]
    T = len(p["args"][0])
    U = R.energy(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    f = TR.objective(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    assert abs(U.sum() + 0.5 * np.trace(W) * p["sigma2"] * T - f) <= 1e-12 * abs(f)


# ---- the natural-gradient driver (multisgp.natural_gradient_in) on the restatement ----
def _driver_case(p, left_var, seed=0):
    from gaussianprocessnode_amd.multisgp import natural_gradient_in
    mean, S, Y, Rv, v, W, Xu = p["args"]
    T, D = mean.shape
    rng = np.random.default_rng(seed)
    left_m = mean + 0.3 * rng.normal(size=mean.shape)
    left_S = np.tile(left_var * np.eye(D), (T, 1, 1))
    calls = []

    def evaluate(idx, m, SS):
        calls.append(len(idx))
        return R.evaluate(p["sigma2"], p["ell"], m, SS, Y[idx], Rv, v, W, Xu, p["jitter"])
    return natural_gradient_in, evaluate, left_m, left_S, calls


def test_driver_never_raises_a_node_s_free_energy():
    p = problem(cov="full")
    step, evaluate, left_m, left_S, calls = _driver_case(p, 0.5)
    m, S, rec = step(evaluate, left_m, left_S, p["args"][0], p["args"][1], iterations=3, halvings=8)
    assert np.all(rec["after"] <= rec["before"]) and np.any(rec["after"] < rec["before"])
    for t in range(len(m)):
        np.linalg.cholesky(S[t])
    assert calls[0] == len(m)


def test_driver_halves_where_the_full_step_is_indefinite():
    """wide left messages (precision 1/50) and targets that put every node on a maximum of its energy, where U is concave in the
    input: Sl^-1 + 2 Gamma is indefinite, so the full step has no Gaussian and rho must come down"""
    p = problem(cov="full", T=4)
    mean, S, Y, Rv, v, W, Xu = p["args"]
    mean = Xu[:4] + 0.05                                                  # on inducing inputs
    S = np.tile(0.02 * np.eye(3), (4, 1, 1))
    Y = -8.0 * np.sign((np.asarray(v).reshape(2, -1)[:, :4]).T)           # s_t[t] < 0: -s_t' Psi1_t peaks at z_t
    p["args"] = (mean, S, Y, Rv, v, W, Xu)
    step, evaluate, left_m, left_S, calls = _driver_case(p, 50.0)
    _, _, Gamma = evaluate(np.arange(4), mean, S)
    full = np.linalg.inv(left_S) + 2.0 * Gamma
    assert all(np.linalg.eigvalsh(full[t])[0] < 0 for t in range(4)), "the case must make the full step indefinite"
    m, S2, rec = step(evaluate, left_m, left_S, mean, S, iterations=1, halvings=12)
    assert np.all(rec["halved"] >= 1) and np.all(rec["rho"] < 1.0)
    assert np.all(rec["after"] <= rec["before"])
    for t in range(4):
        np.linalg.cholesky(S2[t])


def test_driver_keeps_a_node_that_exhausts_its_halvings():
    p = problem(cov="full", T=4)
    mean, S, Y, Rv, v, W, Xu = p["args"]
    mean = Xu[:4] + 0.05
    S = np.tile(0.02 * np.eye(3), (4, 1, 1))
    Y = -8.0 * np.sign((np.asarray(v).reshape(2, -1)[:, :4]).T)
    p["args"] = (mean, S, Y, Rv, v, W, Xu)
    step, evaluate, left_m, left_S, calls = _driver_case(p, 50.0)
    m, S2, rec = step(evaluate, left_m, left_S, mean, S, iterations=1, halvings=0)
    assert np.array_equal(m, mean) and np.array_equal(S2, S) and np.array_equal(rec["after"], rec["before"])
    assert np.all(rec["rho"] == 0.0)
