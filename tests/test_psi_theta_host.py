"""Host checks of tests/psi_theta_ref.py, the reference of the exact-Psi kernel-parameter objective (no GPU): the analytic gradient
against central differences of the value, the S = 0 limit against the cubature-point restatement, d_out = 1 against the UniSGP
objective, a shared lengthscale against the sum over the dimensions, and three injected faults."""
import numpy as np
import pytest

from tests import multi_theta_ref as MR
from tests import psi_theta_ref as R
from tests import theta_descend_ref as DR

# the bound tests/test_gpu_multi_theta.py grants the same comparison (gradient against central differences), element-wise
GRAD_RTOL, GRAD_ATOL = 5e-5, 1e-6


def problem(M=7, D=3, T=5, d_out=2, cov="full", seed=3):
    rng = np.random.default_rng(seed)
    Xu = rng.uniform(-1.5, 1.5, (M, D))
    mean = rng.uniform(-1.5, 1.5, (T, D))
    if cov == "full":
        A = rng.normal(size=(T, D, D)) * 0.3
        S = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(D)
    elif cov == "zero":
        S = np.zeros((T, D, D))
    elif cov == "rank1":
        a = rng.normal(size=(T, D)) * 0.4
        S = a[:, :, None] * a[:, None, :]
    else:
        S = None
    Y = rng.normal(size=(T, d_out))
    v = rng.normal(size=d_out * M) * 0.5
    L = rng.normal(size=(d_out * M, d_out * M)) * 0.1
    Rv = L @ L.T + np.outer(v, v)
    A = rng.normal(size=(d_out, d_out))
    W = 3.0 * (A @ A.T / d_out + np.eye(d_out))
    sigma2, ell = 1.3, rng.uniform(0.7, 1.4, D)
    return dict(sigma2=sigma2, ell=ell, args=(mean, S, Y, Rv, v, W, Xu), jitter=1e-8)


def assert_grad_close(g, n, rtol=GRAD_RTOL, atol=GRAD_ATOL):
    np.testing.assert_allclose(g, n, rtol=rtol, atol=atol * np.abs(n).max())


@pytest.mark.parametrize("cov", ["full", "zero", "rank1", "none"])
def test_gradient_matches_central_differences(cov):
    p = problem(cov=cov)
    g = R.analytic_grad(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    n = R.numeric_grad(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    assert_grad_close(g, n)


def test_zero_covariance_is_the_point_objective():
    p = problem(cov="zero")
    mean, S, Y, Rv, v, W, Xu = p["args"]
    om = np.ones(len(mean))
    f = R.objective(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    g = R.analytic_grad(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    f0 = MR.batched_objective(p["sigma2"], p["ell"], mean, om, Y, Rv, v, W, Xu, jitter=p["jitter"])
    g0 = MR.analytic_grad(p["sigma2"], p["ell"], mean, om, Y, Rv, v, W, Xu, jitter=p["jitter"])
    assert abs(f - f0) <= 1e-12 * abs(f0)
    assert_grad_close(g, g0, rtol=1e-10, atol=1e-13)


def test_one_output_is_the_unisgp_objective():
    p = problem(d_out=1, cov="zero")
    mean, S, Y, Rv, v, W, Xu = p["args"]
    f = R.objective(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    f0 = DR.uni_objective("se", p["sigma2"], p["ell"], Xu, mean, np.ones(len(mean)), Y[:, 0], v, Rv, float(W[0, 0]), p["jitter"])
    assert abs(f - f0) <= 1e-12 * abs(f0)


def test_shared_lengthscale_is_the_sum_over_dimensions():
    p = problem()
    ell = np.full(3, 0.9)
    g = R.analytic_grad(p["sigma2"], ell, *p["args"], jitter=p["jitter"])
    g1 = R.analytic_grad(p["sigma2"], ell[:1], *p["args"], jitter=p["jitter"], n_ell=1)
    assert g1.shape == (2,)
    assert g1[0] == g[0] and abs(g1[1] - g[1:].sum()) <= 1e-14 * np.abs(g[1:]).sum()
    n1 = R.numeric_grad(p["sigma2"], ell[:1], *p["args"], jitter=p["jitter"], n_ell=1)
    assert_grad_close(g1, n1)


@pytest.mark.parametrize("fault", ["no_det", "no_dz", "h_c1"])
def test_injected_faults_are_caught(fault):
    p = problem()
    n = R.numeric_grad(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"])
    bad = R.analytic_grad(p["sigma2"], p["ell"], *p["args"], jitter=p["jitter"], fault=fault)
    with pytest.raises(AssertionError):
        assert_grad_close(bad, n)


def test_descent_restatement_moves_theta_and_lowers_the_value():
    p = problem(T=4, M=5)
    th0 = np.log(np.expm1(np.concatenate([[p["sigma2"]], p["ell"]])))
    th, vals = R.descend(th0, 3, 5, *p["args"], p["jitter"], eta=0.01)
    assert np.all(np.isfinite(th)) and vals[-1] < vals[0]
