"""MultiSGP hyper-parameter objective on the device (sgp_theta_objective with d_out = 2..4): value and analytic gradient of
neg_log_backwardmess_multi (helper_functions/derivative_helper.jl:92-115) against the NumPy restatement, the fresh path
against the re-evaluation path, the inputs it must honour, the state it leaves, the pendulum's inner AdaMax loop and the
refusals."""
import math

import numpy as np
import pytest

from gaussianprocessnode_amd.cubature import SphericalRadialCubature
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass, WishartFast
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel, softplus
from oracle import sgp_oracle as O
from tests import multi_theta_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def problem(n_nodes, M, D, d_out, seed):
    """Gaussian inputs q(x_i) (srcubature points), targets y_i, inducing points spread over the box, a Wishart mean W."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.7, 1.7, (n_nodes, D))
    covs = [np.diag(rng.uniform(0.002, 0.03, D)) for _ in range(n_nodes)]
    Y = np.sin(means @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(n_nodes, d_out))
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)   # spread out in every dimension
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    X, om, Yp = R.expand(Y, means, covs)
    return means, covs, Y, Xu, W, X, om, Yp


def device_for(G, X, om, Yp, Xu, n_nodes, d_out, s2, ell, jitter, family, W, reuse=False, cov_sum=None):
    dev = G.SGPDevice(len(X), Xu.shape[0], Xu.shape[1], d_out, reuse_stats=reuse)
    dev.set_inducing(Xu)
    dev.set_data(X, Yp, weights=om, n_nodes=n_nodes)
    if cov_sum is not None:
        dev.set_output_cov_sum(cov_sum)
    dev.set_kernel(s2, ell, jitter, family=family)
    dev.set_prior_isotropic(50.0)
    dev.set_noise(W, float(np.linalg.slogdet(W)[1]))
    return dev


CASES = [  # d_out, D, M, iso, family, jitter, gaussian q_out
    (2, 2, 48, False, "se", 1e-12, False),
    (3, 1, 20, True, "matern12", 1e-8, True),
    (4, 5, 96, False, "matern32", 1e-12, True),
    (2, 17, 200, False, "matern52", 1e-8, False),
    (3, 2, 48, True, "matern52", 1e-12, False),
    (4, 17, 200, True, "se", 1e-8, True),
    (2, 5, 96, True, "matern12", 1e-12, False),
    (3, 5, 200, False, "matern32", 1e-8, False),
]


@pytest.mark.parametrize("d_out,D,M,iso,family,jitter,gauss_out", CASES)
def test_value_and_gradient_at_a_new_theta(G, d_out, D, M, iso, family, jitter, gauss_out):
    n_nodes = max(3 * M, 150)
    means, covs, Y, Xu, W, X, om, Yp = problem(n_nodes, M, D, d_out, seed=M + 7 * D + d_out)
    n_ell = 1 if iso else D
    ell0 = np.full(n_ell, 0.5 * math.sqrt(D))
    p0 = np.concatenate([[1.05], ell0 * np.linspace(0.9, 1.1, n_ell)])                  # the optimiser's next theta
    cov_sum = 0.01 * n_nodes * np.eye(d_out) if gauss_out else None
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 0.9, ell0, jitter, family, W, cov_sum=cov_sum) as dev:
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        dev.set_kernel(p0[0], p0[1:], jitter, family=family)
        val, grad = dev.theta_objective(want_grad=True, n_ell=n_ell)
        mu1, Sig1, _ = dev.posterior(want_uv=False)

        def f_dev(p):
            dev.set_kernel(p[0], p[1:], jitter, family=family)
            return dev.theta_objective(want_grad=False, n_ell=n_ell)
        g_dev = np.array([(f_dev(p0 + 1e-5 * e) - f_dev(p0 - 1e-5 * e)) / 2e-5 for e in np.eye(1 + n_ell)])
    assert np.array_equal(mu, mu1) and np.array_equal(Sig, Sig1)                          # q(v) untouched
    Rv = Sig + np.outer(mu, mu)
    f = lambda p: R.neg_log_backwardmess_multi(p[0], p[1:], Y, means, covs, Rv, mu, W, Xu, jitter, family)
    ref = f(p0)
    assert math.isclose(val, ref, rel_tol=1e-8), (val, ref)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + n_ell)])
    np.testing.assert_allclose(grad, g_dev, rtol=5e-5, atol=1e-6 * np.abs(g_dev).max())
    np.testing.assert_allclose(grad, g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())
    g_an = R.analytic_grad(p0[0], p0[1:], X, om, Yp, Rv, mu, W, Xu, jitter, family, n_ell=n_ell)
    np.testing.assert_allclose(grad, g_an, rtol=1e-6, atol=1e-9 * np.abs(g_an).max())


@pytest.mark.parametrize("d_out,family", [(2, "se"), (3, "matern32"), (4, "matern52")])
def test_fresh_path_equals_re_evaluation(G, d_out, family):
    n_nodes, M, D = 200, 48, 3
    _, _, _, Xu, W, X, om, Yp = problem(n_nodes, M, D, d_out, seed=11 + d_out)
    ell = np.array([1.6, 1.9, 1.4])
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 0.9, ell, 1e-10, family, W) as dev:
        dev.sweep()
        v_fresh, g_fresh = dev.theta_objective(want_grad=True)
        dev.set_kernel(1.2, ell * 1.1, 1e-10, family=family)
        dev.theta_objective(want_grad=True)                                                  # re-evaluated at another theta
        dev.set_kernel(0.9, ell, 1e-10, family=family)
        v_re, g_re = dev.theta_objective(want_grad=True)                                     # re-evaluated at the sweep's theta
    assert abs(v_re - v_fresh) <= 1e-12 * abs(v_fresh), (v_re, v_fresh)
    np.testing.assert_allclose(g_re, g_fresh, rtol=1e-12, atol=1e-12 * np.abs(g_fresh).max())


def test_new_noise_and_installed_posterior_are_used(G):
    d_out, n_nodes, M, D = 3, 180, 40, 2
    means, covs, Y, Xu, W, X, om, Yp = problem(n_nodes, M, D, d_out, seed=5)
    ell = np.array([0.6, 0.8])
    rng = np.random.default_rng(1)
    A = rng.normal(size=(d_out, d_out))
    W2 = 15.0 * (A @ A.T / d_out + np.eye(d_out))
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 0.8, ell, 1e-10, "se", W) as dev:
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
        dev.set_noise(W2, 0.0)                                                               # mean(q_W) updated after the sweep
        v_fresh, g_fresh = dev.theta_objective(want_grad=True)
        mu_a, Sig_a, Uv_a = dev.posterior()
        # the installed q(v): another mean and factor
        Q = d_out * M
        mu2 = mu + 0.1 * rng.normal(size=Q)
        L2 = np.linalg.cholesky(Sig + np.outer(mu2, mu2) + 0.05 * np.eye(Q))
        dev.set_posterior(mu2, L2.T)
        v_post, g_post = dev.theta_objective(want_grad=True)
        v_post2, g_post2 = dev.theta_objective(want_grad=True)
    assert np.array_equal(mu, mu_a) and np.array_equal(Sig, Sig_a) and np.array_equal(Uv, Uv_a)
    Rv = Sig + np.outer(mu, mu)
    ref = R.neg_log_backwardmess_multi(0.8, ell, Y, means, covs, Rv, mu, W2, Xu, 1e-10, "se")
    assert math.isclose(v_fresh, ref, rel_tol=1e-8), (v_fresh, ref)
    np.testing.assert_allclose(g_fresh, R.analytic_grad(0.8, ell, X, om, Yp, Rv, mu, W2, Xu, 1e-10, "se"), rtol=1e-6)
    Rv2 = L2 @ L2.T
    ref2 = R.neg_log_backwardmess_multi(0.8, ell, Y, means, covs, Rv2, mu2, W2, Xu, 1e-10, "se")
    assert math.isclose(v_post, ref2, rel_tol=1e-8), (v_post, ref2)
    np.testing.assert_allclose(g_post, R.analytic_grad(0.8, ell, X, om, Yp, Rv2, mu2, W2, Xu, 1e-10, "se"), rtol=1e-6)
    assert v_post == v_post2 and np.array_equal(g_post, g_post2)


@pytest.mark.parametrize("reuse", [False, True])
def test_state_after_the_objective(G, reuse):
    d_out, n_nodes, M, D = 2, 160, 48, 2
    _, _, _, Xu, W, X, om, Yp = problem(n_nodes, M, D, d_out, seed=21)
    ell, ell2 = np.array([1.4, 1.2]), np.array([1.5, 1.1])
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 0.9, ell, 1e-10, "matern52", W, reuse=reuse) as dev:
        dev.sweep()
        dev.set_kernel(1.1, ell2, 1e-10, family="matern52")
        r1 = dev.theta_objective(want_grad=True)
        r2 = dev.theta_objective(want_grad=True)
        dev.sweep()
        after = dev.posterior() + (dev.wishart_invscale(), dev.scalars().energy)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1])                                  # bitwise repeatable
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 1.1, ell2, 1e-10, "matern52", W, reuse=reuse) as fresh:
        fresh.sweep()
        ref = fresh.posterior() + (fresh.wishart_invscale(), fresh.scalars().energy)
    for a, b in zip(after, ref):
        assert np.array_equal(a, b)


def pendulum(n_nodes=300, seed=0):
    """A seeded synthetic pendulum: x_t = (angle, angular velocity), q(x_t) Gaussian around a noisy trajectory, targets the
    next state's mean (the GP-SSM transition x_t -> x_t+1)."""
    rng = np.random.default_rng(seed)
    dt, g_l = 0.05, 9.81
    x = np.empty((n_nodes + 1, 2))
    x[0] = [1.2, 0.0]
    for t in range(n_nodes):                                        # semi-implicit Euler: a bounded swing
        a, w = x[t]
        w = w - dt * g_l * math.sin(a)
        x[t + 1] = [a + dt * w, w]
    means = x[:-1] + 0.01 * rng.normal(size=(n_nodes, 2))
    covs = [np.diag(rng.uniform(1e-4, 1e-3, 2)) for _ in range(n_nodes)]
    Y = x[1:] + 0.01 * rng.normal(size=(n_nodes, 2))
    return means, covs, Y


def test_pendulum_inner_loop_matches_the_numpy_gradient(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd import train as TR
    means, covs, Y = pendulum()
    M = 48
    # inducing points on an 8 x 6 grid over the swing (points drawn from the orbit, a curve, leave K_uu near-singular at the
    # reference's jitter 1e-12, and the two loops would then compare rounding, not the gradient)
    Xu = np.stack(np.meshgrid(np.linspace(-1.3, 1.3, 8), np.linspace(-3.7, 3.7, 6), indexing="ij"), -1).reshape(M, 2)
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-12)
    theta0 = O.invsoftplus(np.array([1.0, 0.4, 1.0]))
    q_ins = [MvNormalMeanCovariance(m, P) for m, P in zip(means, covs)]
    q_w = WishartFast(100.0, np.eye(2))
    W = q_w.mean()
    try:
        q_v = MS.sweep(meta, [PointMass(y) for y in Y], q_ins, q_w, PointMass(theta0), MvNormalMeanCovariance(np.zeros(2 * M), 50.0 * np.eye(2 * M)))
        mu, Sig = q_v.mean_cov()
        th_dev = TR.optimize_theta_multi(theta0.copy(), Y, q_ins, q_v, q_w, meta, steps=100, optimizer=TR.AdaMax())
    finally:
        if meta.engine is not None:
            meta.engine.close()
    X, om, Yp = R.expand(Y, means, covs)
    Rv = Sig + np.outer(mu, mu)

    def numpy_grad(th):
        p = softplus(th)
        g = R.analytic_grad(p[0], p[1:], X, om, Yp, Rv, mu, W, Xu, 1e-12, "se")
        return None, g / (1.0 + np.exp(-th))
    th_np = TR.optimize_theta_multi(theta0.copy(), None, None, None, None, None, steps=100, optimizer=TR.AdaMax(), grad_fn=numpy_grad)
    assert not np.allclose(th_np, theta0)
    np.testing.assert_allclose(th_dev, th_np, rtol=1e-6)


def test_refusals(G):
    d_out, n_nodes, M, D = 2, 60, 20, 2
    _, _, _, Xu, W, X, om, Yp = problem(n_nodes, M, D, d_out, seed=2)
    with device_for(G, X, om, Yp, Xu, n_nodes, d_out, 0.9, np.array([1.2, 1.3]), 1e-10, "se", W) as dev:
        with pytest.raises(G.SGPError):
            dev.theta_objective()                                                            # no sweep, no sgp_set_posterior
        dev.set_allreduce(lambda buf, count, stream: None)                                   # single rank: the sum is the identity
        dev.sweep()
        with pytest.raises(G.SGPError):
            dev.theta_objective(want_grad=True)                                              # data-sharded MultiSGP: refused
        dev.set_allreduce(None)
        dev.sweep()
        dev.theta_objective(want_grad=True)
        with pytest.raises(G.SGPError):
            dev.train_begin(X, Yp[:, 0], np.zeros(3), jitter=1e-10)                          # no device-paced MultiSGP training
