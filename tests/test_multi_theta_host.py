"""MultiSGP hyper-parameter objective on the host (no GPU): the summed-statistics form against the literal per-node loop of
neg_log_backwardmess_multi (helper_functions/derivative_helper.jl:92-106), the analytic gradient against central
differences, and the argument handling and softplus chain rule of `multisgp.grad_llh_multi` with a fake engine."""
import numpy as np
import pytest

from gaussianprocessnode_amd import device as DV
from gaussianprocessnode_amd import multisgp as MS
from gaussianprocessnode_amd import train as TR
from gaussianprocessnode_amd.cubature import SphericalRadialCubature
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
from gaussianprocessnode_amd.meta import MaternARDKernel, MultiSGPMeta, SEARDKernel, softplus
from tests import multi_theta_ref as R


def problem(n_nodes, M, D, d_out, seed):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.5, 1.5, (n_nodes, D))
    covs = [np.diag(rng.uniform(0.005, 0.05, D)) for _ in range(n_nodes)]
    Y = np.sin(means @ rng.normal(size=(D, d_out))) + 0.05 * rng.normal(size=(n_nodes, d_out))
    Xu = np.stack([rng.permutation(np.linspace(-1.5, 1.5, M)) for _ in range(D)], axis=1)   # spread out in every dimension
    A = rng.normal(size=(d_out, d_out))
    W = A @ A.T + d_out * np.eye(d_out)
    Q = d_out * M
    mu = rng.normal(size=Q)
    L = rng.normal(size=(Q, Q)) / Q
    Sigma = L @ L.T + 0.01 * np.eye(Q)
    return means, covs, Y, Xu, W, mu, Sigma + np.outer(mu, mu), Sigma


@pytest.mark.parametrize("family", ["se", "matern12", "matern32", "matern52"])
@pytest.mark.parametrize("d_out,D,M", [(2, 2, 12), (3, 1, 9), (4, 3, 15)])
def test_batched_form_equals_the_literal_loop(family, d_out, D, M):
    means, covs, Y, Xu, W, mu, Rv, _ = problem(17, M, D, d_out, seed=M + D)
    s2, ell = 0.9, np.linspace(0.5, 0.8, D)         # K_uu well conditioned: the check is the algebra, not the rounding
    lit = R.neg_log_backwardmess_multi(s2, ell, Y, means, covs, Rv, mu, W, Xu, 1e-8, family)
    X, om, Yp = R.expand(Y, means, covs)
    bat = R.batched_objective(s2, ell, X, om, Yp, Rv, mu, W, Xu, 1e-8, family)
    assert abs(bat - lit) <= 1e-12 * abs(lit), (bat, lit)


@pytest.mark.parametrize("family", ["se", "matern12", "matern32", "matern52"])
@pytest.mark.parametrize("iso", [True, False])
@pytest.mark.parametrize("d_out,D,M", [(2, 2, 10), (3, 4, 14)])
def test_analytic_gradient_matches_central_differences(family, iso, d_out, D, M):
    means, covs, Y, Xu, W, mu, Rv, _ = problem(11, M, D, d_out, seed=7 * M + D)
    n_ell = 1 if iso else D
    p0 = np.concatenate([[1.1], np.linspace(0.9, 1.4, n_ell)])
    X, om, Yp = R.expand(Y, means, covs)
    g = R.analytic_grad(p0[0], p0[1:], X, om, Yp, Rv, mu, W, Xu, 1e-8, family, n_ell=n_ell)
    f = lambda p: R.neg_log_backwardmess_multi(p[0], p[1:], Y, means, covs, Rv, mu, W, Xu, 1e-8, family)
    h = 1e-6
    g_fd = np.array([(f(p0 + h * e) - f(p0 - h * e)) / (2 * h) for e in np.eye(1 + n_ell)])
    np.testing.assert_allclose(g, g_fd, rtol=5e-5, atol=1e-6 * np.abs(g_fd).max())


def test_multi_objective_reduces_to_the_unisgp_objective():
    """d_out = 1, W = w: the formula is UniSGP's neg_log_backwardmess_fast (derivative_helper.jl:23-39) term by term."""
    from oracle import sgp_oracle as O
    means, covs, Y, Xu, W, mu, Rv, Sigma = problem(9, 8, 2, 1, seed=3)
    w = float(W[0, 0])
    X = means
    y = Y[:, 0]
    Uv = np.linalg.cholesky(Rv).T
    uni = O.theta_objective(Xu, X, y, 0.8, np.array([1.1, 0.9]), mu, Uv, w, jitter=1e-8)
    multi = R.batched_objective(0.8, [1.1, 0.9], X, np.ones(len(X)), Y, Rv, mu, W, Xu, 1e-8, "se")
    assert abs(multi - uni) <= 1e-10 * abs(uni), (multi, uni)


# ------------------------------------------------------------------------------------------------
# grad_llh_multi with a fake engine: what it loads, the chain rule, the argument checks
class FakeEngine:
    def __init__(self, d_out, grad):
        self.n_max, self.d_out, self.reuse_stats = 10 ** 6, d_out, False
        self.grad = np.asarray(grad, dtype=np.float64)
        self.calls = []

    def set_data(self, X, y, y_var=None, weights=None, n_nodes=None):
        self.calls.append(("set_data", np.array(X), np.array(y), None if weights is None else np.array(weights), n_nodes))

    def set_noise(self, W, E_log_w=None):
        self.calls.append(("set_noise", np.array(W)))

    def set_posterior(self, mu_v, Uv):
        self.calls.append(("set_posterior", np.array(mu_v), np.array(Uv)))

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.calls.append(("set_kernel", sigma2, np.array(ell), jitter, family))

    def theta_objective(self, want_grad=False, n_ell=None):
        self.calls.append(("theta_objective", want_grad, n_ell))
        return 1.25, self.grad.copy()


@pytest.fixture
def host_potrf(monkeypatch):
    monkeypatch.setattr(DV, "potrf", lambda A, device=0: np.linalg.cholesky(np.asarray(A)))


def fake_meta(d_out, kernel, grad, M=6, D=2):
    Xu = np.random.default_rng(0).uniform(-1, 1, (M, D))
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, kernel, jitter=1e-12)
    meta.engine = FakeEngine(d_out, grad)
    return meta


def qv_of(d_out, M, seed=0):
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(d_out * M, d_out * M)) / M
    return MvNormalMeanCovariance(rng.normal(size=d_out * M), L @ L.T + 0.1 * np.eye(d_out * M))


@pytest.mark.parametrize("softplus_params", [True, False])
def test_grad_llh_multi_loads_the_inputs_and_applies_the_chain_rule(host_potrf, softplus_params):
    d_out, M, D = 2, 6, 2
    theta = np.array([0.3, -0.2, 0.7])
    meta = fake_meta(d_out, SEARDKernel(softplus_params=softplus_params), [2.0, -1.0, 0.5], M, D)
    q_ins = [MvNormalMeanCovariance(np.array([0.1, 0.2]), 0.01 * np.eye(2)), PointMass(np.array([-0.3, 0.4]))]
    Y = np.array([[1.0, 2.0], [3.0, 4.0]])
    q_v = qv_of(d_out, M)
    W = np.array([[3.0, 0.5], [0.5, 2.0]])
    val, g = MS.grad_llh_multi(theta, Y, q_ins, q_v, PointMass(W), meta)
    assert val == 1.25
    want = np.array([2.0, -1.0, 0.5]) * (1.0 / (1.0 + np.exp(-theta)) if softplus_params else 1.0)
    np.testing.assert_allclose(g, want, rtol=1e-15)
    kinds = [c[0] for c in meta.engine.calls]
    assert kinds == ["set_data", "set_noise", "set_posterior", "set_kernel", "theta_objective"]
    _, X, y, wts, n_nodes = meta.engine.calls[0]
    assert X.shape == (5 + 1, D) and n_nodes == 2                       # 2 D + 1 srcubature points + one point mass
    np.testing.assert_array_equal(y[:5], np.repeat(Y[:1], 5, axis=0))
    np.testing.assert_array_equal(y[5], Y[1])
    assert abs(wts[:5].sum() - 1.0) < 1e-15 and wts[5] == 1.0
    np.testing.assert_array_equal(meta.engine.calls[1][1], W)
    mu, Sig = q_v.mean_cov()
    Uv = meta.engine.calls[2][2]
    np.testing.assert_allclose(Uv.T @ Uv, Sig + np.outer(mu, mu), rtol=1e-12)
    _, s2, ell, jit, fam = meta.engine.calls[3]
    p = softplus(theta) if softplus_params else theta
    assert s2 == p[0] and np.array_equal(ell, p[1:]) and jit == 1e-12 and fam == "se"
    assert meta.engine.calls[4] == ("theta_objective", True, 2)


def test_grad_llh_multi_family_and_isotropic_lengthscale(host_potrf):
    meta = fake_meta(3, MaternARDKernel(1.5), [1.0, 2.0], M=4, D=2)
    val, g = MS.grad_llh_multi([0.9, 1.2], np.ones((1, 3)), [PointMass(np.zeros(2))], qv_of(3, 4), PointMass(np.eye(3)), meta)
    _, s2, ell, _, fam = meta.engine.calls[3]
    assert fam == "matern32" and s2 == 0.9 and np.array_equal(ell, [1.2])
    assert meta.engine.calls[4] == ("theta_objective", True, 1)
    np.testing.assert_array_equal(g, [1.0, 2.0])


def test_grad_llh_multi_argument_checks(host_potrf):
    q_ins = [MvNormalMeanCovariance(np.zeros(2), 0.01 * np.eye(2))]
    meta = fake_meta(2, SEARDKernel(), [0.0, 0.0, 0.0])
    W2 = PointMass(np.eye(2))
    with pytest.raises(ValueError, match="d_out"):
        MS.grad_llh_multi([1.0, 1.0, 1.0], np.ones((1, 1)), q_ins, qv_of(1, 6), PointMass(np.eye(1)), meta)
    with pytest.raises(ValueError, match="y_data"):
        MS.grad_llh_multi([1.0, 1.0, 1.0], np.ones((2, 2)), q_ins, qv_of(2, 6), W2, meta)
    with pytest.raises(ValueError, match="y_data"):
        MS.grad_llh_multi([1.0, 1.0, 1.0], np.ones((1, 3)), q_ins, qv_of(2, 6), W2, meta)
    with pytest.raises(ValueError, match="q_v"):
        MS.grad_llh_multi([1.0, 1.0, 1.0], np.ones((1, 2)), q_ins, qv_of(2, 5), W2, meta)
    with pytest.raises(ValueError, match="theta"):
        MS.grad_llh_multi([1.0, 1.0, 1.0, 1.0], np.ones((1, 2)), q_ins, qv_of(2, 6), W2, meta)
    meta.method = None
    with pytest.raises(ValueError, match="method"):
        MS.grad_llh_multi([1.0, 1.0, 1.0], np.ones((1, 2)), q_ins, qv_of(2, 6), W2, meta)


def test_optimize_theta_multi_runs_adamax_on_the_given_gradient():
    """With grad_fn the loop is AdaMax on that gradient: theta moves in place, step by step as Flux.Optimise.update! does."""
    target = np.array([0.5, 1.5, -0.5])
    gfn = lambda th: (float(np.sum((th - target) ** 2)), 2.0 * (th - target))
    theta = np.zeros(3)
    out = TR.optimize_theta_multi(theta, None, None, None, None, None, steps=100, optimizer=TR.AdaMax(eta=0.05), grad_fn=gfn)
    assert out is theta
    ref = np.zeros(3)
    opt = TR.AdaMax(eta=0.05)
    for _ in range(100):
        opt.update(ref, gfn(ref)[1])
    np.testing.assert_array_equal(theta, ref)
    assert np.linalg.norm(theta - target) < np.linalg.norm(target)
