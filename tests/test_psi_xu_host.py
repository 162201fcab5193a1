"""The exact-Psi theta objective's gradient in the inducing inputs without a GPU: the NumPy restatement (tests/psi_xu_ref.py) against
central differences of `psi_theta_ref.objective` in Xu, against the point route's restatement at S = 0, three injected faults that
the check must catch, and the entry point's boundary (declared, exported, bound; argument order, shapes and layout through
`SGPDevice.theta_objective_psi_xu`; the keywords of `train.optimize_inducing`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import psi_theta_ref as TR
from tests import psi_xu_ref as XR
from tests.xu_grad_ref import analytic_grad_xu as point_grad_xu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 1e-6
FD_STEP, FD_BOUND = 1e-6, 1e-7                                       # central-difference step, and the bound as a share of max |grad|
SIGMA2 = 0.9

# (d_out, M, D, T, shared lengthscale, cov): full, rank-1, zero and absent covariances; d_out 1 and 3; shared and ARD; D = 1 and 4
CASES = [(2, 7, 3, 9, False, "full"), (1, 5, 2, 6, False, "null"), (3, 6, 4, 5, False, "rank1"), (3, 6, 4, 5, True, "zero"),
         (1, 6, 1, 7, True, "full"), (3, 5, 1, 6, False, "rank1"), (1, 6, 4, 5, True, "full")]


def problem(d_out, M, D, T, shared, cov, seed):
    """Inducing inputs spread over the box (a jittered grid for D = 1) at a lengthscale that keeps K_uu well conditioned, Gaussian
    inputs in the box, a q(v) and a W."""
    rng = np.random.default_rng(seed)
    if D == 1:
        grid = np.linspace(-1.6, 1.6, M)
        Xu = (grid + rng.uniform(-0.1, 0.1, M) * (grid[1] - grid[0]))[:, None]
        ell = np.array([0.7 * (grid[1] - grid[0])])
    else:
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
        scale = 0.45 * np.sqrt(D)
        ell = np.full(1, scale) if shared else scale * np.linspace(0.9, 1.1, D)
    mean = rng.uniform(-1.7, 1.7, (T, D))
    if cov == "full":
        A = rng.normal(size=(T, D, D)) * 0.3 * ell.mean() / np.sqrt(D)
        S = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    elif cov == "rank1":
        a = rng.normal(size=(T, D, 1)) * 0.3 * ell.mean()
        S = a @ a.transpose(0, 2, 1)
    elif cov == "zero":
        S = np.zeros((T, D, D))
    else:
        S = None
    Y = np.sin(mean @ rng.normal(size=(D, d_out)) / np.sqrt(D) * 2.0) + 0.05 * rng.normal(size=(T, d_out))
    Q = d_out * M
    v = rng.normal(size=Q)
    L = 0.3 * rng.normal(size=(Q, Q))
    Rv = L @ L.T + 0.1 * np.eye(Q) + np.outer(v, v)
    A = rng.normal(size=(d_out, d_out))
    W = 2.0 * (A @ A.T / d_out + np.eye(d_out))
    return (SIGMA2, ell, mean, S, Y, Rv, v, W, Xu, JITTER)


@pytest.fixture(scope="module")
def cases():
    """Each case: the inputs and the central differences of psi_theta_ref.objective in Xu, computed once."""
    out = {}
    for k, spec in enumerate(CASES):
        args = problem(*spec, seed=900 + k)
        out[spec] = args, XR.numeric_grad_xu(*args, h=FD_STEP)
    return out


@pytest.mark.parametrize("spec", CASES, ids=str)
def test_restatement_matches_central_differences(cases, spec):
    args, fd = cases[spec]
    g = XR.analytic_grad_xu(*args)
    err = np.abs(g - fd).max() / np.abs(g).max()
    print(f"psi_xu restatement {spec}: |analytic - central differences| / max|grad| = {err:.2e} (bound {FD_BOUND:g})")
    assert g.shape == args[8].shape
    assert err <= FD_BOUND, err


@pytest.mark.parametrize("fault", ["no_column", "uu_halved", "dz_sign"])
@pytest.mark.parametrize("spec", CASES, ids=str)
def test_injected_faults_are_caught(cases, spec, fault):
    args, fd = cases[spec]
    g = XR.analytic_grad_xu(*args, fault=fault)
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print(f"psi_xu fault {fault} {spec}: {err:.2e}")
    assert err > 10 * FD_BOUND, err


@pytest.mark.parametrize("cov", ["zero", "null"])
@pytest.mark.parametrize("spec", [(3, 6, 4, 5, False), (1, 6, 1, 7, True), (2, 7, 3, 9, True)], ids=str)
def test_zero_covariance_is_the_point_gradient_on_the_means(spec, cov):
    s2, ell, mean, S, Y, Rv, v, W, Xu, jit = problem(*spec, cov, seed=77)
    g = XR.analytic_grad_xu(s2, ell, mean, S, Y, Rv, v, W, Xu, jit)
    g0 = point_grad_xu(s2, ell, mean, np.ones(len(mean)), Y, Rv, v, W, Xu, jit, "se")
    print(f"psi_xu S = 0 ({cov}) {spec}: max rel {np.max(np.abs(g - g0) / np.abs(g0)):.2e}")
    np.testing.assert_allclose(g, g0, rtol=1e-10)


def test_the_entry_point_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    name = "sgp_theta_objective_psi_xu"
    assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
    fn = getattr(_lib.load(), name)
    assert len(fn.argtypes) == 9 and fn.restype is C.c_int
    for kernel in (b"k_psi_xu_prep", b"k_psi1_xu_accumulate", b"k_psi2_xu_accumulate", b"k_psi_xu_finish"):
        assert kernel in blob, kernel
    jl = open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    assert "sgp_theta_objective_psi_xu" in jl and re.search(r"export[^\n]*\btheta_objective_psi_xu\b", jl)
    from gaussianprocessnode_amd import SGPDevice
    assert callable(SGPDevice.theta_objective_psi_xu)


def test_the_python_method_passes_order_shapes_and_layout():
    """`theta_objective_psi_xu` over a stand-in library: the argument order of the header, means (T, D) row-major = D x T
    column-major, targets T x d_out column-major, 1 + n_ell gradient entries, an (M, D) C-order grad_xu (entry m * D + d is inducing
    point m, dimension d -- `set_inducing`'s layout), a NULL cov for None and a NULL grad without want_grad."""
    from gaussianprocessnode_amd import SGPDevice
    M, D, T, d_out, n_ell = 3, 2, 4, 2, 2
    seen = {}

    class Lib:
        @staticmethod
        def sgp_theta_objective_psi_xu(h, mean, cov, y_mean, n_nodes, value, grad, grad_xu, info):
            seen.update(grad_null=not grad, cov_null=not cov, n=n_nodes, mean=[mean[i] for i in range(T * D)],
                        y=[y_mean[i] for i in range(T * d_out)], cov0=None if not cov else [cov[i] for i in range(D * D)])
            value[0] = 1.5
            if grad:
                for i in range(1 + n_ell):
                    grad[i] = 10.0 + i
            for e in range(M * D):
                grad_xu[e] = float(e)
            info[0] = info[1] = 0
            return 0

    dev = object.__new__(SGPDevice)
    dev._lib, dev._h, dev.M, dev.D, dev.d_out = Lib, C.c_void_p(), M, D, d_out
    mean = np.arange(T * D, dtype=float).reshape(T, D)
    Y = 100.0 + np.arange(T * d_out, dtype=float).reshape(T, d_out)
    S = np.tile(np.array([[2.0, 0.5], [0.5, 3.0]]), (T, 1, 1))
    with pytest.raises(ValueError):
        dev.theta_objective_psi_xu(mean, None, Y, want_grad=True)             # no set_kernel yet: the gradient's length is unknown
    dev._n_ell = n_ell
    val, gxu = dev.theta_objective_psi_xu(mean, None, Y)
    assert seen["grad_null"] and seen["cov_null"] and seen["n"] == T and val == 1.5 and gxu.shape == (M, D)
    assert seen["mean"] == list(mean.ravel()) and seen["y"] == list(Y.T.ravel())
    assert np.array_equal(gxu, np.arange(M * D, dtype=float).reshape(M, D))
    val, g, gxu = dev.theta_objective_psi_xu(mean, S, Y, want_grad=True)
    assert not seen["grad_null"] and seen["cov0"] == [2.0, 0.5, 0.5, 3.0]
    assert np.array_equal(g, [10.0, 11.0, 12.0]) and gxu[2, 1] == 5.0


class RestatementEngine:
    """What `optimize_inducing(psi="exact")` drives, on the restatement; it refuses after `set_inducing` until `set_posterior`."""
    kernel_family = "se"

    def __init__(self, W):
        self.W, self.qv, self.calls = W, None, []

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.s2, self.ell, self.jitter = sigma2, np.asarray(ell, dtype=np.float64), jitter
        self.calls.append("kernel")

    def set_inducing(self, Xu):
        self.Xu, self.qv = np.array(Xu, dtype=np.float64), None
        self.calls.append("inducing")

    def set_posterior(self, mu_v, Uv):
        self.qv = (np.asarray(mu_v), np.asarray(Uv).T @ np.asarray(Uv))
        self.calls.append("posterior")

    def theta_objective_xu(self, want_grad=False):
        raise AssertionError("the exact route must not call the point route")

    def theta_objective_psi_xu(self, mean, cov, y_mean, want_grad=False):
        if self.qv is None:
            raise RuntimeError("needs a finished sweep or sgp_set_posterior (q(v))")
        self.calls.append("objective")
        v, Rv = self.qv
        a = (self.s2, self.ell, mean, cov, y_mean, Rv, v, self.W, self.Xu, self.jitter)
        return TR.objective(*a), TR.analytic_grad(*a, n_ell=len(self.ell)), XR.analytic_grad_xu(*a)


@pytest.mark.parametrize("learn_theta", [True, False])
def test_optimize_inducing_exact_is_adamax_on_the_joint_vector(learn_theta):
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.meta import softplus
    from oracle import sgp_oracle as O
    d_out, M, D, T = 2, 7, 3, 9
    s2, ell, mean, S, Y, Rv, v, W, Xu, jit = problem(d_out, M, D, T, False, "full", seed=5)
    Uv = np.linalg.cholesky(Rv).T
    theta0 = O.invsoftplus(np.concatenate([[s2], ell]))
    eng = RestatementEngine(W)
    th, Z, vals = train.optimize_inducing(theta0, Xu, eng, q_v=(v, Uv), steps=6, learn_theta=learn_theta, jitter=jit, psi="exact",
                                          inputs=(mean, S, Y))
    assert eng.calls[:4] == ["kernel", "inducing", "posterior", "objective"] and len(eng.calls) == 4 * 6
    nt = theta0.size if learn_theta else 0

    def grad(x):
        t = x[:nt] if learn_theta else theta0
        p = softplus(t)
        a = (p[0], p[1:], mean, S, Y, Rv, v, W, x[nt:].reshape(M, D), jit)
        g = TR.analytic_grad(*a, n_ell=D) / (1.0 + np.exp(-t))
        return TR.objective(*a), np.concatenate([g[:nt], XR.analytic_grad_xu(*a).ravel()])
    x, values = XR.adamax(np.concatenate([theta0[:nt], Xu.ravel()]), grad, 6)
    np.testing.assert_allclose(Z, x[nt:].reshape(M, D), rtol=1e-12)
    np.testing.assert_allclose(th, x[:nt] if learn_theta else theta0, rtol=1e-12)
    np.testing.assert_allclose(vals, values, rtol=1e-12)


def test_optimize_inducing_exact_refuses_what_it_cannot_do():
    from gaussianprocessnode_amd import train
    s2, ell, mean, S, Y, Rv, v, W, Xu, jit = problem(1, 5, 2, 6, False, "null", seed=6)
    eng = RestatementEngine(W)
    q_v = (v, np.linalg.cholesky(Rv).T)
    with pytest.raises(ValueError):
        train.optimize_inducing(np.zeros(3), Xu, eng, q_v=q_v, steps=1, psi="exact")               # no inputs
    with pytest.raises(ValueError):
        train.optimize_inducing(np.zeros(3), Xu, eng, q_v=q_v, steps=1, psi="closed-form", inputs=(mean, S, Y))
    eng.kernel_family = "matern32"
    with pytest.raises(ValueError):
        train.optimize_inducing(np.zeros(3), Xu, eng, q_v=q_v, steps=1, psi="exact", inputs=(mean, S, Y))
    assert eng.calls == []
