"""The theta objective's gradient in the inducing inputs without a GPU: the NumPy restatement (tests/xu_grad_ref.py) against
central differences of `multi_theta_ref.batched_objective`, three injected faults that the check must catch, `train.
optimize_inducing` against a plain NumPy AdaMax loop, and the entry point's boundary (declared, exported, bound; argument shapes
and layout through `SGPDevice.theta_objective_xu`)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import multi_theta_ref as R
from tests.xu_grad_ref import analytic_grad_xu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["se", "matern12", "matern32", "matern52"]
SHAPES = [(1, 1, 5, 30), (2, 3, 7, 40), (3, 9, 6, 25)]            # d_out, D, M, N
JITTER = 1e-6
FD_STEP, FD_BOUND = 1e-5, 5e-5                                       # the project's finite-difference step and bound (of max |grad|)


def problem(d_out, D, M, N, seed):
    """Weighted points, inducing inputs that keep K_uu well conditioned (D = 1: a jittered grid with spacing >= ell / 2; else
    spread over the box at ell = sqrt(D) / 2), a q(v) and a W.  No point coincides with an inducing input."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    om = rng.uniform(0.2, 1.5, N)
    Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(N, d_out))
    if D == 1:
        grid = np.linspace(-1.6, 1.6, M)
        Xu = (grid + rng.uniform(-0.1, 0.1, M) * (grid[1] - grid[0]))[:, None]
        ell = np.array([0.9])
        assert np.diff(Xu[:, 0]).min() >= ell[0] / 2
    else:
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
        ell = 0.5 * math.sqrt(D) * np.linspace(0.9, 1.1, D)
    Q = d_out * M
    v = rng.normal(size=Q)
    L = 0.3 * rng.normal(size=(Q, Q))
    Rv = L @ L.T + 0.1 * np.eye(Q) + np.outer(v, v)
    A = rng.normal(size=(d_out, d_out))
    W = 2.0 * (A @ A.T / d_out + np.eye(d_out))
    return X, om, Y, Xu, ell, Rv, v, W


def central_differences(f, Xu, h=FD_STEP):
    g = np.empty_like(Xu)
    for idx in np.ndindex(*Xu.shape):
        e = np.zeros_like(Xu)
        e[idx] = h
        g[idx] = (f(Xu + e) - f(Xu - e)) / (2 * h)
    return g


@pytest.fixture(scope="module")
def cases():
    """Each (family, shape): the inputs and the central differences of batched_objective, computed once."""
    out = {}
    for fam in FAMILIES:
        for shp in SHAPES:
            X, om, Y, Xu, ell, Rv, v, W = problem(*shp, seed=sum(shp) + len(fam))
            s2 = 1.1
            fd = central_differences(lambda Z: R.batched_objective(s2, ell, X, om, Y, Rv, v, W, Z, JITTER, fam), Xu)
            out[fam, shp] = (s2, ell, X, om, Y, Rv, v, W, Xu), fd
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_matches_central_differences(cases, family, shape):
    args, fd = cases[family, shape]
    g = analytic_grad_xu(*args, JITTER, family)
    err = np.abs(g - fd).max() / np.abs(g).max()
    print(f"{family} {shape}: |analytic - fd| / max|grad| = {err:.2e}")
    assert err <= FD_BOUND, err


@pytest.mark.parametrize("fault", [dict(uu_scale=0.0), dict(uu_scale=0.5), dict(sign=-1.0)],
                         ids=["uu-half-dropped", "uu-half-halved", "sign-flipped"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_injected_faults_are_caught(cases, family, shape, fault):
    args, fd = cases[family, shape]
    g = analytic_grad_xu(*args, JITTER, family, **fault)
    assert np.abs(g - fd).max() / np.abs(fd).max() > FD_BOUND


class RestatementEngine:
    """What `optimize_inducing` drives, on the restatement: it refuses the objective after `set_inducing` until `set_posterior`,
    as the handle does."""

    def __init__(self, X, om, Y, W, family):
        self.X, self.om, self.Y, self.W, self.family = X, om, Y, W, family
        self.qv = None
        self.calls = []

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.s2, self.ell, self.jitter = sigma2, np.asarray(ell, dtype=np.float64), jitter
        self.calls.append("kernel")

    def set_inducing(self, Xu):
        self.Xu = np.array(Xu, dtype=np.float64)
        self.qv = None
        self.calls.append("inducing")

    def set_posterior(self, mu_v, Uv):
        self.qv = (np.asarray(mu_v), np.asarray(Uv).T @ np.asarray(Uv))
        self.calls.append("posterior")

    def theta_objective_xu(self, want_grad=False):
        if self.qv is None:
            raise RuntimeError("needs a finished sweep or sgp_set_posterior (q(v))")
        self.calls.append("objective")
        v, Rv = self.qv
        a = (self.s2, self.ell, self.X, self.om, self.Y, Rv, v, self.W, self.Xu, self.jitter, self.family)
        return R.batched_objective(*a), R.analytic_grad(*a, n_ell=len(self.ell)), analytic_grad_xu(*a)


def numpy_adamax(x, grad_fn, steps, eta=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    x = x.copy()
    m, u, p1 = np.zeros_like(x), np.zeros_like(x), b1
    for _ in range(steps):
        g = grad_fn(x)
        m = b1 * m + (1 - b1) * g
        u = np.maximum(b2 * u, np.abs(g))
        x = x - eta / (1 - p1) * m / (u + eps)
        p1 *= b1
    return x


@pytest.mark.parametrize("learn_theta", [True, False])
def test_optimize_inducing_is_adamax_on_the_joint_vector(learn_theta):
    from gaussianprocessnode_amd import train as TR
    from gaussianprocessnode_amd.meta import softplus
    from oracle import sgp_oracle as O
    d_out, D, M, N = 2, 3, 7, 40
    X, om, Y, Xu, ell, Rv, v, W = problem(d_out, D, M, N, seed=3)
    Uv = np.linalg.cholesky(Rv).T
    theta0 = O.invsoftplus(np.concatenate([[1.1], ell]))
    eng = RestatementEngine(X, om, Y, W, "matern32")
    th, Z, vals = TR.optimize_inducing(theta0, Xu, eng, q_v=(v, Uv), steps=15, learn_theta=learn_theta, jitter=JITTER)
    assert eng.calls[:4] == ["kernel", "inducing", "posterior", "objective"] and len(eng.calls) == 4 * 15
    nt = theta0.size if learn_theta else 0

    def grad(x):
        t = x[:nt] if learn_theta else theta0
        p = softplus(t)
        a = (p[0], p[1:], X, om, Y, Rv, v, W, x[nt:].reshape(M, D), JITTER, "matern32")
        g = R.analytic_grad(*a, n_ell=D) / (1.0 + np.exp(-t))
        return np.concatenate([g[:nt], analytic_grad_xu(*a).ravel()])
    x = numpy_adamax(np.concatenate([theta0[:nt], Xu.ravel()]), grad, 15)
    np.testing.assert_allclose(Z, x[nt:].reshape(M, D), rtol=1e-12)
    np.testing.assert_allclose(th, x[:nt] if learn_theta else theta0, rtol=1e-12)
    assert vals.shape == (15,) and vals[-1] <= vals[0]
    assert not np.allclose(Z, Xu) and Z is not Xu and th is not theta0


def test_optimize_inducing_takes_a_distribution_and_checks_shapes():
    from gaussianprocessnode_amd import train as TR
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance
    X, om, Y, Xu, ell, Rv, v, W = problem(1, 1, 5, 30, seed=4)
    eng = RestatementEngine(X, om, Y, W, "se")
    q_v = MvNormalMeanCovariance(v, Rv - np.outer(v, v))
    _, Z, vals = TR.optimize_inducing(np.zeros(2), Xu, eng, q_v=q_v, steps=2, jitter=JITTER)
    np.testing.assert_allclose(eng.qv[1], Rv, rtol=1e-10)
    assert Z.shape == Xu.shape and len(vals) == 2
    with pytest.raises(ValueError):
        TR.optimize_inducing(np.zeros(4), Xu, eng, q_v=q_v)                  # 3 lengthscales for D = 1
    with pytest.raises(ValueError):
        TR.optimize_inducing(np.zeros(2), Xu.ravel(), eng, q_v=q_v)          # Xu must be (M, D)


def test_the_entry_point_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    name = "sgp_theta_objective_xu"
    assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
    fn = getattr(_lib.load(), name)
    assert len(fn.argtypes) == 4 and fn.restype is C.c_int
    for kernel in (b"k_xu_grad_uf", b"k_xu_grad_uu", b"k_xu_grad_finish"):
        assert kernel in blob, kernel
    assert "theta_objective_xu" in open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    from gaussianprocessnode_amd import SGPDevice, train
    assert callable(SGPDevice.theta_objective_xu) and callable(train.optimize_inducing)


def test_the_python_method_passes_shapes_and_layout():
    """`theta_objective_xu` over a stand-in library: 1 + n_ell gradient entries, an (M, D) C-order grad_xu (entry m * D + d is
    inducing point m, dimension d -- `set_inducing`'s layout), a NULL grad without want_grad."""
    from gaussianprocessnode_amd import SGPDevice
    M, D, n_ell = 3, 2, 2
    seen = {}

    class Lib:
        @staticmethod
        def sgp_theta_objective_xu(h, value, grad, grad_xu):
            seen["grad_null"] = not grad
            value[0] = 1.5
            if grad:
                for i in range(1 + n_ell):
                    grad[i] = 10.0 + i
            for e in range(M * D):
                grad_xu[e] = float(e)
            return 0

    dev = object.__new__(SGPDevice)
    dev._lib, dev._h, dev.M, dev.D = Lib, C.c_void_p(), M, D
    with pytest.raises(ValueError):
        dev.theta_objective_xu()                                              # no set_kernel yet: the gradient's length is unknown
    dev._n_ell = n_ell
    val, gxu = dev.theta_objective_xu()
    assert seen["grad_null"] and val == 1.5 and gxu.shape == (M, D)
    assert np.array_equal(gxu, np.arange(M * D, dtype=float).reshape(M, D))
    val, g, gxu = dev.theta_objective_xu(want_grad=True)
    assert not seen["grad_null"] and np.array_equal(g, [10.0, 11.0, 12.0]) and gxu[2, 1] == 5.0
