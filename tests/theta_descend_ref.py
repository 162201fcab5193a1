"""NumPy restatement of sgp_theta_descend (helper, no tests): `steps` AdaMax steps on the raw kernel parameters with q(v), data
and noise held, as include/sgp_hip.h states it.

Per step: p = softplus(theta); value and gradient of the objective at p -- d_out >= 2: `multi_theta_ref.batched_objective` and
`analytic_grad`; d_out = 1: neg_log_backwardmess_fast and its analytic gradient as tests/train_step_ref.py forms them, here with
the point weights omega of sgp_set_data (Psi2 = sum omega k k', B = sum omega k y, s_w = sum omega) --; chain rule through
softplus; `train.AdaMax`.  The cases of tests/test_gpu_theta_descend.py are built here from seeds, and `host_qv` is the q(v) of
one VMP update in NumPy, so that the host file can run the loop without a device."""
from __future__ import annotations

import functools
import math

import numpy as np

from gaussianprocessnode_amd import train as TR
from oracle import sgp_oracle as O
from tests import multi_theta_ref as MR
from tests import train_step_ref as TS


# ---------------------------------------------------------------------------------------------------------------------------
# d_out = 1 with point weights
# ---------------------------------------------------------------------------------------------------------------------------
def uni_objective(family, sigma2, ell, Xu, X, omega, y, mu, R, w, jitter):
    """f = w/2 [sigma2 s_w - tr(Kinv Psi2) + tr(R Psi2)] - w mu' B"""
    M, D = Xu.shape
    ell = TS.full_ell(ell, D)
    Kinv = np.linalg.inv(TS.kernelmatrix(family, sigma2, ell, Xu, Xu) + jitter * np.eye(M))
    Kuf = TS.kernelmatrix(family, sigma2, ell, Xu, X)
    Psi2 = (Kuf * omega) @ Kuf.T
    return 0.5 * w * (sigma2 * omega.sum() - np.sum(Kinv * Psi2) + np.sum(R * Psi2)) - w * float(mu @ (Kuf @ (omega * y)))


def uni_grad(family, sigma2, ell, n_ell, Xu, X, omega, y, mu, R, w, jitter):
    """df = w [ sum_pn omega_n dK_uf o ((R - Kinv) K_uf - mu y') + 1/2 sum H o dK_uu + 1/2 s_w dsigma2 ],  H = Kinv Psi2 Kinv"""
    M, D = Xu.shape
    ell = TS.full_ell(ell, D)
    s_uu, s_uf = TS.sq_dist(ell, Xu, Xu), TS.sq_dist(ell, Xu, X)
    Kuu, Kuf = sigma2 * TS.kappa(family, s_uu), sigma2 * TS.kappa(family, s_uf)
    Kinv = np.linalg.inv(Kuu + jitter * np.eye(M))
    Psi2 = (Kuf * omega) @ Kuf.T
    H = Kinv @ Psi2 @ Kinv
    A = ((R - Kinv) @ Kuf - np.outer(mu, y)) * omega
    dsu, dsf = -2.0 * sigma2 * TS.dkappa_ds(family, s_uu), -2.0 * sigma2 * TS.dkappa_ds(family, s_uf)
    d_uf = [Kuf / sigma2] + [dsf * (Xu[:, k:k + 1] - X[None, :, k]) ** 2 / ell[k] ** 3 for k in range(D)]
    d_uu = [Kuu / sigma2] + [dsu * (Xu[:, k:k + 1] - Xu[None, :, k]) ** 2 / ell[k] ** 3 for k in range(D)]
    full = np.array([np.sum(A * f) + 0.5 * np.sum(H * u) for f, u in zip(d_uf, d_uu)])
    full[0] += 0.5 * omega.sum()
    return w * (np.array([full[0], full[1:].sum()]) if n_ell == 1 else full)


# ---------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------
def value_and_grad(case, p, mu, Sigma):
    """(f, df / d(sigma2, ell...)) at the kernel values p with q(v) = N(mu, Sigma)."""
    R = Sigma + np.outer(mu, mu)
    n_ell = len(p) - 1
    if case["d_out"] == 1:
        args = (case["Xu"], case["X"], case["omega"], case["Y"][:, 0], mu, R, float(case["W"][0, 0]), case["jitter"])
        return (uni_objective(case["family"], p[0], p[1:], *args), uni_grad(case["family"], p[0], p[1:], n_ell, *args))
    args = (case["X"], case["omega"], case["Y"], R, mu, case["W"], case["Xu"], case["jitter"], case["family"])
    return MR.batched_objective(p[0], p[1:], *args), MR.analytic_grad(p[0], p[1:], *args, n_ell=n_ell)


def descend(case, mu, Sigma, theta0, steps, *, eta=1e-3, beta=(0.9, 0.999), eps=1e-8, state=None):
    """(theta, values, state): the loop with `train.AdaMax`; `state` in the [m | u | beta1^t, beta2^t] layout (None: fresh)."""
    theta = np.array(theta0, dtype=np.float64)
    opt = TR.AdaMax(eta=eta, beta=beta, eps=eps)
    if state is not None:
        opt.set_state(theta, state)
    values = np.empty(steps)
    for k in range(steps):
        f, g = value_and_grad(case, O.softplus(theta), mu, Sigma)
        values[k] = f
        opt.update(theta, g * TR.sigmoid(theta))
    return theta, values, opt.get_state(theta)


def host_qv(case, theta0, prior_var=50.0):
    """q(v) of one VMP update at softplus(theta0) from the isotropic prior, in NumPy: precision block (d, e) = W_de Psi2 (+ prior),
    xi block d = sum_e W_de B_e; v = [v^(1); ..; v^(d_out)]."""
    p = O.softplus(np.asarray(theta0, dtype=np.float64))
    M, D = case["Xu"].shape
    Kuf = MR.kernelmatrix(case["family"], p[0], MR.full_ell(p[1:], D), case["Xu"], case["X"])
    Psi2 = (Kuf * case["omega"]) @ Kuf.T
    B = Kuf @ (case["omega"][:, None] * case["Y"])
    W = case["W"]
    Lam = np.kron(W, Psi2) + np.eye(case["d_out"] * M) / prior_var
    Sigma = np.linalg.inv(Lam)
    Sigma = 0.5 * (Sigma + Sigma.T)
    return Sigma @ (B @ W.T).T.ravel(), Sigma


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def pendulum(n_nodes, seed=0):
    """The seeded synthetic pendulum of tests/test_gpu_multi_theta.py, restated: x_t = (angle, angular velocity), q(x_t) Gaussian
    around a noisy trajectory, targets the next state's mean."""
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


def pendulum_grid():
    """48 inducing points on the 8 x 6 grid over the swing"""
    return np.stack(np.meshgrid(np.linspace(-1.3, 1.3, 8), np.linspace(-3.7, 3.7, 6), indexing="ij"), -1).reshape(48, 2)


# name: d_out, D, M, isotropic, family, jitter, points, point weights, steps, eta
SHAPES = {
    "uni_m20_d1_iso_se": (1, 1, 20, True, "se", 1e-8, 60, False, 8, 0.01),
    "pendulum": (2, 2, 48, False, "se", 1e-12, 300, True, 100, 1e-3),
    "d4_m96_d5_ard_m32": (4, 5, 96, False, "matern32", 1e-8, 300, False, 8, 0.01),
    "d3_m130_d2_iso_m12": (3, 2, 130, True, "matern12", 1e-8, 200, False, 8, 0.01),
    "uni_m130_d3_ard_m52_weights": (1, 3, 130, False, "matern52", 1e-8, 200, True, 8, 0.01),
}


@functools.lru_cache(maxsize=None)
def get_case(name):
    """The case's inputs (arrays not to be written to): points X, weights omega, targets Y (n x d_out), n_nodes, Xu, W, theta0."""
    d_out, D, M, iso, family, jitter, n, weighted, steps, eta = SHAPES[name]
    rng = np.random.default_rng(1000 + sorted(SHAPES).index(name))
    if name == "pendulum":
        means, covs, Yn = pendulum(n // 5)                          # 60 nodes x 5 srcubature points
        X, omega, Y = MR.expand(Yn, means, covs)
        Xu, W, n_nodes = pendulum_grid(), 100.0 * np.eye(2), len(Yn)
        theta0 = O.invsoftplus(np.array([1.0, 0.4, 1.0]))
    else:
        X = rng.uniform(-1.7, 1.7, (n, D))
        Y = np.sin(X @ rng.normal(size=(D, d_out)) / math.sqrt(D) * 2.0) + 0.05 * rng.normal(size=(n, d_out))
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
        omega = rng.uniform(0.5, 1.5, n) if weighted else np.ones(n)
        A = rng.normal(size=(d_out, d_out))
        W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
        n_ell = 1 if iso else D
        theta0 = O.invsoftplus(np.concatenate([[1.05], 0.5 * math.sqrt(D) * np.linspace(0.9, 1.1, n_ell)]))
        n_nodes = n
    return dict(name=name, d_out=d_out, D=D, M=M, family=family, jitter=jitter, X=X, omega=omega, Y=Y, n_nodes=n_nodes, Xu=Xu, W=W,
                theta0=theta0, n_ell=len(theta0) - 1, steps=steps, eta=eta, weighted=weighted)
