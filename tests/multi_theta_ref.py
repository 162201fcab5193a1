"""NumPy restatement of the MultiSGP hyper-parameter objective (helper, no tests).

`neg_log_backwardmess_multi` is the literal per-node loop of helper_functions/derivative_helper.jl:92-106: srcubature
points of each q(x_i), the node's Psi-statistics, `sum_diagonal_M` of V = v y_i' W and `sum(Rv_blk .* W)` over the blocks
of `create_blockmatrix`.  `batched_objective` is the same sum written with the summed statistics (what the device
evaluates), and `analytic_grad` its gradient w.r.t. (sigma2, ell...):

    f  = 1/2 tr(W) (sigma2 s_w - tr(Kinv Psi2)) + 1/2 tr(S Psi2) - sum_de W_de mu^(d)' B_e
    df = sum_n omega_n dk_n' (G k_n) - sum_n dk_n' sum_d mu^(d) omega_n (W y_n)_d
         + 1/2 tr(W) tr(Kinv Psi2 Kinv dK_uu) + 1/2 tr(W) s_w dsigma2,            G = S - tr(W) Kinv
"""
from __future__ import annotations

import numpy as np

from oracle import sgp_oracle as O
from tests.test_kernel_family_host import kappa, phi, scaled_sq_dist


def kernelmatrix(family, sigma2, ell, A, B=None):
    if family == "se":
        return O.kernelmatrix(sigma2, ell, A, B)
    return float(sigma2) * kappa(family, scaled_sq_dist(ell, A, B))


def full_ell(ell, D):
    return np.broadcast_to(np.asarray(ell, dtype=np.float64).ravel(), (D,)).copy()


def create_blockmatrix(A, d, M):
    """helper_functions/gp_helperfunction.jl:133-135: the d x d grid of M x M views."""
    return [[A[i * M:(i + 1) * M, j * M:(j + 1) * M] for j in range(d)] for i in range(d)]


def sum_rv_wbar(Rv, W, M):
    """`sum(Rv_blk .* W)` of the pendulum notebook: sum_ij W_ij Rv[i][j]."""
    d = W.shape[0]
    blk = create_blockmatrix(Rv, d, M)
    return sum(blk[i][j] * W[i, j] for i in range(d) for j in range(d))


def sum_diagonal_M(V, M):
    """helper_functions/derivative_helper.jl:119-122"""
    return sum(V[M * i:(i + 1) * M, i] for i in range(V.shape[1]))


def psi_statistics(family, Xu, pts, wts, sigma2, ell):
    if family == "se":
        return O.psi_statistics(Xu, pts, wts, sigma2, ell)
    K = kernelmatrix(family, sigma2, ell, Xu, pts)
    w = np.asarray(wts, dtype=np.float64)
    return float(sigma2 * w.sum()), K @ w, (K * w) @ K.T


def neg_log_backwardmess_multi(sigma2, ell, y_data, q_means, q_covs, Rv, v, W, Xu, jitter=1e-12, family="se"):
    """The literal loop: one node at a time, its srcubature points (a node with q_cov None is a point mass)."""
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    ell = full_ell(ell, D)
    Kuu_inverse = np.linalg.inv(kernelmatrix(family, sigma2, ell, Xu) + jitter * np.eye(M))
    sumRv_Wbar = sum_rv_wbar(Rv, W, M)
    tr_W = np.trace(W)
    llh = 0.0
    for i in range(len(q_means)):
        V = np.outer(v, np.asarray(y_data[i]) @ W)
        sumdiagV = sum_diagonal_M(V, M)
        if q_covs is None or q_covs[i] is None:
            pts, wts = np.atleast_2d(q_means[i]), np.ones(1)
        else:
            pts, wts = O.srcubature(q_means[i], q_covs[i])
        Psi0, Psi1, Psi2 = psi_statistics(family, Xu, pts, wts, sigma2, ell)
        llh += -0.5 * tr_W * (Psi0 - np.sum(Kuu_inverse * Psi2)) + np.sum(sumdiagV * Psi1) - 0.5 * np.sum(sumRv_Wbar * Psi2)
    return -llh


def expand(y_data, q_means, q_covs):
    """All nodes' srcubature points, weights and targets (y_data[i] repeated over node i's points)."""
    P, Wt, Y = [], [], []
    for i in range(len(q_means)):
        if q_covs is None or q_covs[i] is None:
            p, w = np.atleast_2d(q_means[i]), np.ones(1)
        else:
            p, w = O.srcubature(q_means[i], q_covs[i])
        P.append(p)
        Wt.append(w)
        Y.append(np.repeat(np.atleast_2d(y_data[i]), len(w), axis=0))
    return np.concatenate(P), np.concatenate(Wt), np.concatenate(Y)


def batched_objective(sigma2, ell, X, omega, Y, Rv, v, W, Xu, jitter=1e-12, family="se"):
    """The summed-statistics form over all points at once."""
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    d = W.shape[0]
    ell = full_ell(ell, D)
    Kinv = np.linalg.inv(kernelmatrix(family, sigma2, ell, Xu) + jitter * np.eye(M))
    Kuf = kernelmatrix(family, sigma2, ell, Xu, X)
    Psi2 = (Kuf * omega) @ Kuf.T
    B = Kuf @ (omega[:, None] * Y)                                  # M x d
    S = sum_rv_wbar(Rv, W, M)
    mu = np.asarray(v, dtype=np.float64).reshape(d, M).T            # M x d
    trW = np.trace(W)
    return (0.5 * trW * (sigma2 * omega.sum() - np.sum(Kinv * Psi2)) + 0.5 * np.sum(S * Psi2)
            - np.sum(W * (mu.T @ B)))


def analytic_grad(sigma2, ell, X, omega, Y, Rv, v, W, Xu, jitter=1e-12, family="se", n_ell=None):
    """d f / d(sigma2, ell_1..ell_n_ell) of batched_objective (n_ell = 1: one shared lengthscale)."""
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    d = W.shape[0]
    n_ell = D if n_ell is None else n_ell
    ellf = full_ell(ell, D)
    Kuu = kernelmatrix(family, sigma2, ellf, Xu)
    Kinv = np.linalg.inv(Kuu + jitter * np.eye(M))
    Kuf = kernelmatrix(family, sigma2, ellf, Xu, X)
    Psi2 = (Kuf * omega) @ Kuf.T
    S = sum_rv_wbar(Rv, W, M)
    mu = np.asarray(v, dtype=np.float64).reshape(d, M).T
    trW = np.trace(W)
    G = S - trW * Kinv
    A = (G @ Kuf) * omega - mu @ (W @ (omega[:, None] * Y).T)       # coefficient of dk_mn
    H = 0.5 * trW * Kinv @ Psi2 @ Kinv
    g = np.empty(1 + n_ell)
    g[0] = 0.5 * trW * omega.sum() + (np.sum(A * Kuf) + np.sum(H * Kuu)) / sigma2
    phi_uf = sigma2 * phi(family, scaled_sq_dist(ellf, Xu, X))
    phi_uu = sigma2 * phi(family, scaled_sq_dist(ellf, Xu))
    gd = np.empty(D)
    for k in range(D):
        duf = (Xu[:, k:k + 1] - X[None, :, k]) ** 2 / ellf[k] ** 3
        duu = (Xu[:, k:k + 1] - Xu[None, :, k]) ** 2 / ellf[k] ** 3
        gd[k] = np.sum(A * phi_uf * duf) + np.sum(H * phi_uu * duu)
    if n_ell == 1:
        g[1] = gd.sum()
    else:
        g[1:] = gd
    return g
