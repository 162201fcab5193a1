"""NumPy restatement of the theta objective's gradient in the inducing inputs (helper, no tests).

With the notation of `multi_theta_ref.batched_objective` (G = S - tr(W) Kinv, H = Kinv Psi2 Kinv without the 1/2: z_m moves row
and column m of K_uu; A_mn = omega_n (G k_n)_m - sum_d mu^(d)_m (omega_n W y_n)_d) and dk(a, b)/db_d = sigma2 phi (a_d - b_d) /
ell_d^2:

    df/dz_md = [ sum_n A_mn sigma2 phi(z_m, x_n) (x_nd - z_md) + tr(W) sum_m' H_mm' sigma2 phi(z_m, z_m') (z_m'd - z_md) ] / ell_d^2

UniSGP is d_out = 1 with W = [[w]].  `uu_scale` and `sign` exist for the tests' injected faults only.
"""
from __future__ import annotations

import numpy as np

from tests.multi_theta_ref import full_ell, kernelmatrix, phi, scaled_sq_dist, sum_rv_wbar


def analytic_grad_xu(sigma2, ell, X, omega, Y, Rv, v, W, Xu, jitter=1e-12, family="se", *, uu_scale=1.0, sign=1.0):
    """d f / d Xu of batched_objective, (M, D)."""
    Xu = np.asarray(Xu, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).reshape(-1, Xu.shape[1])
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    M, D = Xu.shape
    d = W.shape[0]
    ellf = full_ell(ell, D)
    Kinv = np.linalg.inv(kernelmatrix(family, sigma2, ellf, Xu) + jitter * np.eye(M))
    Kuf = kernelmatrix(family, sigma2, ellf, Xu, X)
    Psi2 = (Kuf * omega) @ Kuf.T
    S = sum_rv_wbar(np.asarray(Rv, dtype=np.float64), W, M)
    mu = np.asarray(v, dtype=np.float64).reshape(d, M).T
    trW = np.trace(W)
    G = S - trW * Kinv
    A = (G @ Kuf) * omega - mu @ (W @ (omega[:, None] * np.asarray(Y, dtype=np.float64).reshape(len(omega), d)).T)
    H = Kinv @ Psi2 @ Kinv
    Zuf = A * (sigma2 * phi(family, scaled_sq_dist(ellf, Xu, X)))
    Zuu = trW * H * (sigma2 * phi(family, scaled_sq_dist(ellf, Xu)))
    g = np.empty((M, D))
    for k in range(D):
        duf = sign * (X[None, :, k] - Xu[:, k:k + 1])
        duu = sign * (Xu[None, :, k] - Xu[:, k:k + 1])
        g[:, k] = (np.sum(Zuf * duf, axis=1) + uu_scale * np.sum(Zuu * duu, axis=1)) / ellf[k] ** 2
    return g
