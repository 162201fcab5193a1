"""NumPy restatement of the closed-form prediction at Gaussian inputs (helper, no tests) -- the reference of
tests/test_gpu_psi_predict.py, itself checked by tests/test_psi_predict_host.py against a tensor Gauss-Hermite rule.

With x_t ~ N(m_t, S_t), Lambda = diag(ell^2), P_c = (Lambda + c S_t)^-1, Kinv = (K_uu + jitter I)^-1, q(v) = N(mu, Sigma_v) and
R^(ij) = Sigma_v^(ij) + mu^(i) mu^(j)' (the (i, j) block of R_v, outputs major):

    mean[t, i]     = Psi1_t' mu^(i)
    C_f[t][i][j]   = delta_ij (sigma2 - tr(Kinv Psi2_t)) + tr(R^(ij) Psi2_t) - mean[t, i] mean[t, j]
    cross[t][:, i] = Cov[x_t, f_i] = S_t P_1 sum_m mu^(i)_m Psi1_t[m] (z_m - m_t)

Psi1_t and Psi2_t come from tests/psi_stats_ref (determinants and dense solves: no factors, no g), the rest is dense.  Beside the values
`predict` returns the magnitudes the error bounds are stated in:

    mag[t][i][j]    = delta_ij (sigma2 + |tr(Kinv Psi2_t)|) + |tr(R^(ij) Psi2_t)| + |mean_i mean_j|
    cmag[t][:, i]   = sum_m |mu^(i)_m Psi1_t[m]| |S_t P_1 (z_m - m_t)|

`fault` injects the three mistakes the host test must catch: "keep_mean_sq" (- mean_i mean_j dropped), "p2_cross" (P_2 used for P_1 in
cross), "offdiag_once" (the off-diagonal entries of the double sums over Psi2_t counted once).
"""
import numpy as np

from tests import multi_theta_ref as MR
from tests import psi_stats_ref as PR


def predict(sigma2, ell, mean, cov, Rv, v, Xu, d_out, jitter=1e-12, fault=None):
    """(mean (T, d_out), C_f (T, d_out, d_out), cross (T, D, d_out), mag (T, d_out, d_out), cmag (T, D, d_out)); mean (T, D), cov
    (T, D, D) or None, Rv (d_out M, d_out M), v (d_out M,)."""
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    ellf = MR.full_ell(ell, D)
    Kinv = np.linalg.inv(MR.kernelmatrix("se", sigma2, ellf, Xu) + jitter * np.eye(M))
    mu = np.asarray(v, dtype=np.float64).reshape(d_out, M)
    R = MR.create_blockmatrix(np.asarray(Rv, dtype=np.float64), d_out, M)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, D)
    T = len(mean)
    out, Cf, cross = np.empty((T, d_out)), np.empty((T, d_out, d_out)), np.empty((T, D, d_out))
    mag, cmag = np.empty((T, d_out, d_out)), np.empty((T, D, d_out))
    for t in range(T):
        S = np.zeros((D, D)) if cov is None else np.asarray(cov[t], dtype=np.float64).reshape(D, D)
        psi1 = PR.psi1_node(Xu, sigma2, ellf, mean[t], S)
        psi2 = PR.psi2_node(Xu, sigma2, ellf, mean[t], S)
        if fault == "offdiag_once":
            psi2 = np.tril(psi2)
        out[t] = mu @ psi1
        tk = np.sum(Kinv * psi2)
        for i in range(d_out):
            for j in range(d_out):
                tr = np.sum(R[i][j] * psi2.T)                           # tr(R^(ij) Psi2_t)
                sq = 0.0 if fault == "keep_mean_sq" else out[t, i] * out[t, j]
                Cf[t, i, j] = (sigma2 - tk if i == j else 0.0) + tr - sq
                mag[t, i, j] = (sigma2 + abs(tk) if i == j else 0.0) + abs(tr) + abs(out[t, i] * out[t, j])
        P = np.linalg.inv(np.diag(ellf ** 2) + (2.0 if fault == "p2_cross" else 1.0) * S)
        a = (Xu - mean[t][None, :]) @ (S @ P).T                         # (M, D): S P_1 (z_m - m_t)
        wgt = mu * psi1[None, :]                                        # (d_out, M)
        cross[t] = a.T @ wgt.T
        cmag[t] = np.abs(a).T @ np.abs(wgt).T
    return out, Cf, cross, mag, cmag


def point_predictive(sigma2, ell, X, Sigma_v, v, Xu, d_out, jitter=1e-12):
    """The plain predictive of the latent f at points X (n, D): mean (n, d_out), cov (n, d_out, d_out) = delta_ij (sigma2 - k' Kinv k) +
    k' Sigma_v^(ij) k."""
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    ellf = MR.full_ell(ell, D)
    X = np.asarray(X, dtype=np.float64).reshape(-1, D)
    Kinv = np.linalg.inv(MR.kernelmatrix("se", sigma2, ellf, Xu) + jitter * np.eye(M))
    K = MR.kernelmatrix("se", sigma2, ellf, X, Xu)                      # (n, M)
    mu = np.asarray(v, dtype=np.float64).reshape(d_out, M)
    Sg = MR.create_blockmatrix(np.asarray(Sigma_v, dtype=np.float64), d_out, M)
    m = K @ mu.T
    C = np.zeros((len(X), d_out, d_out))
    q = sigma2 - np.einsum("nm,mk,nk->n", K, Kinv, K)
    for i in range(d_out):
        for j in range(d_out):
            C[:, i, j] = np.einsum("nm,mk,nk->n", K, Sg[i][j], K) + (q if i == j else 0.0)
    return m, C
