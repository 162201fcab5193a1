"""NumPy restatement of the exact-Psi theta objective's gradient in the inducing inputs (helper, no tests) -- the reference of
tests/test_gpu_psi_xu.py, itself checked against central differences of `psi_theta_ref.objective` by tests/test_psi_xu_host.py.

With the notation of tests/psi_theta_ref.py (G = S_q - tr(W) Kinv, s_t = sum_d mu^(d) (W y_t)_d), P_c = (Lambda + c S_t)^-1,
h(c)_tm = P_c (m_t - z_m) and H = Kinv Psi2 Kinv (no 1/2: z_m moves row and column m of K_uu):

    df/dz_md = - sum_t s_t[m] Psi1_t[m] h(1)_tm,d                                  (Psi1 half)
               + 1/2 sum_t sum_j G_mj Psi2_t[m,j] (h(2)_tm,d + h(2)_tj,d)          (Psi2 half, node part: the row and the column contribution)
               - 1/2 sum_j G_mj Psi2[m,j] (z_md - z_jd) / ell_d^2                  (Psi2 half, node-independent part)
               + tr(W) sum_j H_mj K_uu[m,j] (z_jd - z_md) / ell_d^2                (K_uu half)

Psi1_t and Psi2_t come from psi_stats_ref.psi1_node / psi2_node (determinants and dense solves), the inverses are dense and nothing
is reused between the terms.  `fault` injects the three mistakes the host test must catch: "no_column" drops sum_j omega h_j,
"uu_halved" halves the K_uu half, "dz_sign" flips the sign of the (z_m - z_j) term.
"""
import numpy as np

from tests import multi_theta_ref as MR
from tests import psi_stats_ref as PR
from tests import psi_theta_ref as TR


def analytic_grad_xu(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12, fault=None):
    """d f / d Xu of psi_theta_ref.objective, (M, D); mean (T, D), cov (T, D, D) or None, Y (T, d_out)."""
    Xu, M, D, W, ellf, Kuu, Kinv, G, mu = TR._common(sigma2, ell, Xu, Rv, v, W, jitter)
    mean = np.asarray(mean, dtype=np.float64)
    T = len(mean)
    Y = np.asarray(Y, dtype=np.float64).reshape(T, -1)
    s = (Y @ W.T) @ mu                                                  # (T, M)
    trW = np.trace(W)
    lam = ellf ** 2
    dz = Xu[:, None, :] - Xu[None, :, :]                                # (M, M, D): z_m - z_j
    g, psi2 = np.zeros((M, D)), np.zeros((M, M))
    for t in range(T):
        S = np.zeros((D, D)) if cov is None else np.asarray(cov[t], dtype=np.float64)
        p1 = PR.psi1_node(Xu, sigma2, ellf, mean[t], S)
        p2 = PR.psi2_node(Xu, sigma2, ellf, mean[t], S)
        psi2 += p2
        a = mean[t][None, :] - Xu                                       # (M, D)
        h1 = a @ np.linalg.inv(np.diag(lam) + S)
        h2 = a @ np.linalg.inv(np.diag(lam) + 2.0 * S)
        om = G * p2
        g -= (s[t] * p1)[:, None] * h1
        g += 0.5 * om.sum(axis=1)[:, None] * h2
        if fault != "no_column":
            g += 0.5 * om @ h2
    sign = -1.0 if fault == "dz_sign" else 1.0
    g -= sign * 0.5 * np.einsum("mj,mjd->md", G * psi2, dz) / lam
    H = Kinv @ psi2 @ Kinv
    Koff = MR.kernelmatrix("se", sigma2, ellf, Xu)                      # (its diagonal meets z_m - z_m = 0)
    g += (0.5 if fault == "uu_halved" else 1.0) * trW * np.einsum("mj,mjd->md", H * Koff, -dz) / lam
    return g


def numeric_grad_xu(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12, h=1e-6):
    """central differences of psi_theta_ref.objective in Xu"""
    Xu = np.asarray(Xu, dtype=np.float64)
    g = np.empty_like(Xu)
    for idx in np.ndindex(*Xu.shape):
        e = np.zeros_like(Xu)
        e[idx] = h
        g[idx] = (TR.objective(sigma2, ell, mean, cov, Y, Rv, v, W, Xu + e, jitter)
                  - TR.objective(sigma2, ell, mean, cov, Y, Rv, v, W, Xu - e, jitter)) / (2 * h)
    return g


def adamax(x, grad_fn, steps, eta=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """The loop of `train.optimize_inducing` on a flat vector: returns (x, values) with grad_fn(x) -> (value, gradient)."""
    x = np.array(x, dtype=np.float64)
    m, u, p1 = np.zeros_like(x), np.zeros_like(x), b1
    values = np.empty(steps)
    for k in range(steps):
        values[k], g = grad_fn(x)
        m = b1 * m + (1 - b1) * g
        u = np.maximum(b2 * u, np.abs(g))
        x = x - eta / (1 - p1) * m / (u + eps)
        p1 *= b1
    return x, values
