"""NumPy restatement of the kernel-parameter objective over exact Psi-statistics and of its analytic gradient (helper, no tests) -- the
reference of tests/test_gpu_psi_theta.py and tests/test_gpu_psi_theta_descend.py, itself checked by tests/test_psi_theta_host.py.

With q(v) = N(v, Sigma_v), R_v = Sigma_v + v v', W = mean(q_W), S_q = sum_ij W_ij R_v^(ij), Kinv = (K_uu + jitter I)^-1,
G = S_q - tr(W) Kinv and s_t = sum_d mu^(d) (W y_t)_d:

    f  = 1/2 tr(W) sigma2 T + 1/2 tr(G Psi2) - sum_t s_t' Psi1_t,                     Psi2 = sum_t Psi2_t
    df = 1/2 tr(G dPsi2) - sum_t s_t' dPsi1_t + 1/2 tr(W) tr(Kinv Psi2 Kinv dK_uu) + 1/2 tr(W) T dsigma2

    dlog Psi1_t[m]   / dell_d = 1/ell_d - ell_d (P_1)_dd + ell_d (h1_tm,d)^2                                   P_c = (Lambda + c S_t)^-1
    dlog Psi2_t[m,m']/ dell_d = 1/ell_d - ell_d (P_2)_dd + 1/2 (z_md - z_m'd)^2 / ell_d^3 + 1/2 ell_d (h2_tm,d + h2_tm',d)^2
                                                                                                               h^(c)_tm = P_c (m_t - z_m)

`objective` takes Psi1 and Psi2 from tests/psi_stats_ref.psi_stats (determinants and dense solves: no factors, no g, no h), so the value
shares nothing with the device's factorised form; `analytic_grad` is the formulas as they stand above, with dense inverses.  `fault`
injects the three mistakes the host test must catch.
"""
import numpy as np

from tests import multi_theta_ref as MR
from tests import psi_stats_ref as PR


def _common(sigma2, ell, Xu, Rv, v, W, jitter):
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    d = W.shape[0]
    ellf = MR.full_ell(ell, D)
    Kuu = MR.kernelmatrix("se", sigma2, ellf, Xu)
    Kinv = np.linalg.inv(Kuu + jitter * np.eye(M))
    G = MR.sum_rv_wbar(np.asarray(Rv, dtype=np.float64), W, M) - np.trace(W) * Kinv
    mu = np.asarray(v, dtype=np.float64).reshape(d, M)                  # (d, M)
    return Xu, M, D, W, ellf, Kuu, Kinv, G, mu


def objective(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12):
    """f at (sigma2, ell); mean (T, D), cov (T, D, D) or None, Y (T, d_out)."""
    Xu, M, D, W, ellf, _, _, G, mu = _common(sigma2, ell, Xu, Rv, v, W, jitter)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(mean), -1)
    psi1, psi2 = PR.psi_stats(Xu, sigma2, ellf, mean, cov)
    s = (Y @ W.T) @ mu                                                  # (T, M): s_t = sum_d mu^(d) (W y_t)_d
    return 0.5 * np.trace(W) * sigma2 * len(mean) + 0.5 * np.sum(G * psi2) - np.sum(s * psi1)


def analytic_grad(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12, n_ell=None, fault=None):
    """d f / d(sigma2, ell_1 .. ell_n_ell) (n_ell = 1: one shared lengthscale, the sum over the dimensions)."""
    Xu, M, D, W, ellf, Kuu, Kinv, G, mu = _common(sigma2, ell, Xu, Rv, v, W, jitter)
    n_ell = D if n_ell is None else n_ell
    mean = np.asarray(mean, dtype=np.float64)
    T = len(mean)
    Y = np.asarray(Y, dtype=np.float64).reshape(T, -1)
    s = (Y @ W.T) @ mu
    trW = np.trace(W)
    lam = ellf ** 2
    dz2 = (Xu[:, None, :] - Xu[None, :, :]) ** 2                        # (M, M, D)
    g_s2, g_ell, psi2 = 0.0, np.zeros(D), np.zeros((M, M))
    for t in range(T):
        S = np.zeros((D, D)) if cov is None else np.asarray(cov[t], dtype=np.float64)
        p1 = PR.psi1_node(Xu, sigma2, ellf, mean[t], S)
        p2 = PR.psi2_node(Xu, sigma2, ellf, mean[t], S)
        psi2 += p2
        P1, P2 = np.linalg.inv(np.diag(lam) + S), np.linalg.inv(np.diag(lam) + 2.0 * S)
        a = mean[t][None, :] - Xu                                       # (M, D)
        h1 = a @ P1
        h2 = a @ (P1 if fault == "h_c1" else P2)
        det1 = 0.0 if fault == "no_det" else 1.0 / ellf - ellf * np.diag(P1)
        det2 = 0.0 if fault == "no_det" else 1.0 / ellf - ellf * np.diag(P2)
        dl1 = det1 + ellf * h1 ** 2                                     # (M, D)
        dl2 = det2 + 0.5 * ellf * (h2[:, None, :] + h2[None, :, :]) ** 2
        if fault != "no_dz":
            dl2 = dl2 + 0.5 * dz2 / ellf ** 3
        g_s2 += np.sum(G * p2) / sigma2 - np.sum(s[t] * p1) / sigma2
        g_ell += 0.5 * np.einsum("ab,ab,abd->d", G, p2, dl2) - (s[t] * p1) @ dl1
    H = 0.5 * trW * Kinv @ psi2 @ Kinv
    g = np.empty(1 + n_ell)
    g[0] = g_s2 + np.sum(H * Kuu) / sigma2 + 0.5 * trW * T
    gd = g_ell + np.einsum("ab,ab,abd->d", H, Kuu, dz2) / ellf ** 3
    if n_ell == 1:
        g[1] = gd.sum()
    else:
        g[1:] = gd
    return g


def numeric_grad(sigma2, ell, *args, n_ell=None, rel=1e-6, **kw):
    """central differences of `objective` in (sigma2, ell_1 .. ell_n_ell)"""
    D = np.asarray(args[-1]).shape[1]
    n_ell = D if n_ell is None else n_ell
    ell0 = MR.full_ell(ell, D) if n_ell == D else np.atleast_1d(np.asarray(ell, dtype=np.float64))[:1].copy()
    x0 = np.concatenate([[sigma2], ell0])
    g = np.empty(1 + n_ell)
    for i in range(1 + n_ell):
        hstep = rel * x0[i]
        xp, xm = x0.copy(), x0.copy()
        xp[i] += hstep
        xm[i] -= hstep
        g[i] = (objective(xp[0], xp[1:], *args, **kw) - objective(xm[0], xm[1:], *args, **kw)) / (2 * hstep)
    return g


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def descend(theta_raw, n_ell, steps, mean, cov, Y, Rv, v, W, Xu, jitter, eta=0.002, beta1=0.9, beta2=0.999, eps=1e-8):
    """The NumPy loop of sgp_theta_descend_psi: AdaMax on the raw parameters with the chain rule through softplus, as
    tests/theta_descend_ref.py restates it for the cubature objective.  Returns (theta, values)."""
    th = np.array(theta_raw, dtype=np.float64)
    m, u, p1 = np.zeros_like(th), np.zeros_like(th), beta1
    values = np.empty(steps)
    for k in range(steps):
        par = softplus(th)
        values[k] = objective(par[0], par[1:], mean, cov, Y, Rv, v, W, Xu, jitter)
        g = analytic_grad(par[0], par[1:], mean, cov, Y, Rv, v, W, Xu, jitter, n_ell=n_ell) / (1.0 + np.exp(-th))
        m = beta1 * m + (1.0 - beta1) * g
        u = np.maximum(beta2 * u, np.abs(g))
        th = th - (eta / (1.0 - p1)) * m / (u + eps)
        p1 *= beta1
    return th, values
