"""NumPy restatement of the exact-Psi input messages (helper, no tests): the part of a node's average energy that depends on its
Gaussian input x_t ~ N(m_t, S_t) and its derivatives with respect to m_t and S_t -- the reference of tests/test_gpu_psi_in.py, itself
checked by tests/test_psi_in_host.py.

With q(v), W = mean(q_W), G = S_q - tr(W) (K_uu + jitter I)^-1 and s_t = sum_d mu^(d) (W y_t)_d as in tests/psi_theta_ref.py,
P_c = (Lambda + c S_t)^-1, h^(c)_tm = P_c (m_t - z_m) and u_ij = h^(2)_ti + h^(2)_tj:

    U_t     = 1/2 tr(G Psi2_t) - s_t' Psi1_t                        (the theta objective is 1/2 tr(W) sigma2 T + sum_t U_t)
    gamma_t = dU_t / dm_t = -1/2 b_t + b1_t
    Gamma_t = dU_t / dS_t = -1/2 A_t P_2 + 1/4 C_t + 1/2 a1_t P_1 - 1/2 C1_t          (dU = <Gamma, dS> for symmetric dS)
    A_t, b_t, C_t    = sum_ij G_ij Psi2_t[i,j] (1, u_ij, u_ij u_ij')
    a1_t, b1_t, C1_t = sum_m s_t[m] Psi1_t[m] (1, h^(1)_tm, h^(1)_tm h^(1)_tm')

`energy` takes Psi1_t and Psi2_t from tests/psi_stats_ref (determinants and dense solves: no factors, no g, no h); `analytic` is the
formulas as they stand above, with dense inverses.  `fault` injects the three mistakes the host test must catch: "h_c1" (P_1 used for
h^(2)), "no_p2" (the -1/2 A_t P_2 term dropped), "offdiag_once" (the off-diagonal entries of the double sum counted once).
"""
import numpy as np

from tests import psi_stats_ref as PR
from tests import psi_theta_ref as TR


def _inputs(sigma2, ell, mean, Y, Rv, v, W, Xu, jitter):
    Xu, M, D, W, ellf, _, _, G, mu = TR._common(sigma2, ell, Xu, Rv, v, W, jitter)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, D)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(mean), -1)
    return Xu, M, D, W, ellf, G, mean, (Y @ W.T) @ mu                   # s (T, M): s_t = sum_d mu^(d) (W y_t)_d


def _cov(cov, t, D):
    return np.zeros((D, D)) if cov is None else np.asarray(cov[t], dtype=np.float64).reshape(D, D)


def energy(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12):
    """U (T,); mean (T, D), cov (T, D, D) or None, Y (T, d_out)."""
    Xu, M, D, W, ellf, G, mean, s = _inputs(sigma2, ell, mean, Y, Rv, v, W, Xu, jitter)
    U = np.empty(len(mean))
    for t in range(len(mean)):
        S = _cov(cov, t, D)
        U[t] = 0.5 * np.sum(G * PR.psi2_node(Xu, sigma2, ellf, mean[t], S)) - s[t] @ PR.psi1_node(Xu, sigma2, ellf, mean[t], S)
    return U


def analytic(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12, fault=None):
    """(gamma (T, D), Gamma (T, D, D))"""
    Xu, M, D, W, ellf, G, mean, s = _inputs(sigma2, ell, mean, Y, Rv, v, W, Xu, jitter)
    lam = ellf ** 2
    T = len(mean)
    gamma, Gamma = np.empty((T, D)), np.empty((T, D, D))
    for t in range(T):
        S = _cov(cov, t, D)
        P1, P2 = np.linalg.inv(np.diag(lam) + S), np.linalg.inv(np.diag(lam) + 2.0 * S)
        a = mean[t][None, :] - Xu                                       # (M, D)
        h1 = a @ P1
        h2 = a @ (P1 if fault == "h_c1" else P2)
        w2 = G * PR.psi2_node(Xu, sigma2, ellf, mean[t], S)
        if fault == "offdiag_once":
            w2 = np.tril(w2)
        u = h2[:, None, :] + h2[None, :, :]
        A, b, C = w2.sum(), np.einsum("ij,ijd->d", w2, u), np.einsum("ij,ijd,ije->de", w2, u, u)
        w1 = s[t] * PR.psi1_node(Xu, sigma2, ellf, mean[t], S)
        a1, b1, C1 = w1.sum(), w1 @ h1, np.einsum("m,md,me->de", w1, h1, h1)
        gamma[t] = -0.5 * b + b1
        Gamma[t] = 0.25 * C + 0.5 * a1 * P1 - 0.5 * C1
        if fault != "no_p2":
            Gamma[t] -= 0.5 * A * P2
    return gamma, 0.5 * (Gamma + Gamma.transpose(0, 2, 1))


def evaluate(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12):
    """(U, gamma, Gamma): what SGPDevice.psi_in_grad returns"""
    return (energy(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter),) + analytic(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter)


def numeric(sigma2, ell, mean, cov, Y, Rv, v, W, Xu, jitter=1e-12, step=1e-5):
    """Central differences of `energy`: gamma (T, D) and Gamma (T, D, D).  Gamma_aa from the direction E_aa; Gamma_ab, a != b, from the
    symmetric direction E_ab + E_ba, which gives 2 Gamma_ab."""
    mean = np.asarray(mean, dtype=np.float64)
    T, D = mean.shape
    S0 = np.zeros((T, D, D)) if cov is None else np.asarray(cov, dtype=np.float64)
    rest = (Y, Rv, v, W, Xu, jitter)
    gamma, Gamma = np.empty((T, D)), np.empty((T, D, D))
    for d in range(D):
        e = np.zeros(D)
        e[d] = step
        gamma[:, d] = (energy(sigma2, ell, mean + e, S0, *rest) - energy(sigma2, ell, mean - e, S0, *rest)) / (2 * step)
    for a in range(D):
        for b in range(a + 1):
            E = np.zeros((D, D))
            E[a, b] = E[b, a] = step
            dU = (energy(sigma2, ell, mean, S0 + E, *rest) - energy(sigma2, ell, mean, S0 - E, *rest)) / (2 * step)
            Gamma[:, a, b] = Gamma[:, b, a] = dU if a == b else 0.5 * dU
    return gamma, Gamma


def stacked(gamma, Gamma):
    """(T, D + D D): a node's gamma and Gamma side by side, as the gradient bounds take them"""
    return np.concatenate([gamma, Gamma.reshape(len(gamma), -1)], axis=1)
