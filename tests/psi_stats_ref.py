"""NumPy restatement of the closed-form SE Psi-statistics of Gaussian inputs and of the statistics packing of an exact sweep -- the
reference of tests/test_gpu_psi_stats.py and tests/test_gpu_psi_sweep.py, itself validated against quadrature, the point kernel
and the cubature restatement by tests/test_psi_stats_host.py.

    k(x, z)       = sigma2 exp(-1/2 sum_d (x_d - z_d)^2 / ell_d^2),   Lambda = diag(ell^2),   x ~ N(m, S)
    Psi1[m]       = sigma2 |I + Lambda^-1 S|^-1/2 exp(-1/2 (m - z_m)' (Lambda + S)^-1 (m - z_m))
    Psi2[m, m']   = sigma2^2 |I + 2 Lambda^-1 S|^-1/2 exp(-1/4 (z_m - z_m')' Lambda^-1 (z_m - z_m') - (m - zb)' (Lambda + 2 S)^-1 (m - zb))

The formulas are written as they stand above -- determinants and linear solves of the D x D matrices, no Cholesky factors, no
g-vectors -- so that the device's factorised form is checked against something that does not share it.  The `fault` argument
injects the three mistakes the host test must catch.
"""
import numpy as np


def _ell(ell, D):
    ell = np.atleast_1d(np.asarray(ell, dtype=np.float64))
    return np.full(D, ell[0]) if ell.size == 1 else ell


def psi1_node(Xu, sigma2, ell, m, S, fault=None):
    Xu = np.asarray(Xu, dtype=np.float64)
    D = Xu.shape[1]
    lam = _ell(ell, D) ** 2
    S = np.zeros((D, D)) if S is None else np.asarray(S, dtype=np.float64).reshape(D, D)
    det = 1.0 if fault == "no_det" else np.linalg.det(np.eye(D) + S / lam[:, None]) ** -0.5
    diff = np.asarray(m, dtype=np.float64).ravel()[None, :] - Xu                    # (M, D)
    sol = np.linalg.solve(np.diag(lam) + S, diff.T).T
    return sigma2 * det * np.exp(-0.5 * np.einsum("md,md->m", diff, sol))


def psi2_node(Xu, sigma2, ell, m, S, fault=None):
    Xu = np.asarray(Xu, dtype=np.float64)
    M, D = Xu.shape
    lam = _ell(ell, D) ** 2
    S = np.zeros((D, D)) if S is None else np.asarray(S, dtype=np.float64).reshape(D, D)
    c = 1.0 if fault == "drop2" else 2.0
    det = 1.0 if fault == "no_det" else np.linalg.det(np.eye(D) + c * S / lam[:, None]) ** -0.5
    dz = Xu[:, None, :] - Xu[None, :, :]
    e1 = -0.25 * np.einsum("abd,abd->ab", dz, dz / lam)
    zbar = np.broadcast_to(Xu[:, None, :], (M, M, D)) if fault == "zbar" else 0.5 * (Xu[:, None, :] + Xu[None, :, :])
    diff = (np.asarray(m, dtype=np.float64).ravel()[None, None, :] - zbar).reshape(M * M, D)
    sol = np.linalg.solve(np.diag(lam) + c * S, diff.T).T
    e2 = -np.einsum("nd,nd->n", diff, sol).reshape(M, M)
    return sigma2 ** 2 * det * np.exp(e1 + e2)


def psi_stats(Xu, sigma2, ell, mean, cov=None, node_weight=None, fault=None):
    """psi1 (T, M) and psi2 (M, M) = sum_t w_t Psi2_t of T inputs N(mean[t], cov[t]) (cov None: all zero)."""
    mean = np.asarray(mean, dtype=np.float64)
    T = mean.shape[0]
    M = np.asarray(Xu).shape[0]
    psi1, psi2 = np.zeros((T, M)), np.zeros((M, M))
    for t in range(T):
        S = None if cov is None else cov[t]
        psi1[t] = psi1_node(Xu, sigma2, ell, mean[t], S, fault)
        w = 1.0 if node_weight is None else float(node_weight[t])
        if w != 0.0:
            psi2 += w * psi2_node(Xu, sigma2, ell, mean[t], S, fault)
    return psi1, 0.5 * (psi2 + psi2.T)


def exact_suff_stats(Xu, sigma2, ell, mean, cov, Y, y_var=None, cov_sum=None):
    """The statistics of an exact sweep, packed as the oracle's update functions take them: (oracle.sgp_oracle.SuffStats,
    oracle.sgp_oracle.MultiStats) of Psi2 = sum_t Psi2_t, B = sum_t Psi1_t y_t', S_W = S_N = T, Ryy = sum_t y_t y_t' (+ sum_t var_t
    for d_out = 1, + the output-covariance sum)."""
    from oracle import sgp_oracle as O
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    T = Y.shape[0]
    psi1, psi2 = psi_stats(Xu, sigma2, ell, mean, cov)
    Ryy = Y.T @ Y
    if y_var is not None:
        Ryy = Ryy + np.sum(y_var)
    if cov_sum is not None:
        Ryy = Ryy + np.asarray(cov_sum, dtype=np.float64)
    B = psi1.T @ Y
    return (O.SuffStats(psi2, B, Ryy, float(sigma2 * T), float(T)), O.MultiStats(psi2, B, Ryy, float(sigma2 * T), float(T)))


# ------------------------------------------------------------------------------------------------
# the GP-SSM schedule with exact statistics: train.vmp_gpssm(psi="exact")
def vmp_gpssm_exact_ref(sigma2, ell, y, Xu, *, P, x0_prior, v_prior_var, w_prior, iterations, jitter, displace_out=False):
    """tests/gpssm_ref.vmp_gpssm_ref with the cubature sums of steps 1 (the :out means) and 4 (the :v statistics, which step 5 and
    the energy read again) replaced by psi1_node / psi2_node of q(x_{t-1}); steps 2, 3 and 5 as they stand there (step 3's closure
    stays on srcubature points).  displace_out: every :out mean displaced by + 50 eps |Psi1|' |mu_v^(d)|, its rounding bound."""
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, WishartFast
    from tests import gpssm_ref as GR
    import math
    sr = srcubature()
    y = np.asarray(y, dtype=np.float64)
    T, d = y.shape
    M = len(Xu)
    Qv = d * M
    m0, P0 = x0_prior
    nu0, invS0 = float(w_prior[0]), np.asarray(w_prior[1], dtype=np.float64)
    Pinv = np.linalg.inv(P)
    Kinv = np.linalg.inv(GR.kernel("se", sigma2, ell, Xu, Xu) + jitter * np.eye(M))
    Kinv = 0.5 * (Kinv + Kinv.T)
    q_x = [MvNormalMeanCovariance(np.array(m0), np.array(P0))] + [MvNormalMeanCovariance(np.zeros(d), 50.0 * np.eye(d)) for _ in range(T)]
    mu_v, Sig_v = np.zeros(Qv), v_prior_var * np.eye(Qv)
    q_w = WishartFast(nu0, invS0.copy())
    fe = []
    for _ in range(iterations):
        W = q_w.mean()
        E_logdet = GR.wishart_mean_logdet(q_w.nu, q_w.invS)
        mus = mu_v.reshape(d, M)
        outs = np.empty((T, d))                                                        # 1
        for t in range(T):
            p1 = psi1_node(Xu, sigma2, ell, q_x[t].m, q_x[t].S)
            outs[t] = mus @ p1
            if displace_out:
                outs[t] += 50 * GR.EPS * (np.abs(mus) @ np.abs(p1))
        S = np.linalg.inv(W + Pinv)                                                    # 2
        S = 0.5 * (S + S.T)
        lefts = [MvNormalMeanCovariance(np.array(m0), np.array(P0))] + [MvNormalMeanCovariance(S @ (W @ outs[t] + Pinv @ y[t]), S) for t in range(T)]
        Rv = Sig_v + np.outer(mu_v, mu_v)                                              # 3
        S_W = sum(W[i, j] * Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] for i in range(d) for j in range(d))
        S_W = 0.5 * (S_W + S_W.T)
        trW = float(np.trace(W))
        new_x = []
        for t in range(T):
            pts, w = sr.points_weights(lefts[t].m, lefts[t].S)
            K = GR.kernel("se", sigma2, ell, Xu, pts)
            s_t = mus.T @ (q_x[t + 1].m @ W)
            lp = np.array([-0.5 * trW * (sigma2 - k @ Kinv @ k) + s_t @ k - 0.5 * k @ S_W @ k for k in K.T])
            if GR.moments_are_nan(lp):
                new_x.append(lefts[t])
                continue
            g = w * np.exp(lp - lp.max())
            mean = (g @ pts) / g.sum()
            dv = pts - mean
            new_x.append(MvNormalMeanCovariance(mean, (dv * g[:, None]).T @ dv / g.sum()))
        q_x = new_x + [lefts[T]]
        Psi2s, B, stats = np.zeros((M, M)), np.zeros((M, d)), []                       # 4
        for t in range(T):
            Psi1, Psi2 = psi1_node(Xu, sigma2, ell, q_x[t].m, q_x[t].S), psi2_node(Xu, sigma2, ell, q_x[t].m, q_x[t].S)
            stats.append((sigma2, Psi1, Psi2))
            Psi2s += Psi2
            B += np.outer(Psi1, q_x[t + 1].m)
        Lam = np.eye(Qv) / v_prior_var + np.kron(W, Psi2s)
        Sig_v = np.linalg.inv(Lam)
        Sig_v = 0.5 * (Sig_v + Sig_v.T)
        mu_v = Sig_v @ (B @ W).T.reshape(-1)
        Rv = Sig_v + np.outer(mu_v, mu_v)                                              # 5 and the energy
        mus = mu_v.reshape(d, M)
        invS_sum, energy = np.zeros((d, d)), 0.0
        for t in range(T):
            Psi0, Psi1, Psi2 = stats[t]
            my, Sy = q_x[t + 1].m, q_x[t + 1].S
            I1 = (Psi0 - np.sum(Kinv * Psi2)) * np.eye(d)
            E = mus @ Psi1
            Psi4 = np.array([[np.sum(Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] * Psi2) for j in range(d)] for i in range(d)])
            tmp = np.outer(my, E)
            inv_t = Psi4 + np.outer(my, my) + Sy - (tmp + tmp.T) + I1
            invS_sum += inv_t
            energy += 0.5 * d * math.log(2 * math.pi) - 0.5 * E_logdet + 0.5 * np.trace(W @ inv_t)
        fe.append(energy + GR.host_energy(y, P, q_x, mu_v, Sig_v, q_w, x0_prior, v_prior_var, (nu0, invS0)))
        q_w = WishartFast(nu0 + T, invS0 + invS_sum)
    return dict(q_x=q_x, q_v=MvNormalMeanCovariance(mu_v, Sig_v), q_w=q_w, fe=fe)


GPSSM = dict(T=12, M=10, seed=31, sigma2=1.0, ell=np.array([0.8, 1.0]), jitter=1e-6)


def gpssm_inducing():
    """10 inducing inputs on a 2 x 5 grid over [-1.5, 1.5] x [-4, 4]."""
    return np.array([[a, b] for a in (-1.5, 1.5) for b in np.linspace(-4.0, 4.0, 5)])


_GPSSM_RUNS = {}


def gpssm_reference(iterations):
    """(y, Xu, plain run, run with the :out means displaced by + their bounds) of the exact-schedule case, once per process."""
    from tests import gpssm_ref as GR
    if iterations not in _GPSSM_RUNS:
        p = GPSSM
        _, y = GR.pendulum(p["T"], p["seed"])
        Xu = gpssm_inducing()
        kw = dict(P=GR.P_OBS, x0_prior=GR.X0_PRIOR, iterations=iterations, jitter=p["jitter"], **GR.TEST_PRIORS)
        _GPSSM_RUNS[iterations] = (y, Xu, vmp_gpssm_exact_ref(p["sigma2"], p["ell"], y, Xu, **kw),
                                   vmp_gpssm_exact_ref(p["sigma2"], p["ell"], y, Xu, displace_out=True, **kw))
    return _GPSSM_RUNS[iterations]
