"""NumPy restatement of sgp_vmp_run_w (include/sgp_hip.h), written from its formulas and independent of the library: K coordinate
updates of q(v) and q(W) of `y_t ~ MultiSGP(x_t, v, W, theta), W ~ Wishart(nu0, R0^-1)` with the free energy after each.

The float64 run is built from oracle.sgp_oracle (multi_suff_stats for the SE kernel, multi_v_update, multi_w_update, cholinv) and
SciPy's digamma / gammaln.  `dtype=np.longdouble` runs the same formulas in extended precision (tests/vmp_ref's own Cholesky and,
where mpmath is installed, its psi and lgamma): the float64-vs-extended difference is the floor of every tolerance of
tests/test_gpu_vmp_w.py.  `displace` moves Psi2, B and W_bar relatively by that much at every iteration, as tests/vmp_ref.py does;
`displace_w` moves W_bar alone; `mutant` seeds one of the faults the checks of tests/test_vmp_w_host.py must tell apart.

A problem is given by nodes: points (T, S, D) with weights (T, S) -- S = 1 and weight 1 for PointMass inputs, the cubature points of a
held q(x_t) otherwise --, targets Y (T, d) and, optionally, the sum over the nodes of the targets' covariances (d, d)."""
import numpy as np

from oracle import sgp_oracle as O
from tests import vmp_ref as R

LOG2PI = R.LOG2PI
MUTANTS = ("nu_half_n", "elogdet_no_dlog2", "energy_old_qw")


def make_problem(T, S, M, D, d, seed, noise=0.1):
    """T nodes of S weighted points each around a centre in [-1.7, 1.7]^D, d outputs sin / cos of the inputs' sum with noise that is
    correlated between the outputs; Xu drawn from the same box (as many from the centres as there are)."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(-1.7, 1.7, (T, D))
    if S == 1:
        pts, wts = C[:, None, :], np.ones((T, 1))
    else:
        pts = C[:, None, :] + 0.15 * rng.normal(size=(T, S, D))
        wts = rng.uniform(0.5, 1.5, (T, S))
        wts /= wts.sum(axis=1, keepdims=True)
    s = C.sum(axis=1)
    F = np.stack([np.sin(s + 0.7 * j) * (1.0 + 0.3 * j) for j in range(d)], axis=1)
    A = np.eye(d) + 0.4 * rng.normal(size=(d, d))
    Y = F + noise * rng.normal(size=(T, d)) @ A.T
    Xu = np.concatenate([C[rng.permutation(T)[:min(M, T)]], rng.uniform(-1.7, 1.7, (max(M - T, 0), D))])
    return pts, wts, Y, Xu


def flat(pts, wts, Y):
    """the nodes as sgp_set_data takes them: X (T S, D), y (T S, d), pt_weight (T S) or None, n_nodes or None"""
    T, S, D = pts.shape
    if S == 1:
        return pts.reshape(T, D), Y, None, None
    return pts.reshape(T * S, D), np.repeat(Y, S, axis=0), wts.reshape(T * S), T


def suff_stats(Xu, pts, wts, Y, cov_sum, s2, ell, family="se", dtype=np.float64):
    """oracle.MultiStats of the nodes; the SE kernel in float64 through oracle.multi_suff_stats itself"""
    T, S, D = pts.shape
    if dtype == np.float64 and family == "se":
        ms = O.multi_suff_stats(Xu, pts, wts, Y, None, s2, ell)
        if cov_sum is not None:
            ms.Ryy = ms.Ryy + np.asarray(cov_sum, dtype=np.float64)
        return ms
    t = dtype
    Xu, X, w, Y = (np.asarray(v, dtype=t) for v in (Xu, pts.reshape(T * S, D), wts.reshape(T * S), Y))
    K = R.kernel(Xu, X, t(s2), np.asarray(ell, dtype=t), family)
    Psi1 = (K * w).reshape(K.shape[0], T, S).sum(axis=2)
    Ryy = Y.T @ Y
    if cov_sum is not None:
        Ryy = Ryy + np.asarray(cov_sum, dtype=t)
    return O.MultiStats((K * w) @ K.T, Psi1 @ Y, Ryy, t(s2) * w.sum(), t(T))


def logdet(A):
    return 2 * np.log(np.diag(R._chol(A))).sum()


def wishart_mean_logdet(nu, Rm, digamma, d_log2=True):
    """(W_bar, E[logdet W]) of Wishart(nu, R^-1), W_bar exactly symmetric"""
    d = Rm.shape[0]
    Ri, ldr = R._inv_logdet(Rm)
    Ri = (Ri + Ri.T) / 2
    el = sum(digamma(0.5 * (nu - i)) for i in range(d)) + (d * np.log(Rm.dtype.type(2)) if d_log2 else 0) - ldr
    return nu * Ri, el


def wishart_kl(nu, Rm, nu0, R0, digamma, gammaln):
    """KL(Wishart(nu, R^-1) || Wishart(nu0, R0^-1)), both by their inverse scales; lnGamma_d's d (d - 1) / 4 log pi cancel"""
    d = Rm.shape[0]
    Ri, ldr = R._inv_logdet(Rm)
    lg = lambda a: sum(gammaln(a - 0.5 * i) for i in range(d))
    psis = sum(digamma(0.5 * (nu - i)) for i in range(d))
    return (0.5 * nu0 * (ldr - logdet(R0)) + 0.5 * nu * (np.sum(R0 * Ri) - d) + lg(0.5 * nu0) - lg(0.5 * nu)
            + 0.5 * (nu - nu0) * psis)


def node_energy(Wbar, elog, S, N):
    """sum over the nodes of @average_energy at q(v) (through S) and q(W)"""
    d = S.shape[0]
    return 0.5 * (np.sum(Wbar * S) - N * elog + N * d * S.dtype.type(LOG2PI))


def vmp_run_w_ref(pts, wts, Y, Xu, s2, ell, jitter, prior, iterations, *, w_prior=None, wishart=None, hold_w=None, cov_sum=None,
                  family="se", dtype=np.float64, displace=0.0, displace_w=0.0, mutant=None):
    """prior: tests/vmp_ref.prior_natural's forms over Q = d M; w_prior = (nu0, R0), wishart = (nu, R) entering the run (default the
    prior); hold_w = (W_bar, E[logdet W]) holds q(W).  Returns dict(mu, Sigma, nu, R, Wbar, elog, S, values, terms (K, 4), qv)."""
    t = dtype
    pts, wts, Y, Xu = (np.asarray(v, dtype=np.float64) for v in (pts, wts, Y, Xu))
    M, d = Xu.shape[0], Y.shape[1]
    Q = d * M
    digamma, gammaln, _ = R._special(t)
    ms = suff_stats(Xu, pts, wts, Y, cov_sum, s2, ell, family, t)
    Xt = np.asarray(Xu, dtype=t)
    Kuu = R.kernel(Xt, Xt, t(s2), np.asarray(ell, dtype=t), family) + t(jitter) * np.eye(M, dtype=t)
    Kinv = O.cholinv(Kuu) if t == np.float64 else R._inv_logdet(Kuu)[0]
    L0, xi0, mu0, ld0 = R.prior_natural(prior, Q, t)
    N = t(ms.n)
    if hold_w is None:
        nu0, R0 = t(w_prior[0]), np.asarray(w_prior[1], dtype=t)
        nu, Rm = (nu0, R0) if wishart is None else (t(wishart[0]), np.asarray(wishart[1], dtype=t))
    else:
        nu, Rm = None, None
    values, terms, qv = [], [], []
    for k in range(iterations):
        if hold_w is None:
            Wbar, elog = wishart_mean_logdet(nu, Rm, digamma, d_log2=mutant != "elogdet_no_dlog2")
        else:
            Wbar, elog = np.asarray(hold_w[0], dtype=t), t(hold_w[1])
        Wd = Wbar * (1 + t(displace)) * (1 + t(displace_w))
        sk = O.MultiStats(ms.Psi2 * (1 + t(displace)), ms.B * (1 - t(displace)), ms.Ryy, ms.s_kk, ms.n)
        if t == np.float64:
            mu, Sigma = O.multi_v_update(sk, Wd, L0, xi0)
            ldL = np.linalg.slogdet(L0 + np.kron(Wd, sk.Psi2))[1]
        else:
            Sigma, ldL = R._inv_logdet(L0 + np.kron(Wd, sk.Psi2))
            mu = Sigma @ (xi0 + (sk.B @ Wd).T.reshape(-1))
        S = O.multi_w_update(sk, mu, Sigma, Kinv)
        W_old, elog_old, t3 = Wd, elog, t(0)
        if hold_w is None:
            nu, Rm = nu0 + (N / 2 if mutant == "nu_half_n" else N), R0 + S
            Wbar, elog = wishart_mean_logdet(nu, Rm, digamma, d_log2=mutant != "elogdet_no_dlog2")
            t3 = wishart_kl(nu, Rm, nu0, R0, digamma, gammaln)
        t0 = node_energy(W_old, elog_old, S, N) if mutant == "energy_old_qw" else node_energy(Wbar, elog, S, N)
        dm = mu - mu0
        t2 = 0.5 * (np.sum(L0 * Sigma) + dm @ L0 @ dm - Q - ld0 + ldL)
        terms.append([t0, t(0), t2, t3])
        values.append(((t0 + t(0)) + t2) + t3)
        qv.append((mu.copy(), Sigma.copy()))
    return dict(mu=mu, Sigma=Sigma, nu=nu, R=Rm, Wbar=Wbar, elog=elog, S=S, values=np.array(values, dtype=t),
                terms=np.array(terms, dtype=t), qv=qv)


# ---- the ledger of exported names (tests/call_sequence_ref.ENTRY_POINTS; tests/test_call_sequences_host.py holds it to the header).
# sgp_vmp_run_w sweeps and rewrites q(v) and the noise: a mutator, as sgp_vmp_run is; what it leaves is held to the host-paced
# sequence by tests/test_gpu_vmp_w.py (test_state_equals_the_host_paced_sequence).
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_vmp_run_w", CR.MUTATOR)


register_entry_point()
