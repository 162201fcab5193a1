"""NumPy restatement of sgp_vmp_run (include/sgp_hip.h), written from its formulas and independent of the library: K coordinate
updates of q(f) (Probit), q(v) and q(w) of `f[i] ~ UniSGP(x[i], v, w, theta)` with the free energy after each.

`dtype=np.longdouble` runs the same code in extended precision (own Cholesky; psi, lgamma and log Phi through mpmath where it is
installed): the float64-vs-extended difference is the floor of every tolerance of tests/test_gpu_vmp_run.py.  `displace` moves Psi2,
B and w relatively by that much at every iteration (the sensitivity rule of tests/test_gpu_gpssm.py); `mutant` seeds one of the
faults the tolerances must see; `displace_w` moves w alone (the rule of the comparison with the host-paced loop).

The mutant "vz_new_w" takes vz = 1 / mean(q_w) from the q(w) of step 3 of the SAME iteration where the Probit factors' share is
evaluated.  (In the forward message itself the two readings cannot differ from iteration 1 on: the q(w) that enters iteration k is
the one step 3 of iteration k - 1 left.  What can go wrong is the term of the free energy: it belongs to the tilted q(f), which was
formed at the entering vz, and a closing stage that evaluates it at the noise it has just written gets another number.)"""
import numpy as np

try:
    import mpmath
except ImportError:                                          # pragma: no cover
    mpmath = None
from scipy import special

LOG2PI = np.log(2.0 * np.pi)
FORMULA_MUTANTS = ("elogw_pointmass", "energy_old_qw", "drop_M", "logdet0_sign", "last_block_lik", "vz_new_w")
# one fault per branch of the three kernels that only a shape beyond the first workgroup (or the first pass, or the asymptotic range)
# reaches; each is invisible, bitwise, at the shapes below those thresholds (tests/test_vmp_host.py)
BRANCH_MUTANTS = ("kl_iso_tail", "kl_dense_tail", "reduce_tail", "digamma_no_recurrence", "log_ndtr_naive")
MUTANTS = FORMULA_MUTANTS + BRANCH_MUTANTS
KL_BLOCK = 256                                               # entries per workgroup (isotropic prior) / rows per pass (dense) of k_vmp_kl
REDUCE_PASS = 256 * 256                                      # points behind one pass of the reduce stage: 256 pairs of 256 points


def make_toy(N, M, D, seed, probit=False):
    """The `fe`-style toys: y = sin(sum x) + noise, labels by thresholding; Xu a subset of X."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    f = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    return X, ((f > 0).astype(np.float64) if probit else f), Xu


def kernel(A, B, s2, ell, family="se"):
    ell = np.broadcast_to(np.asarray(ell, dtype=A.dtype), (A.shape[1],))
    a, b = A / ell, B / ell
    s = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    if family == "se":
        return s2 * np.exp(-s / 2)
    r = np.sqrt(s)
    if family == "matern12":
        return s2 * np.exp(-r)
    if family == "matern32":
        return s2 * (1 + np.sqrt(A.dtype.type(3)) * r) * np.exp(-np.sqrt(A.dtype.type(3)) * r)
    if family == "matern52":
        return s2 * (1 + np.sqrt(A.dtype.type(5)) * r + 5 * s / 3) * np.exp(-np.sqrt(A.dtype.type(5)) * r)
    raise ValueError(family)


def _chol(A):
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _tri_inv(L):
    """inverse of a lower-triangular matrix by forward substitution"""
    if L.dtype == np.float64:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, np.eye(L.shape[0]), lower=True)
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        W[i, i] = 1 / L[i, i]
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
    return W


def _inv_logdet(A):
    L = _chol(A)
    W = _tri_inv(L)
    return W.T @ W, 2 * np.log(np.diag(L)).sum()


def _special(dtype):
    if dtype == np.float64 or mpmath is None:
        return special.digamma, special.gammaln, special.log_ndtr
    mpmath.mp.dps = 40
    f = lambda fn: (lambda x: np.vectorize(lambda v: np.longdouble(str(fn(mpmath.mpf(float(v)) if not isinstance(v, np.longdouble)
                                                                      else mpmath.mpf(str(v))))), otypes=[np.longdouble])(x))
    return f(mpmath.digamma), f(mpmath.loggamma), f(lambda g: mpmath.log(mpmath.ncdf(g)))


def digamma_asymptotic(x):
    """log x - 1 / (2 x) - sum_k B_2k / (2 k x^2k) through x^-14, with no recurrence in front of it (the mutant "digamma_no_recurrence")"""
    i2 = 1 / (x * x)
    s = i2 * (1 / 12 - i2 * (1 / 120 - i2 * (1 / 252 - i2 * (1 / 240 - i2 * (1 / 132 - i2 * (691 / 32760 - i2 / 12))))))
    return np.log(x) - 0.5 / x - s


def log_ndtr_naive(g):
    """log Phi(g) as log(erfc(-g / sqrt 2) / 2) in both tails (the mutant "log_ndtr_naive": -inf below g = -38.5)"""
    with np.errstate(divide="ignore"):
        return np.log(0.5 * special.erfc(-np.asarray(g, dtype=np.float64) / np.sqrt(2.0)))


def probit_moments(y, mz, vz, log_ndtr):
    """(mf, vf, g) of the tilted q(f) ~ N(f; mz, vz) Phi(s f), s = 2 y - 1"""
    s = 2 * y - 1
    q = 1 / np.sqrt(1 + vz)
    g = s * mz * q
    r = np.exp(-g * g / 2 - LOG2PI / 2 - log_ndtr(g))
    return mz + s * vz * r * q, vz - vz * vz / (1 + vz) * r * (g + r), g


def probit_lik(mz, vz, mf, vf, g, log_ndtr):
    """per point: E_q[log q(f) - log Phi(s f)] = -1/2 log(2 pi vz) - ((mf - mz)^2 + vf) / (2 vz) - log Phi(g)"""
    return -0.5 * np.log(2 * np.pi * vz) - ((mf - mz) ** 2 + vf) / (2 * vz) - log_ndtr(g)


def prior_natural(prior, M, dtype=np.float64):
    """(Lambda0, xi0, mu0, log|Lambda0|) of ("iso", s) | ("meancov", mu0, Sigma0) | ("precision", xi0, Lambda0)"""
    if prior[0] == "iso":
        s = dtype(prior[1])
        return np.eye(M, dtype=dtype) / s, np.zeros(M, dtype=dtype), np.zeros(M, dtype=dtype), -M * np.log(s)
    if prior[0] == "meancov":
        mu0, S0 = np.asarray(prior[1], dtype=dtype), np.asarray(prior[2], dtype=dtype)
        L0, ld = _inv_logdet(S0)
        return L0, L0 @ mu0, mu0, -ld
    xi0, L0 = np.asarray(prior[1], dtype=dtype), np.asarray(prior[2], dtype=dtype)
    S0, ld = _inv_logdet(L0)
    return L0, xi0, S0 @ xi0, ld


def vmp_run_ref(X, y, Xu, s2, ell, jitter, prior, iterations, *, likelihood="gaussian", gamma_prior=(1e-2, 1e-2), gamma=None,
                mu_init=None, hold_w=None, family="se", dtype=np.float64, displace=0.0, displace_w=0.0, mutant=None):
    """hold_w = (w, E[log w]) holds q(w).  Returns dict(mu, Sigma, gamma, values, terms (K, 4), mus)."""
    t = dtype
    X, y, Xu = (np.asarray(v, dtype=t) for v in (X, y, Xu))
    N, M = X.shape[0], Xu.shape[0]
    digamma, gammaln, log_ndtr = _special(t)
    Kuu = kernel(Xu, Xu, t(s2), ell, family) + t(jitter) * np.eye(M, dtype=t)
    Kuf = kernel(Xu, X, t(s2), ell, family)
    Kinv, _ = _inv_logdet(Kuu)
    Psi2 = Kuf @ Kuf.T
    L0, xi0, mu0, ld0 = prior_natural(prior, M, t)
    if mutant == "logdet0_sign":
        ld0 = -ld0
    a0, b0 = (t(gamma_prior[0]), t(gamma_prior[1])) if hold_w is None else (t(1), t(1))
    a, b = (a0, b0) if gamma is None else (t(gamma[0]), t(gamma[1]))
    mu = np.zeros(M, dtype=t) if mu_init is None else np.asarray(mu_init, dtype=t)
    probit = likelihood == "probit"
    values, terms, mus = [], [], []
    for k in range(iterations):
        w, elog = (a / b, digamma(a) - np.log(b)) if hold_w is None else (t(hold_w[0]), t(hold_w[1]))
        wd = w * (1 + t(displace)) * (1 + t(displace_w))
        lik = t(0)
        if probit:
            vz = 1 / wd
            mz = Kuf.T @ mu
            mf, vf, g = probit_moments(y, mz, vz, log_ndtr)
            li = probit_lik(mz, vz, mf, vf, g, log_ndtr_naive if mutant == "log_ndtr_naive" else log_ndtr)
            if mutant == "last_block_lik":
                li = li[:(N - 1) // 256 * 256] if N > 256 else li[:0]
            sq = mf * mf + vf
            if mutant == "reduce_tail" and N > REDUCE_PASS:      # the pairs of the second pass never arrive
                li, sq = li[:REDUCE_PASS], sq[:REDUCE_PASS]
            lik = li.sum()
            moments = (mz, mf, vf, g)
            tgt, syy = mf, sq.sum()
        else:
            tgt, syy = y, (y * y).sum()
        P2 = Psi2 * (1 + t(displace))
        B = (Kuf @ tgt) * (1 - t(displace))
        Sigma, ldL = _inv_logdet(L0 + wd * P2)
        mu = Sigma @ (xi0 + wd * B)
        I1 = t(s2) * N - np.sum(Kinv * P2)
        I2 = syy - 2 * B @ mu + np.sum((Sigma + np.outer(mu, mu)) * P2)
        S = I1 + I2
        w_old, elog_old = wd, elog
        t3 = t(0)
        if hold_w is None:
            a, b = a0 + t(N) / 2, b0 + S / 2
            psi = digamma_asymptotic(a) if mutant == "digamma_no_recurrence" and a < 10 else digamma(a)
            w, elog = a / b, (np.log(a / b) if mutant == "elogw_pointmass" else psi - np.log(b))
            t3 = (a - a0) * psi - gammaln(a) + gammaln(a0) + a0 * (np.log(b) - np.log(b0)) + a * (b0 - b) / b
        if probit and mutant == "vz_new_w":
            lik = probit_lik(moments[0], 1 / w, moments[1], moments[2], moments[3], log_ndtr).sum()
        we, ee = (w_old, elog_old) if mutant == "energy_old_qw" else (w, elog)
        t0 = 0.5 * (we * S - N * ee + N * t(LOG2PI))
        d = mu - mu0
        L0k = L0
        if M > KL_BLOCK and mutant == ("kl_iso_tail" if prior[0] == "iso" else "kl_dense_tail"):
            L0k = L0.copy()                                  # the diagonal entries resp. the rows of Lambda0 from 256 on never arrive
            L0k[KL_BLOCK:, :] = 0
        t2 = 0.5 * (np.sum(L0k * Sigma) + d @ L0k @ d - (0 if mutant == "drop_M" else M) - ld0 + ldL)
        terms.append([t0, lik, t2, t3])
        values.append(((t0 + lik) + t2) + t3)
        mus.append(mu.copy())
    return dict(mu=mu, Sigma=Sigma, gamma=(a, b), values=np.array(values, dtype=t), terms=np.array(terms, dtype=t), mus=mus)


# ---- the ledger of exported names --------------------------------------------------------------------------------------------
# tests/call_sequence_ref.ENTRY_POINTS classifies every exported sgp_* name (tests/test_call_sequences_host.py holds it to the header).
# sgp_vmp_run sweeps: it rewrites q(v), the noise and, for Probit, the resident targets, so it is a mutator; what it leaves is held to
# the host-paced sequence by tests/test_gpu_vmp_run.py (test_state_afterwards, test_state_equals_the_host_paced_sequence) and by the
# vmp_run_* entries of the call grid.  ENTRY_POINTS names it itself now; the registration below is kept and changes nothing.
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_vmp_run", CR.MUTATOR)


register_entry_point()
