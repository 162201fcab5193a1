"""NumPy restatement of sgp_vmp_run_t (include/sgp_hip.h), written from its formulas and independent of the library: K coordinate
updates of q(v), q(w) and the q(tau_i) of `y_i ~ N(f_i, 1 / (w tau_i)), tau_i ~ Gamma(nu / 2, nu / 2), f_i ~ UniSGP(x_i, v, ., theta)`
with the free energy after each.  The kernel, the factorisations, the prior forms and the special functions are tests/vmp_ref.py's.

`dtype=np.longdouble` runs the same code in extended precision; `displace` moves Psi2, B and w relatively by that much at every
iteration; `mutant` seeds one of the faults the tolerances must see (tests/test_vmp_t_host.py)."""
import numpy as np

from tests import vmp_ref as R

LOG2PI = R.LOG2PI
MUTANTS = ("old_w_rates", "sweep_scalar_energy", "no_elog_tau", "last_block_dropped")
BLOCK = 256                                                  # points per workgroup of k_t_points
EPS = np.finfo(np.float64).eps


def make_outlier_toy(N, M, seed, frac=0.05, shift=20.0, noise=0.1):
    """y = sin(2 x) + noise on [-1.7, 1.7], with `frac` of the targets displaced by `shift` noise standard deviations.
    Returns (X, y, Xu, clean mask, the noise-free function values)."""
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-1.7, 1.7, (N, 1)), axis=0)
    f = np.sin(2.0 * X[:, 0])
    y = f + noise * rng.normal(size=N)
    bad = rng.permutation(N)[:max(1, int(round(frac * N)))]
    y[bad] += shift * noise * np.where(rng.uniform(size=bad.size) < 0.8, 1.0, -1.0)
    clean = np.ones(N, dtype=bool)
    clean[bad] = False
    Xu = np.linspace(-1.7, 1.7, M)[:, None]
    return X, y, Xu, clean, f


def gamma_kl(a, b, a0, b0, digamma, gammaln):
    """KL(Gamma(a, b) || Gamma(a0, b0)), shape / rate, in the form the header gives for q(w)"""
    return (a - a0) * digamma(a) - gammaln(a) + gammaln(a0) + a0 * (np.log(b) - np.log(b0)) + a * (b0 - b) / b


def vmp_run_t_ref(X, y, Xu, s2, ell, jitter, prior, iterations, nu, *, gamma_prior=(1e-2, 1e-2), gamma=None, tau_rate=None,
                  hold_w=None, family="se", dtype=np.float64, displace=0.0, mutant=None):
    """Returns dict(mu, Sigma, gamma, tau_rate, omega (the last sweep's weights), values, terms (K, 4), r (the last r_i))."""
    t = dtype
    X, y, Xu = (np.asarray(v, dtype=t) for v in (X, y, Xu))
    N, M = X.shape[0], Xu.shape[0]
    digamma, gammaln, _ = R._special(t)
    Kuu = R.kernel(Xu, Xu, t(s2), ell, family) + t(jitter) * np.eye(M, dtype=t)
    Kuf = R.kernel(Xu, X, t(s2), ell, family)
    Kinv, _ = R._inv_logdet(Kuu)
    L0, xi0, mu0, ld0 = R.prior_natural(prior, M, t)
    a0, b0 = (t(gamma_prior[0]), t(gamma_prior[1])) if hold_w is None else (t(1), t(1))
    a, b = (a0, b0) if gamma is None else (t(gamma[0]), t(gamma[1]))
    alpha, hn = (t(nu) + 1) / 2, t(nu) / 2
    beta = np.full(N, alpha, dtype=t) if tau_rate is None else np.asarray(tau_rate, dtype=t).copy()
    psi_a = digamma(alpha)
    I1 = t(s2) - np.einsum("mn,mn->n", Kuf, Kinv @ Kuf)       # per point, fixed for the run
    values, terms = [], []
    for k in range(iterations):
        w, elog = (a / b, digamma(a) - np.log(b)) if hold_w is None else (t(hold_w[0]), t(hold_w[1]))
        wd = w * (1 + t(displace))
        om = alpha / beta
        P2 = ((Kuf * om) @ Kuf.T) * (1 + t(displace))
        B = (Kuf @ (om * y)) * (1 - t(displace))
        Sigma, ldL = R._inv_logdet(L0 + wd * P2)
        mu = Sigma @ (xi0 + wd * B)
        Rv = Sigma + np.outer(mu, mu)
        r = I1 + (y * y - 2 * y * (Kuf.T @ mu) + np.einsum("mn,mn->n", Kuf, Rv @ Kuf))
        # sum I1 + sum I2 of the sweep at the weights it ran at, from the statistics as the sweep forms them (tests/vmp_ref.py): a
        # difference of traces, which feels the rounding of Psi2 and B; the per-point r_i above are k_w_point_finish's, from K_uf
        S = (t(s2) * om.sum() - np.sum(Kinv * P2)) + (np.sum(om * y * y) - 2 * B @ mu + np.sum(Rv * P2))
        t3 = t(0)
        if hold_w is None:
            a, b = a0 + t(N) / 2, b0 + S / 2
            w, elog = a / b, digamma(a) - np.log(b)
            t3 = gamma_kl(a, b, a0, b0, digamma, gammaln)
        beta = hn + (wd if mutant == "old_w_rates" else w) * r / 2
        e = (alpha / beta) * r
        li = gamma_kl(alpha, beta, hn, hn, digamma, gammaln) - (0 if mutant == "no_elog_tau" else (psi_a - np.log(beta)) / 2)
        if mutant == "last_block_dropped":
            keep = (N - 1) // BLOCK * BLOCK
            e, li = e[:keep], li[:keep]
        t0 = (w * (S if mutant == "sweep_scalar_energy" else e.sum()) - N * elog + N * t(LOG2PI)) / 2
        lik = li.sum()
        d = mu - mu0
        t2 = (np.sum(L0 * Sigma) + d @ L0 @ d - M - ld0 + ldL) / 2
        terms.append([t0, lik, t2, t3])
        values.append(((t0 + lik) + t2) + t3)
    return dict(mu=mu, Sigma=Sigma, gamma=(a, b), tau_rate=beta, omega=om, r=r, values=np.array(values, dtype=t),
                terms=np.array(terms, dtype=t))


def tolerances(P, K, nu, **kw):
    """(the float64 restatement of a K-iteration run, per-quantity tolerance) by the rule of tests/test_gpu_vmp_run.py: 10 x the larger
    of the float64-vs-extended difference and the change under a relative displacement of Psi2, B and w by 50 eps per iteration"""
    args = (P["X"], P["y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], K, nu)
    kw = dict(family=P.get("family", "se"), gamma_prior=P.get("g0", (1e-2, 1e-2)), hold_w=P.get("hold"), **kw)
    ref = vmp_run_t_ref(*args, **kw)
    ext = vmp_run_t_ref(*args, dtype=np.longdouble, **kw)
    dis = vmp_run_t_ref(*args, displace=50 * EPS, **kw)
    tol = {}
    for q in ("values", "terms", "mu", "Sigma", "tau_rate"):
        worst = np.maximum(np.abs(np.asarray(ext[q], dtype=np.float64) - ref[q]), np.abs(dis[q] - ref[q]))
        tol[q] = 10 * (worst.max(axis=0) if q == "terms" else worst.max())
    tol["gamma"] = 10 * max(abs(float(ext["gamma"][1]) - ref["gamma"][1]), abs(dis["gamma"][1] - ref["gamma"][1]))
    return ref, tol


# ---- the ledger of exported names (tests/call_sequence_ref.ENTRY_POINTS; tests/test_call_sequences_host.py holds it to the header).
# sgp_vmp_run_t sweeps and rewrites q(v), the noise, the point weights, the weighted targets and the data scalars: a mutator.  What it
# leaves is held to the host-paced sequence by tests/test_gpu_vmp_t.py (test_state_afterwards, test_against_the_host_paced_loop).
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_vmp_run_t", CR.MUTATOR)


register_entry_point()
