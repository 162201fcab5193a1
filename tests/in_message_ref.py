"""NumPy restatement of the batched :in messages and their moment-matched marginals (sgp_in_message), on top of the oracle's
`multi_rule_in_logpdf`, `srcubature` and `ghcubature_1d`, with the fixtures and the error bounds the host and the GPU tests share.

Per point p of node t, k = K(Xu, x_p):
    logpdf_p = -1/2 tr(W) (sigma2 - k' Kuu^-1 k) + s_t . k - 1/2 k' S k,   s_t = sum_d mu_v^(d) (y_t' W)_d,
    S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)')
and its bound is the error model of tests/test_gpu_predict_var.py, one term per summand:
    tol_p = 50 eps [ 1/2 tr(W) cond(K_uu) sigma2 + 1/2 cond(S) k' S k + |k|' |s_t| ]
(the Q_ff term cancels: cond(K_uu) eps of its size sigma2; a Cholesky factor's backward error is cond(S) eps of the form; a dot
product's is eps |k|' |s|).  Per node, with a = max logpdf, g = w exp(logpdf - a):
    log_norm = a + log sum g,  mean = sum g x / sum g,  cov = sum g (x - mean)(x - mean)' / sum g,
and with tau = max_s tol_s, r = max_s |x_s - mean|: |d log_norm| <= 2 tau, |d mean| <= 4 tau r, |d cov| <= 8 tau r^2, each + 1e-13
relative for rounding -- first-order propagation of dg / g = d logpdf (d log_norm <= tau; d mean = sum g dl (x - mean) / sum g
<= 2 tau r as dl varies in [-tau, tau]; d cov likewise <= 2 tau r^2 plus the second-order shift of the mean), with a factor 2 of
margin."""
import contextlib
import math

import numpy as np

from oracle import sgp_oracle as O

EPS = np.finfo(np.float64).eps
LOG_DBL_MAX = math.log(np.finfo(np.float64).max)

# case -> (M, D, d_out, nodes, cubature ("sr", "gh" or points per node), jitter, sigma2, lengthscale range, seed, W scale, family)
CASES = {
    "a": dict(M=48, D=2, d_out=2, nodes=7, cub="sr", jitter=1e-8, seed=1),
    "b": dict(M=129, D=3, d_out=3, nodes=5, cub=7, jitter=1e-8, seed=2),
    "c": dict(M=70, D=1, d_out=1, nodes=4, cub="gh", jitter=1e-6, seed=3),
    "d": dict(M=200, D=5, d_out=4, nodes=3, cub=11, jitter=1e-8, seed=4),
    "e": dict(M=48, D=2, d_out=2, nodes=7, cub="sr", jitter=1e-8, seed=5, w_scale=500.0),
    "f": dict(M=48, D=2, d_out=2, nodes=7, cub="sr", jitter=1e-8, seed=6, family="matern32"),
}
SIGMA2 = 0.8
ELL = {1: (0.25, 0.25), 2: (0.7, 0.9), 3: (0.9, 1.3), 5: (1.8, 2.6)}     # lengthscales per input dimension: linspace(lo, hi, D)


@contextlib.contextmanager
def oracle_family(family):
    """The oracle's closures evaluate `family` inside the block: its kernelmatrix is replaced by the restatement the
    kernel-family tests use (tests/test_kernel_family_host.matern)."""
    if family in (None, "se"):
        yield
        return
    from tests.test_kernel_family_host import matern
    saved = O.kernelmatrix
    O.kernelmatrix = matern(family)
    try:
        yield
    finally:
        O.kernelmatrix = saved


def make_case(name):
    """The inputs of one case, by the recipe of the module's tests: Xu ~ U(-2, 2); Sigma_v = 0.02 A A' / Q + 0.01 I, mu_v = 0.3
    randn; W = B B' / d_out + I (times w_scale); node means ~ U(-1.5, 1.5), left covariances 0.05 (L L' / D + I); y ~ randn.
    Points: srcubature of the left message ("sr"), ghcubature(21) ("gh"), or that many points mean + chol(P) randn with weights
    ~ U(0.5, 1.5) normalised."""
    c = dict(CASES[name])
    M, D, d_out, T = c["M"], c["D"], c["d_out"], c["nodes"]
    rng = np.random.default_rng(c["seed"])
    Q = M * d_out
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    A = rng.normal(size=(Q, Q))
    Sigma_v = 0.02 * (A @ A.T) / Q + 0.01 * np.eye(Q)
    mu_v = 0.3 * rng.normal(size=Q)
    B = rng.normal(size=(d_out, d_out))
    W = (B @ B.T / d_out + np.eye(d_out)) * c.get("w_scale", 1.0)
    means = rng.uniform(-1.5, 1.5, (T, D))
    covs = []
    for _ in range(T):
        L = rng.normal(size=(D, D))
        covs.append(0.05 * (L @ L.T / D + np.eye(D)))
    Y = rng.normal(size=(T, d_out))
    pts, wts = [], []
    for t in range(T):
        if c["cub"] == "sr":
            p, w = O.srcubature(means[t], covs[t])
        elif c["cub"] == "gh":
            p, w = O.ghcubature_1d(21, float(means[t][0]), float(covs[t][0, 0]))
            p = p[:, None]
        else:
            S = int(c["cub"])
            p = means[t] + rng.normal(size=(S, D)) @ np.linalg.cholesky(covs[t]).T
            w = rng.uniform(0.5, 1.5, S)
            w /= w.sum()
        pts.append(np.asarray(p, dtype=np.float64))
        wts.append(np.asarray(w, dtype=np.float64))
    start = np.concatenate([[0], np.cumsum([len(w) for w in wts])]).astype(np.int64)
    lo, hi = ELL[D]
    c.update(Xu=Xu, Sigma_v=Sigma_v, mu_v=mu_v, W=W, means=means, covs=covs, Y=Y, X=np.concatenate(pts), wts=np.concatenate(wts),
             start=start, sigma2=SIGMA2, ell=np.linspace(lo, hi, D), family=c.get("family", "se"))
    return c


def contraction(mu_v, Sigma_v, W, M):
    """S = sum_ij W_ij (Sigma_v^(ij) + mu^(i) mu^(j)') (symmetrised) and the columns mu^(d) as an (M, d_out) array."""
    d_out = W.shape[0]
    Rv = Sigma_v + np.outer(mu_v, mu_v)
    S = sum(Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] * W[i, j] for i in range(d_out) for j in range(d_out))
    return 0.5 * (S + S.T), mu_v.reshape(d_out, M).T


def logpdf_and_bound(c, fault=None):
    """(logpdf (n,), tol (n,), diagnostics) of a case from the oracle's closure.  fault: None, "zero_y" (every node uses a zero
    row y' W) or "drop_tile" (the first 64-row tile of k is left out of k' S k)."""
    Xu, M = c["Xu"], c["M"]
    W, Y, start = c["W"], c["Y"], c["start"]
    with oracle_family(c["family"]):
        Kuu = O.kernelmatrix(c["sigma2"], c["ell"], Xu) + c["jitter"] * np.eye(M)
        Kinv = O.cholinv(Kuu)
        K = O.kernelmatrix(c["sigma2"], c["ell"], Xu, c["X"])                  # M x n
        S, mus = contraction(c["mu_v"], c["Sigma_v"], W, M)
        lp = np.empty(len(c["X"]))
        tol = np.empty(len(c["X"]))
        for t in range(len(Y)):
            y = np.zeros_like(Y[t]) if fault == "zero_y" else Y[t]
            f = O.multi_rule_in_logpdf(Xu, c["sigma2"], c["ell"], y, c["mu_v"], c["Sigma_v"], W, Kinv)
            s_t = mus @ (Y[t] @ W)
            for p in range(start[t], start[t + 1]):
                lp[p] = f(c["X"][p])
                k = K[:, p]
                kSk = float(k @ S @ k)
                if fault == "drop_tile":
                    kd = k.copy()
                    kd[:64] = 0.0
                    lp[p] += 0.5 * kSk - 0.5 * float(kd @ S @ kd)
                tol[p] = 50 * EPS * (0.5 * np.trace(W) * np.linalg.cond(Kuu) * c["sigma2"] + 0.5 * np.linalg.cond(S) * kSk
                                     + float(np.abs(k) @ np.abs(s_t)))
    return lp, tol, dict(cond_kuu=float(np.linalg.cond(Kuu)), cond_S=float(np.linalg.cond(S)))


def node_moments(X, wts, start, lp, shifted=True):
    """Per node (log_norm, mean, cov): the log-sum-exp-shifted moments, or (shifted=False) the reference's unshifted arithmetic
    (approximate_meancov over exp(logpdf)), which overflows to NaN where logpdf > log(DBL_MAX)."""
    T = len(start) - 1
    D = X.shape[1]
    log_norm, mean, cov = np.empty(T), np.empty((T, D)), np.empty((T, D, D))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(T):
            sl = slice(start[t], start[t + 1])
            a = float(lp[sl].max()) if shifted else 0.0
            g = wts[sl] * np.exp(lp[sl] - a)
            Z = g.sum()
            log_norm[t] = a + np.log(Z)
            mean[t] = (g @ X[sl]) / Z
            d = X[sl] - mean[t]
            cov[t] = (d * g[:, None]).T @ d / Z
    return log_norm, mean, cov


def moment_bounds(X, start, tol, log_norm, mean, cov):
    """(b_log_norm (T,), b_mean (T,), b_cov (T,)): absolute bounds per node, see the module docstring."""
    T = len(start) - 1
    b0, b1, b2 = np.empty(T), np.empty(T), np.empty(T)
    for t in range(T):
        sl = slice(start[t], start[t + 1])
        tau = float(tol[sl].max())
        r = float(np.linalg.norm(X[sl] - mean[t], axis=1).max())
        b0[t] = 2 * tau + 1e-13 * abs(log_norm[t])
        b1[t] = 4 * tau * r + 1e-13 * float(np.abs(mean[t]).max())
        b2[t] = 8 * tau * r * r + 1e-13 * float(np.abs(cov[t]).max())
    return b0, b1, b2


_cache = {}


def reference(name):
    """Everything the tests compare against for one case, computed once per process and not to be modified: the case's inputs,
    lp, tol, cond_kuu, cond_S, (log_norm, mean, cov) shifted, and their bounds."""
    if name not in _cache:
        c = make_case(name)
        lp, tol, diag = logpdf_and_bound(c)
        mom = node_moments(c["X"], c["wts"], c["start"], lp)
        c.update(lp=lp, tol=tol, log_norm=mom[0], mean=mom[1], cov=mom[2], bounds=moment_bounds(c["X"], c["start"], tol, *mom), **diag)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]
