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
margin.

The shape cases (SHAPE_CASES, make_shape_case: dimensions up to 32, every family, ragged M and Q, many small nodes, the size
limit, zero weights) keep this model and add one term, shape_moment_bounds.  A one-point node has cov = 0 and mean = x exactly,
but the kernel's mean (g x) / g is not always bit-equal to x, and at 129+ points the sums' own rounding is no longer hidden by
tau r.  The kernel forms sum g x and sum g as 64 lane chains of R = ceil(S / 64) fused multiply-adds or additions (one rounding
each), six butterfly additions and one division: 2 (R + 6) + 1 roundings of u = eps / 2 between the exact weighted mean of the
computed g and the stored one, each relative to sum g |x| / sum g <= max |x|_2.  g itself carries exp's 2 ulp, one product and the
rounding of logpdf - a (relative u |logpdf - a|, which weighs in only where exp(logpdf - a) does: <= u / e): under 5 eps, a
weighted mean's perturbation of at most 5 eps r <= 10 eps max |x|_2.  Together (R + 6.5 + 10) eps; the float64 reference rounds
likewise, so the term is
    m_term = 2 (R + 17) eps max_s |x_s|_2        (mean),      m_term^2      (cov),
the latter because sum g (x - m')(x - m')' / sum g = cov + (m' - m)(m' - m)' exactly for any m' (the cross terms vanish); the
covariance sum's own rounding, (R + 10) eps sqrt(cov_ii cov_jj), stays inside the model's 1e-13 max |cov|.  log_norm needs
nothing: log's and the sums' relative rounding (R + 8) eps is inside 1e-13 |log_norm| or 2 tau.  tests/test_in_message_host.py
evaluates the kernel's summation order in float64 against mpmath on every shape case and records the worst ratio to the term.

Points of weight 0 take no part: the shift a, tau and r are taken over the points of positive weight (shape_node_moments)."""
import contextlib
import functools
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
ELL = {1: (0.25, 0.25), 2: (0.7, 0.9), 3: (0.9, 1.3), 4: (1.1, 1.7), 5: (1.8, 2.6)}     # per input dimension: linspace(lo, hi, D)


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


# ------------------------------------------------------------------------------------------------
# the shape cases: explicit node sizes, dimensions up to 32, every family, the size limit, zero weights
DIMS = [5, 7, 9, 16, 31, 32]
FAMILIES = ["se", "matern12", "matern32", "matern52"]
DIM_SIZES = [1, 64, 65, 129, 200, 3]                    # one point, one full lane round, a second, a third, a fourth, a few
LIMIT_SIZES = [1, 70, 9]
SHAPE_CASES = {}
for _D in DIMS:
    for _iso in (False, True):
        SHAPE_CASES[f"dim{_D}{'iso' if _iso else ''}"] = dict(M=70, D=_D, d_out=2, family="se", sizes=DIM_SIZES, seed=100 + _D, iso=_iso)
for _f, _fam in enumerate(FAMILIES):
    for _do in (1, 2, 3, 4):
        SHAPE_CASES[f"{_fam}x{_do}"] = dict(M=65, D=9, d_out=_do, family=_fam, sizes=[7, 12, 5], seed=200 + 10 * _f + _do, coincident=1)
for _M in (1, 63, 64, 129):
    for _do in (3, 4):
        SHAPE_CASES[f"ragged{_M}x{_do}"] = dict(M=_M, D=3, d_out=_do, family="se", sizes=[5, 70, 1], seed=300 + 10 * _do + _M)
SHAPE_CASES["many"] = dict(M=48, D=6, d_out=4, family="se", sizes=[1 + t % 3 for t in range(1001)], seed=400)
SHAPE_CASES["limit1"] = dict(M=4032, D=2, d_out=1, family="se", sizes=LIMIT_SIZES, seed=500, jitter=1e-6)
SHAPE_CASES["limit4"] = dict(M=1008, D=2, d_out=4, family="se", sizes=LIMIT_SIZES, seed=501, jitter=1e-6)
WEIGHT_SIZES = [12, 9, 12, 5]
for _k in ("some_zero", "top_zero_near", "top_zero_far"):
    SHAPE_CASES["w_" + _k] = dict(M=48, D=2, d_out=2, family="se", sizes=WEIGHT_SIZES, seed=600, weights=_k)
VECTOR_ABOVE = 512                                      # M above which the reference is the vectorised restatement


def make_shape_case(M, D, d_out, family, sizes, seed, jitter=1e-8, iso=False, w_scale=1.0, coincident=None, weights=None,
                    rank=64):
    """Inputs with explicit node sizes: Xu ~ U(-1.745, 1.745); lengthscales tests/test_gpu_dims.lengthscales(D) for D >= 5 (the
    ELL table below), or one isotropic value (`ell_dev` is what the device is given: n_ell = 1); node centres ~ U(-1.2, 1.2),
    points centre + 0.25 randn, weights ~ U(0.1, 1); mu_v, W, Y as make_case; Sigma_v = 0.01 I + 0.02 U U' / rank, U Q x rank.
    coincident = t: node t's first five points are inducing inputs, its next five lie ~1e-9 from the next five inducing inputs.
    weights: one of the zero-weight constructions of `_zero_weights`."""
    from tests.test_gpu_dims import iso_lengthscale, lengthscales
    rng = np.random.default_rng(seed)
    Q, T, n = M * d_out, len(sizes), int(np.sum(sizes))
    Xu = rng.uniform(-1.745, 1.745, (M, D))
    if D >= 5:
        ell = np.full(D, iso_lengthscale(D)) if iso else lengthscales(D)
    else:
        ell = np.full(D, 0.5 * sum(ELL[D])) if iso else np.linspace(*ELL[D], D)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    centres = rng.uniform(-1.2, 1.2, (T, D))
    X = np.repeat(centres, sizes, axis=0) + 0.25 * rng.normal(size=(n, D))
    wts = rng.uniform(0.1, 1.0, n)
    mu_v = 0.3 * rng.normal(size=Q)
    B = rng.normal(size=(d_out, d_out))
    W = (B @ B.T / d_out + np.eye(d_out)) * w_scale
    Y = rng.normal(size=(T, d_out))
    U = rng.normal(size=(Q, rank))
    Sigma_v = 0.02 * (U @ U.T) / rank
    Sigma_v[np.diag_indices(Q)] += 0.01
    if coincident is not None:
        p = start[coincident]
        X[p:p + 5] = Xu[:5]
        X[p + 5:p + 10] = Xu[5:10] + 1e-9 * rng.normal(size=(5, D))
    c = dict(M=M, D=D, d_out=d_out, nodes=T, family=family, jitter=jitter, sigma2=SIGMA2, ell=ell, ell_dev=ell[:1] if iso else ell,
             Xu=Xu, X=X, wts=wts, start=start, mu_v=mu_v, Sigma_v=Sigma_v, W=W, Y=Y, sizes=list(sizes))
    if weights is not None:
        _zero_weights(c, weights, rng)
    return c


def _zero_weights(c, kind, rng):
    """Node 0: four weights exactly 0 (every kind).  Node 2 (top_zero_*): nine points of positive weight in a tight cluster
    (0.02 randn) and three of weight 0 in another, the zero-weight cluster being the one the closure values are larger at; W is
    then scaled (logpdf is linear in W, as in case e) so that the largest zero-weight logpdf lies 300 ("near": the shifted sums
    of the earlier kernel were still finite) or 850 ("far": all of them underflowed) above the largest positively weighted one."""
    st = c["start"]
    c["wts"][st[0] + np.array([0, 3, 4, 11])] = 0.0
    if kind == "some_zero":
        return
    A, B = np.array([-0.9, 0.7]), np.array([0.8, -0.6])
    noise = 0.02 * rng.normal(size=(12, c["D"]))
    for first, second in ((A, B), (B, A)):
        c["X"][st[2]:st[3]] = np.concatenate([np.tile(first, (3, 1)), np.tile(second, (9, 1))]) + noise
        lp = vector_logpdf(c)["lp"][st[2]:st[3]]
        gap = lp[:3].max() - lp[3:].max()
        if gap > 0:
            break
    assert gap > 0
    c["wts"][st[2]:st[2] + 3] = 0.0
    c["W"] = c["W"] * ({"top_zero_near": 300.0, "top_zero_far": 850.0}[kind] / gap)


def kernel_of(c):
    from tests.test_kernel_family_host import matern
    return matern(c["family"])


def padded_blocks(Sigma_v, M, d_out, stride):
    """The Q x Q matrix whose block (a, b) is read at rows a * stride, columns b * stride of Sigma_v padded with the identity to
    a multiple of 64 -- stride = M is Sigma_v itself; stride = M_p is the mis-strided read k_form_S_in could make."""
    Q = M * d_out
    Qp = (Q + 63) // 64 * 64
    P = np.eye(max(Qp, (d_out - 1) * stride + M))
    P[:Q, :Q] = Sigma_v
    out = np.empty((Q, Q))
    for a in range(d_out):
        for b in range(d_out):
            out[a * M:(a + 1) * M, b * M:(b + 1) * M] = P[a * stride:a * stride + M, b * stride:b * stride + M]
    return out


def vector_logpdf(c, yw=None, Sigma_v=None, want_bound=False, Kinv=None):
    """The three terms of the closure for all points at once, through Cholesky solves (no explicit inverse, no M x M outer
    product per point): q = |L_K^-1 k|^2, lin = sum_d (y_t' W)_d k' mu^(d), form = k' S k with S never wider than M x M.
    yw (T, d_out) and Sigma_v replace the case's rows y_t' W and covariance (the host tests' faults).  want_bound adds tol and the
    condition numbers (extreme eigenvalues above VECTOR_ABOVE, as tests/test_envelope_host.spd_cond, the SVD's below).  Kinv: q is
    taken as k' Kinv k with that inverse, the closure's own arithmetic for this term (the two differ by the inverse's
    conditioning error, cond(K_uu) eps sigma2, whatever the order of the sums)."""
    from scipy.linalg import cholesky, solve_triangular
    M, d_out, W, start = c["M"], c["d_out"], c["W"], c["start"]
    kern = kernel_of(c)
    Kuu = kern(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(M)
    K = kern(c["sigma2"], c["ell"], c["Xu"], c["X"])                            # M x n
    if Kinv is None:
        A = solve_triangular(cholesky(Kuu, lower=True), K, lower=True)
        q = np.sum(A * A, axis=0)
    else:
        q = np.sum(K * (Kinv @ K), axis=0)
    Sig = c["Sigma_v"] if Sigma_v is None else Sigma_v
    mus = c["mu_v"].reshape(d_out, M).T                                         # M x d_out
    S = sum(W[i, j] * (Sig[i * M:(i + 1) * M, j * M:(j + 1) * M] + np.outer(mus[:, i], mus[:, j]))
            for i in range(d_out) for j in range(d_out))
    S = 0.5 * (S + S.T)
    form = np.sum(K * (S @ K), axis=0)
    yw = c["Y"] @ W if yw is None else yw
    node = np.repeat(np.arange(len(start) - 1), np.diff(start))
    s = mus @ yw.T                                                              # M x T: s_t
    lin = np.sum(K * s[:, node], axis=0)
    out = dict(lp=-0.5 * np.trace(W) * (c["sigma2"] - q) + lin - 0.5 * form, form=form)
    if want_bound:
        if M > VECTOR_ABOVE:
            from tests.test_envelope_host import spd_cond
            cond_kuu, cond_S = spd_cond(Kuu), spd_cond(S)
        else:
            cond_kuu, cond_S = float(np.linalg.cond(Kuu)), float(np.linalg.cond(S))
        out.update(cond_kuu=cond_kuu, cond_S=cond_S,
                   tol=50 * EPS * (0.5 * np.trace(W) * cond_kuu * c["sigma2"] + 0.5 * cond_S * form
                                   + np.sum(np.abs(K) * np.abs(s[:, node]), axis=0)))
    return out


def closure_logpdf(c):
    """logpdf of every point from the oracle's per-point closure O.multi_rule_in_logpdf (an M x M outer product per point)."""
    start = c["start"]
    lp = np.empty(len(c["X"]))
    with oracle_family(c["family"]):
        Kinv = O.cholinv(O.kernelmatrix(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(c["M"]))
        for t in range(len(start) - 1):
            f = O.multi_rule_in_logpdf(c["Xu"], c["sigma2"], c["ell"], c["Y"][t], c["mu_v"], c["Sigma_v"], c["W"], Kinv)
            for p in range(start[t], start[t + 1]):
                lp[p] = f(c["X"][p])
    return lp


def shape_node_moments(X, wts, start, lp):
    """node_moments over the points of positive weight alone, the shift taken over those."""
    T, D = len(start) - 1, X.shape[1]
    log_norm, mean, cov = np.empty(T), np.empty((T, D)), np.empty((T, D, D))
    for t in range(T):
        keep = np.arange(start[t], start[t + 1])[wts[start[t]:start[t + 1]] > 0]
        one = node_moments(X[keep], wts[keep], np.array([0, len(keep)]), lp[keep])
        log_norm[t], mean[t], cov[t] = one[0][0], one[1][0], one[2][0]
    return log_norm, mean, cov


def mean_rounding_term(X, wts, start):
    """m_term per node (module docstring): 2 (R + 17) eps max |x|_2, R = ceil(points / 64), over the points of positive weight."""
    out = np.empty(len(start) - 1)
    for t in range(len(out)):
        sl = slice(start[t], start[t + 1])
        R = -(-(start[t + 1] - start[t]) // 64)
        out[t] = 2 * (R + 17) * EPS * float(np.linalg.norm(X[sl][wts[sl] > 0], axis=1).max())
    return out


def shape_moment_bounds(X, wts, start, tol, log_norm, mean, cov):
    """moment_bounds over the points of positive weight, plus the mean-rounding term: b_mean + m_term, b_cov + m_term^2."""
    T = len(start) - 1
    b0, b1, b2 = np.empty(T), np.empty(T), np.empty(T)
    for t in range(T):
        keep = np.arange(start[t], start[t + 1])[wts[start[t]:start[t + 1]] > 0]
        one = moment_bounds(X[keep], np.array([0, len(keep)]), tol[keep], log_norm[t:t + 1], mean[t:t + 1], cov[t:t + 1])
        b0[t], b1[t], b2[t] = one[0][0], one[1][0], one[2][0]
    m = mean_rounding_term(X, wts, start)
    return b0, b1 + m, b2 + m * m


def finish_shape(c):
    """The reference of a shape case's inputs: lp (the oracle's closure up to M = VECTOR_ABOVE, the vectorised restatement
    above it), tol, the condition numbers, the moments over the positive weights and their bounds; arrays read-only."""
    c = dict(c)
    v = vector_logpdf(c, want_bound=True)
    lp = v["lp"] if c["M"] > VECTOR_ABOVE else closure_logpdf(c)
    mom = shape_node_moments(c["X"], c["wts"], c["start"], lp)
    c.update(lp=lp, tol=v["tol"], cond_kuu=v["cond_kuu"], cond_S=v["cond_S"], log_norm=mom[0], mean=mom[1], cov=mom[2],
             bounds=shape_moment_bounds(c["X"], c["wts"], c["start"], v["tol"], *mom))
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def shape_reference(name):
    """finish_shape(make_shape_case(**SHAPE_CASES[name])), computed once per process."""
    return finish_shape(make_shape_case(**SHAPE_CASES[name]))


def worst_ratios(c, lp, log_norm, mean, cov):
    """Worst error / bound of each compared output (a zero bound admits a zero error only)."""
    T = len(c["start"]) - 1

    def worst(err, bound):
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        err = np.where(np.isfinite(err), err, np.inf)
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
    b0, b1, b2 = c["bounds"]
    return dict(logpdf=worst(np.abs(lp - c["lp"]), c["tol"]), log_norm=worst(np.abs(log_norm - c["log_norm"]), b0),
                mean=worst(np.abs(mean - c["mean"]).reshape(T, -1).max(axis=1), b1),
                cov=worst(np.abs(cov - c["cov"]).reshape(T, -1).max(axis=1), b2))


# ------------------------------------------------------------------------------------------------
# the kernel's summation order in float64, and the same moments in mpmath (the host file's check of the mean-rounding term)
def kernel_order_moments(X, wts, start, lp):
    """k_in_moments' arithmetic in NumPy float64: lane l sums the points l, l + 64, .. in order, the 64 partial sums meet in an
    xor butterfly, the shift is taken over the positive weights.  (A product and a sum where the kernel has one fused
    multiply-add: one rounding more per step, never fewer.)"""
    T, D = len(start) - 1, X.shape[1]
    lanes = np.arange(64)
    log_norm, mean, cov = np.empty(T), np.empty((T, D)), np.empty((T, D, D))

    def wave_sum(terms):                                                   # terms: (S, ...) in point order
        R = -(-len(terms) // 64)
        pad = np.zeros((R * 64,) + terms.shape[1:])
        pad[:len(terms)] = terms
        v = np.zeros((64,) + terms.shape[1:])
        for r in range(R):
            v = v + pad[r * 64:(r + 1) * 64]
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ o]
        return v[0]
    for t in range(T):
        sl = slice(start[t], start[t + 1])
        x, w, l = X[sl], wts[sl], lp[sl]
        a = l[w > 0].max()
        with np.errstate(over="ignore", invalid="ignore"):
            g = np.where(w > 0, w * np.exp(l - a), 0.0)
        z = wave_sum(g)
        log_norm[t] = a + np.log(z)
        mean[t] = wave_sum(g[:, None] * x) / z
        d = x - mean[t]
        cov[t] = wave_sum((g[:, None] * d)[:, :, None] * d[:, None, :]) / z
    return log_norm, mean, cov


def mp_moments(X, wts, start, lp):
    """(log_norm, mean, cov) of the float64 inputs at 60 digits (mpmath): the exact moments up to the last conversion.  cov is
    summed in float64 from the deviations about the 60-digit mean, each rounded once (relative errors only; a one-point node's
    deviation is exactly 0)."""
    import mpmath
    T, D = len(start) - 1, X.shape[1]
    log_norm, mean, cov = np.empty(T), np.empty((T, D)), np.empty((T, D, D))
    with mpmath.workdps(60):
        for t in range(T):
            idx = [p for p in range(start[t], start[t + 1]) if wts[p] > 0]
            a = max(lp[p] for p in idx)
            g = [mpmath.mpf(float(wts[p])) * mpmath.exp(mpmath.mpf(float(lp[p])) - mpmath.mpf(float(a))) for p in idx]
            z = mpmath.fsum(g)
            log_norm[t] = float(mpmath.mpf(float(a)) + mpmath.log(z))
            m = [mpmath.fsum(gs * mpmath.mpf(float(X[p, d])) for gs, p in zip(g, idx)) / z for d in range(D)]
            mean[t] = [float(v) for v in m]
            dev = np.array([[float(mpmath.mpf(float(X[p, d])) - m[d]) for d in range(D)] for p in idx])
            gn = np.array([float(gs / z) for gs in g])
            cov[t] = (dev * gn[:, None]).T @ dev
    return log_norm, mean, cov
