"""NumPy restatement of the batched :out messages (sgp_out_message) and of the GP-SSM VMP schedule (train.vmp_gpssm), written from
the reference's rules (GPnode/MultiSGPnode.jl: :out 90-120, :in 162-208 with the product 37-44, :v 290-328, :w 367-444, average
energy 544-632; UniSGPnode.jl:85-93) with dense algebra, one node at a time.  It takes nothing from the library but the cubature
rules and the distribution containers.

:out of node t:  mean[t, d] = sum_s w_s k_s' mu_v^(d),  k_s = K(Xu, x_s), with the bound
    tol[t, d] = 50 eps sum_s |w_s| |k_s|' |mu_v^(d)|
-- the |k|'|s_t| term of tests/in_message_ref.py, summed with the weights' magnitudes: a dot product's error is eps |k|'|mu| per
term of its length's logarithm, the kernel values carry a few eps each, and 50 covers both at these sizes.

The out-message cases are the smallest shapes at which the kernel can go wrong: (a) the pendulum's shape; (b) d_out = 1 with node
sizes 1, 21, 1, 3 (a one-point node, a node of several lane rounds' worth is case d's) and Gauss-Hermite weights; (c) M above two
64-row tiles, D = 5 through the generic kernel form, d_out = 4, explicit mu_v; (d) a node longer than a chunk of 64 or 128 points
that straddles chunks, zero and negative weights, a node whose weights sum to 0."""
import functools
import math

import numpy as np

from gaussianprocessnode_amd.cubature import ghcubature, srcubature
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, WishartFast

EPS = np.finfo(np.float64).eps
SQRT3, SQRT5 = math.sqrt(3.0), math.sqrt(5.0)


def kernel(family, sigma2, ell, A, B, dtype=np.float64):
    """K(A, B) (na x nb) of sigma2 kappa(|(a - b) / ell|), kappa of KernelFunctions.jl's SEKernel / Matern32Kernel / Matern52Kernel."""
    A = np.asarray(A, dtype=dtype).reshape(len(A), -1)
    B = np.asarray(B, dtype=dtype).reshape(len(B), -1)
    ell = np.broadcast_to(np.asarray(ell, dtype=dtype), (A.shape[1],))
    t = (A[:, None, :] - B[None, :, :]) / ell
    s = np.sum(t * t, axis=2)
    if family == "se":
        kap = np.exp(-s / 2)
    elif family == "matern32":
        r = np.sqrt(s) * dtype(SQRT3) if dtype is np.float64 else np.sqrt(s) * np.sqrt(dtype(3))
        kap = (1 + r) * np.exp(-r)
    elif family == "matern52":
        r = np.sqrt(s) * dtype(SQRT5) if dtype is np.float64 else np.sqrt(s) * np.sqrt(dtype(5))
        kap = (1 + r + 5 * s / 3) * np.exp(-r)
    else:
        raise ValueError(family)
    return dtype(sigma2) * kap


# ------------------------------------------------------------------------------------------------
# the :out cases
OUT_CASES = {
    "a": dict(M=48, D=2, d_out=2, family="se", ell=(0.7, 0.9), sizes=[5] * 12, cub="sr", seed=11),
    "b": dict(M=70, D=1, d_out=1, family="matern52", ell=(0.5,), sizes=[1, 21, 1, 3], cub="gh", seed=12),
    "c": dict(M=130, D=5, d_out=4, family="matern32", ell=(1.8, 2.0, 2.2, 2.4, 2.6), sizes=[11] * 9, cub="sr", seed=13),
    "d": dict(M=20, D=3, d_out=3, family="se", ell=(0.9, 1.1, 1.3), sizes=[7, 150, 1], cub="random", seed=14),
}
SIGMA2 = 0.8


@functools.lru_cache(maxsize=None)
def make_out_case(name):
    """Inputs of one case: Xu ~ U(-2, 2), mu_v = 0.3 randn; node centres ~ U(-1.5, 1.5) with covariance 0.05 (L L' / D + I).
    Points: srcubature ("sr": 2 D + 1 per node), Gauss-Hermite of the node's size ("gh"; a one-point node is its centre with
    weight 1), or ("random") centre + chol randn with weights ~ U(-0.5, 1.5), every fifth one of a longer node exactly 0, and node 0's weights
    (0.5, -0.5, 0.25, -0.25, 1, -1, 0): their sum is 0.  Arrays are read-only."""
    c = dict(OUT_CASES[name])
    M, D, d_out, sizes = c["M"], c["D"], c["d_out"], c["sizes"]
    rng = np.random.default_rng(c["seed"])
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    mu_v = 0.3 * rng.normal(size=M * d_out)
    pts, wts = [], []
    for size in sizes:
        m = rng.uniform(-1.5, 1.5, D)
        L = rng.normal(size=(D, D))
        P = 0.05 * (L @ L.T / D + np.eye(D))
        if c["cub"] == "sr":
            p, w = srcubature().points_weights(m, P)
        elif c["cub"] == "gh":
            p, w = (m[None, :], np.ones(1)) if size == 1 else ghcubature(size).points_weights(m, P)
        else:
            p = m + rng.normal(size=(size, D)) @ np.linalg.cholesky(P).T
            w = rng.uniform(-0.5, 1.5, size)
            if size > 1:
                w[::5] = 0.0
        assert len(w) == size
        pts.append(np.asarray(p, dtype=np.float64).reshape(size, D))
        wts.append(np.asarray(w, dtype=np.float64))
    if c["cub"] == "random":
        wts[0] = np.array([0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 0.0])
    c.update(Xu=Xu, mu_v=mu_v, X=np.concatenate(pts), wts=np.concatenate(wts), sigma2=SIGMA2, ell=np.array(c["ell"]), jitter=1e-8,
             start=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), nodes=len(sizes))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def out_message_ref(c, dtype=np.float64, reverse=False):
    """(mean (T, d_out), tol (T, d_out), point_mean (n, d_out)) of a case, one node at a time: sum_s w_s k_s' mu^(d) in `dtype`
    (np.float64 or np.longdouble), the points of a node and the entries of every dot product taken in order or (reverse) backwards."""
    M, d_out, start = c["M"], c["d_out"], c["start"]
    mus = np.asarray(c["mu_v"], dtype=dtype).reshape(d_out, M)
    T = len(start) - 1
    mean, tol = np.zeros((T, d_out), dtype=dtype), np.zeros((T, d_out))
    point = np.zeros((len(c["X"]), d_out), dtype=dtype)
    order = (lambda n: range(n - 1, -1, -1)) if reverse else range
    for t in range(T):
        K = kernel(c["family"], c["sigma2"], c["ell"], c["Xu"], c["X"][start[t]:start[t + 1]], dtype)     # M x S
        w = np.asarray(c["wts"][start[t]:start[t + 1]], dtype=dtype)
        for d in range(d_out):
            acc = dtype(0)
            for s in order(K.shape[1]):
                dot = dtype(0)
                for m in order(M):
                    dot = dot + K[m, s] * mus[d, m]
                point[start[t] + s, d] = dot
                acc = acc + w[s] * dot
            mean[t, d] = acc
            tol[t, d] = 50 * EPS * float(np.abs(np.asarray(w, dtype=np.float64))
                                         @ (np.abs(np.asarray(K, dtype=np.float64)).T @ np.abs(np.asarray(mus[d], dtype=np.float64))))
    return mean, tol, point


@functools.lru_cache(maxsize=None)
def out_reference(name):
    """(case, mean, tol, point_mean) in float64, computed once per process; read-only."""
    c = make_out_case(name)
    mean, tol, point = out_message_ref(c)
    for v in (mean, tol, point):
        v.setflags(write=False)
    return c, mean, tol, point


# ------------------------------------------------------------------------------------------------
# the pendulum and the VMP schedule
N_FULL, MAX_TIME = 700, 7.0
DT = MAX_TIME / (N_FULL - 1)
QC = 0.01
Q_PROC = np.array([[QC * DT ** 3 / 3, QC * DT ** 2 / 2], [QC * DT ** 2 / 2, QC * DT]])
P_OBS = 0.1 * np.eye(2)
X_INIT = np.array([1.5, 0.0])
X0_PRIOR = (np.array([1.6, 0.0]), 0.1 * np.eye(2))


def pendulum(n, seed):
    """(states (n, 2), observations (n, 2)) of the notebook's pendulum (cells 4-5) from NumPy's generator."""
    rng = np.random.default_rng(seed)
    Lq, Lp = np.linalg.cholesky(Q_PROC), np.linalg.cholesky(P_OBS)
    x, xs, ys = X_INIT.copy(), [], []
    for _ in range(n):
        x = np.array([x[0] + x[1] * DT, x[1] - 9.81 * math.sin(x[0]) * DT]) + Lq @ rng.normal(size=2)
        xs.append(x)
        ys.append(x + Lp @ rng.normal(size=2))
    return np.array(xs), np.array(ys)


def grid_inducing():
    """48 inducing inputs on a 6 x 8 grid over [-2.5, 2.5] x [-4.5, 4.5] (spacing 1 and 9 / 7): with the lengthscales (0.8, 1.0)
    K_uu + 1e-6 I has a condition number below 1e3, so the :in and sweep steps' own conditioning-driven errors stay small beside
    the :out bound the driver comparison's tolerance is derived from."""
    g1, g2 = np.linspace(-2.5, 2.5, 6), np.linspace(-4.5, 4.5, 8)
    return np.array([[a, b] for a in g1 for b in g2])


# The priors of the test runs: v ~ N(0, 5 I) and W ~ Wishart(3, I) (mean 3 I) in place of the notebook's 50 I and mean 100 I.  With
# the notebook's, the first iteration's closures lie near -5000 |k|^2 (S = sum_ij W_ij Rv_ij = 10^4 I): every exp underflows and
# every node takes the NaN fallback; and a transition precision ten times the observation precision shrinks every left message
# towards the GP's zero prior mean, so that a 40-step run needs about 30 Jacobi iterations to beat its observations (measured
# with this file: SMSE 8.5 / 1.45 after 6 iterations, 5.6 / 0.23 after 30, raw observations 1.71 / 0.079).
TEST_PRIORS = dict(v_prior_var=5.0, w_prior=(3.0, np.eye(2)))
PARITY = dict(T=12, seed=31, sigma2=1.0, ell=np.array([0.8, 1.0]), jitter=1e-6, iterations=3)


def smse(y_true, y_approx):
    y_true, y_approx = np.asarray(y_true, dtype=np.float64), np.asarray(y_approx, dtype=np.float64)
    return float(np.sum((y_true - y_approx) ** 2) / y_true.size / np.var(y_true, ddof=1))


def wishart_mean_logdet(nu, invS):
    from scipy.special import digamma
    d = invS.shape[0]
    return float(sum(digamma(0.5 * (nu - i)) for i in range(d)) + d * math.log(2.0) - np.linalg.slogdet(invS)[1])


def moments_are_nan(lp):
    """The reference's products exponentiate unshifted: NaN moments when an exp overflows or all of them underflow."""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(lp)
    return bool(np.any(~np.isfinite(e)) or not np.any(e > 0.0))


def vmp_gpssm_ref(sigma2, ell, y, Xu, *, P=P_OBS, x0_prior=X0_PRIOR, v_prior_var=50.0, w_prior=(100.0, np.eye(2)), iterations=10,
                  jitter=0.0, family="se", displace_out=False):
    """The schedule of train.vmp_gpssm with per-node loops (its docstring numbers the steps).  displace_out: every :out mean is
    displaced by + its bound tol[t, d].  Returns dict(q_x, q_v, q_w, fe, fallbacks): fallbacks[i] = the nodes of iteration i that
    took the reference's NaN fallback (their left message returned)."""
    sr = srcubature()
    y = np.asarray(y, dtype=np.float64)
    T, d = y.shape
    M = len(Xu)
    Qv = d * M
    m0, P0 = x0_prior
    nu0, invS0 = float(w_prior[0]), np.asarray(w_prior[1], dtype=np.float64)
    Pinv = np.linalg.inv(P)
    Kinv = np.linalg.inv(kernel(family, sigma2, ell, Xu, Xu) + jitter * np.eye(M))
    Kinv = 0.5 * (Kinv + Kinv.T)
    q_x = [MvNormalMeanCovariance(np.array(m0), np.array(P0))] + [MvNormalMeanCovariance(np.zeros(d), 50.0 * np.eye(d)) for _ in range(T)]
    mu_v, Sig_v = np.zeros(Qv), v_prior_var * np.eye(Qv)
    q_w = WishartFast(nu0, invS0.copy())
    fe, fallbacks = [], []
    for _ in range(iterations):
        W = q_w.mean()
        E_logdet = wishart_mean_logdet(q_w.nu, q_w.invS)
        mus = mu_v.reshape(d, M)
        # 1: the forward messages from q(x_{t-1})
        outs = np.empty((T, d))
        for t in range(T):
            pts, w = sr.points_weights(q_x[t].m, q_x[t].S)
            K = kernel(family, sigma2, ell, Xu, pts)
            outs[t] = mus @ (K @ w)
            if displace_out:
                outs[t] += 50 * EPS * (np.abs(mus) @ (np.abs(K) @ np.abs(w)))
        # 2: the left messages
        S = np.linalg.inv(W + Pinv)
        S = 0.5 * (S + S.T)
        lefts = [MvNormalMeanCovariance(np.array(m0), np.array(P0))] + [MvNormalMeanCovariance(S @ (W @ outs[t] + Pinv @ y[t]), S) for t in range(T)]
        # 3: q(x_t) = left_t x :in of node t + 1, closure at q_out = the previous q(x_{t+1})
        Rv = Sig_v + np.outer(mu_v, mu_v)
        S_W = sum(W[i, j] * Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] for i in range(d) for j in range(d))
        S_W = 0.5 * (S_W + S_W.T)
        trW = float(np.trace(W))
        new_x, fell = [], []
        for t in range(T):
            pts, w = sr.points_weights(lefts[t].m, lefts[t].S)
            K = kernel(family, sigma2, ell, Xu, pts)                                   # M x S
            s_t = mus.T @ (q_x[t + 1].m @ W)
            lp = np.array([-0.5 * trW * (sigma2 - k @ Kinv @ k) + s_t @ k - 0.5 * k @ S_W @ k for k in K.T])
            if moments_are_nan(lp):
                new_x.append(lefts[t])
                fell.append(t)
                continue
            g = w * np.exp(lp - lp.max())
            mean = (g @ pts) / g.sum()
            dv = pts - mean
            new_x.append(MvNormalMeanCovariance(mean, (dv * g[:, None]).T @ dv / g.sum()))
        q_x = new_x + [lefts[T]]
        fallbacks.append(fell)
        # 4: q(v) from all nodes' :v messages at the new q(x)
        Psi2s, B, stats = np.zeros((M, M)), np.zeros((M, d)), []
        for t in range(T):
            pts, w = sr.points_weights(q_x[t].m, q_x[t].S)
            K = kernel(family, sigma2, ell, Xu, pts)
            Psi0, Psi1, Psi2 = sigma2 * w.sum(), K @ w, (K * w) @ K.T
            stats.append((Psi0, Psi1, Psi2))
            Psi2s += Psi2
            B += np.outer(Psi1, q_x[t + 1].m)
        Lam = np.eye(Qv) / v_prior_var + np.kron(W, Psi2s)
        Sig_v = np.linalg.inv(Lam)
        Sig_v = 0.5 * (Sig_v + Sig_v.T)
        mu_v = Sig_v @ (B @ W).T.reshape(-1)
        # 5 (and the energy): the :w messages' inverse scales I1_t + I2_t at the new q(x), q(v)
        Rv = Sig_v + np.outer(mu_v, mu_v)
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
        fe.append(energy + host_energy(y, P, q_x, mu_v, Sig_v, q_w, x0_prior, v_prior_var, (nu0, invS0)))
        q_w = WishartFast(nu0 + T, invS0 + invS_sum)
    return dict(q_x=q_x, q_v=MvNormalMeanCovariance(mu_v, Sig_v), q_w=q_w, fe=fe, fallbacks=fallbacks)


def host_energy(y, P, q_x, mu_v, Sig_v, q_w, x0_prior, v_prior_var, w_prior):
    """The free energy's terms beside the MultiSGP factors: observation energies, KL(q(x_0) || prior), minus the entropies of
    q(x_1..T), KL(q(v) || prior), KL(q(W) || prior)."""
    from scipy.special import multigammaln

    def gauss_kl(m, S, m0, S0):
        S0inv = np.linalg.inv(S0)
        return 0.5 * (np.trace(S0inv @ S) + (m - m0) @ S0inv @ (m - m0) - len(m) + np.linalg.slogdet(S0)[1] - np.linalg.slogdet(S)[1])
    d = y.shape[1]
    Pinv = np.linalg.inv(P)
    total = gauss_kl(q_x[0].m, q_x[0].S, *x0_prior)
    for t in range(1, len(q_x)):
        r = y[t - 1] - q_x[t].m
        total += 0.5 * (d * math.log(2 * math.pi) + np.linalg.slogdet(P)[1] + r @ Pinv @ r + np.trace(Pinv @ q_x[t].S))
        total -= 0.5 * np.linalg.slogdet(2 * math.pi * math.e * q_x[t].S)[1]
    Q = len(mu_v)
    total += gauss_kl(mu_v, Sig_v, np.zeros(Q), v_prior_var * np.eye(Q))
    nu, invS, (nu0, invS0) = q_w.nu, q_w.invS, w_prior
    psi_d = wishart_mean_logdet(nu, invS) - d * math.log(2.0) + np.linalg.slogdet(invS)[1]
    total += (0.5 * nu0 * (np.linalg.slogdet(invS)[1] - np.linalg.slogdet(invS0)[1]) + 0.5 * nu * (np.trace(invS0 @ np.linalg.inv(invS)) - d)
              + multigammaln(0.5 * nu0, d) - multigammaln(0.5 * nu, d) + 0.5 * (nu - nu0) * psi_d)
    return float(total)


@functools.lru_cache(maxsize=None)
def parity_reference():
    """The driver-parity case: (y, Xu, plain run, run with the :out means displaced by + their bounds), computed once."""
    p = PARITY
    _, y = pendulum(p["T"], p["seed"])
    Xu = grid_inducing()
    kw = dict(iterations=p["iterations"], jitter=p["jitter"], **TEST_PRIORS)
    return y, Xu, vmp_gpssm_ref(p["sigma2"], p["ell"], y, Xu, **kw), vmp_gpssm_ref(p["sigma2"], p["ell"], y, Xu, displace_out=True, **kw)


def compared(run):
    """The quantities the driver comparison takes from a run: mean and cov of every q(x_t), mean(q(v)), mean(q(W))."""
    return dict(x_mean=np.stack([q.m for q in run["q_x"]]), x_cov=np.stack([q.S for q in run["q_x"]]),
                v_mean=np.asarray(run["q_v"].m), w_mean=np.asarray(run["q_w"].mean()))


def parity_tolerances():
    """Per compared quantity, 10 x the largest relative change (max |delta| / max |value|) under the displaced :out means."""
    _, _, plain, moved = parity_reference()
    a, b = compared(plain), compared(moved)
    return {k: 10.0 * float(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(a[k]))) for k in a}
