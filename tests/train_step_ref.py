"""NumPy float64 restatement of one device-paced training step (helper, no tests).

What `sgp_train_begin` / `sgp_train_likelihood` / `sgp_train_step` / `sgp_train_end` promise in include/sgp_hip.h, written from
that header and the notebooks it cites (experiments/regression_kin40k.ipynb:196-230, experiments/classification_banana.ipynb
cells 7 and 9), without the package's host loop (`gaussianprocessnode_amd.train` is not imported): `TrainRef` keeps the run's
state -- raw theta, AdaMax m / u / running powers of beta, q(w) = (shape, rate), the prior in natural form, the carried mean --
and `TrainRef.step` does one minibatch and returns what is observable after `train_end`.

Per step, Gaussian likelihood:   window scalars -> sweep at softplus(theta) -> carry -> gradient at the carried q(v) ->
chain rule through softplus (d softplus = sigmoid) -> Flux's AdaMax.
Probit likelihood, the same with: forward message k_i' mu_v from the carried mean (zero before the first step); q(f) by
`probit_moments`; the sweep takes var(q_f); q(w) <- Gamma(a + n / 2, b + (sum I1 + sum I2) / 2) with n the whole window; the
gradient, linear in w, is rescaled to the NEW mean(q_w).

Error models (all from the reference side, none fitted to device output)
  * probit moments (`probit_bounds`): with g = s mz q, q = 1 / sqrt(1 + vz), r = phi(g) / Phi(g),
        |d mean| <= C_MEAN eps (|mz| + vz r q)
        |d var|  <= C_VAR  eps (vz + vz^2 / (1 + vz) r (|g| + r))
    The variance vz - vz^2 / (1 + vz) r (g + r) cancels twice in the far tail g -> -inf: r = |g| + 1 / |g| - ..., so g + r is
    1 / |g| with the absolute error of r (eps |g|), and r (g + r) -> 1 takes vz^2 / (1 + vz) back out of vz.  The bound is the
    sum of the terms' sizes.  Settled on the CPU against the mpmath form over g in [-40, 10], vz in {1e-2, 1, 1e2}
    (tests/test_train_step_host.py prints the figures): the float64 form's worst error / (eps x size) is 2.48 for the mean
    and 2.39 for the variance (both at vz = 100; in relative terms the variance is then off by 2.3e5 eps at g = -40).  C_MEAN =
    C_VAR = 8 leave the device's erfcx / erfc / exp (a few ulp each where SciPy's are within one) the rest: the float64 form
    alone uses 31 % and 30 % of them.
  * theta gradient (`theta_grad(..., bound=True)`): the project's model for everything that goes through K_uu^-1 -- cond(K_uu) eps
    of the cancelling terms' sizes -- per component i
        bound_i = 50 eps w [ cond(K_uu) ( sum |dK_uf,i| o (|Kinv| |K_uf|) + 1/2 sum |H| o |dK_uu,i| )
                             + sum |dK_uf,i| o (|R| |K_uf| + |mu| |y|') + 1/2 n [i = sigma2] ]
  * raw theta after k steps (`theta_tolerance`): the reference trajectory is run again with every step's gradient moved by plus
    and by minus its own bound; the tolerance is the largest movement of theta, times 4 (the sweep's own q(v) difference feeds
    the next gradient, which the model does not chain), plus the optimiser's own arithmetic, 16 eps (|theta| + eta) per step
    (one exp, two divisions, four products and two sums per component).
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.special import erfc, erfcx

from oracle import sgp_oracle as O

EPS = float(np.finfo(np.float64).eps)
C_MEAN, C_VAR = 8.0, 8.0
C_GRAD = 50.0
SQRT2 = math.sqrt(2.0)


def post_tol(cond_L):
    """The project's posterior bound (tests/test_gpu_parity.py)."""
    return min(1e-5, max(1e-9, 20 * EPS * cond_L))


# ---------------------------------------------------------------------------------------------------------------------------
# kernel families (include/sgp_hip.h: k = sigma2 kappa(r), s = sum_d ((a_d - b_d) / ell_d)^2, r = sqrt(s)) and d kappa / d s
# ---------------------------------------------------------------------------------------------------------------------------
def sq_dist(ell, A, B):
    A, B = np.atleast_2d(A) / ell, np.atleast_2d(B) / ell
    s = np.zeros((A.shape[0], B.shape[0]))
    for d in range(A.shape[1]):
        t = A[:, d:d + 1] - B[None, :, d]
        s += t * t
    return s


def kappa(family, s):
    r = np.sqrt(s)
    if family == "se":
        return np.exp(-0.5 * s)
    if family == "matern12":
        return np.exp(-r)
    if family == "matern32":
        return (1.0 + math.sqrt(3.0) * r) * np.exp(-math.sqrt(3.0) * r)
    if family == "matern52":
        return (1.0 + math.sqrt(5.0) * r + 5.0 * s / 3.0) * np.exp(-math.sqrt(5.0) * r)
    raise ValueError(family)


def dkappa_ds(family, s):
    """d kappa / d s (Matern-1/2: -exp(-r) / (2 r), taken as 0 at r = 0, where the numerator of dk/d ell vanishes too)."""
    r = np.sqrt(s)
    if family == "se":
        return -0.5 * np.exp(-0.5 * s)
    if family == "matern12":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, -np.exp(-r) / (2.0 * np.where(r > 0, r, 1.0)), 0.0)
    if family == "matern32":
        return -1.5 * np.exp(-math.sqrt(3.0) * r)
    if family == "matern52":
        return -(5.0 / 6.0) * (1.0 + math.sqrt(5.0) * r) * np.exp(-math.sqrt(5.0) * r)
    raise ValueError(family)


def kernelmatrix(family, sigma2, ell, A, B):
    return float(sigma2) * kappa(family, sq_dist(ell, A, B))


def full_ell(ell, D):
    return np.broadcast_to(np.asarray(ell, dtype=np.float64).ravel(), (D,)).copy()


# ---------------------------------------------------------------------------------------------------------------------------
# the d_out = 1 objective (helper_functions/derivative_helper.jl:23-39) and its analytic gradient
# ---------------------------------------------------------------------------------------------------------------------------
def theta_objective(family, sigma2, ell, Xu, X, y, mu, Sigma, w, jitter, omega=None):
    """f = w/2 [sigma2 n - tr(Kinv Psi2) + tr(R Psi2)] - w mu' K_uf y,  R = Sigma + mu mu', Kinv = (K_uu + jitter I)^-1.
    `omega`: the point weights of sgp_set_data (include/sgp_hip.h, sgp_theta_objective) -- Psi2 = K_uf diag(omega) K_uf', the
    targets omega .* y and s_w = sum omega in place of n; None is every weight 1."""
    M, D = Xu.shape
    ell = full_ell(ell, D)
    om = np.ones(len(y)) if omega is None else np.asarray(omega, dtype=np.float64)
    Kinv = np.linalg.inv(kernelmatrix(family, sigma2, ell, Xu, Xu) + jitter * np.eye(M))
    Kuf = kernelmatrix(family, sigma2, ell, Xu, X)
    Psi2 = (Kuf * om) @ Kuf.T
    R = Sigma + np.outer(mu, mu)
    return 0.5 * w * (sigma2 * om.sum() - np.sum(Kinv * Psi2) + np.sum(R * Psi2)) - w * float(mu @ (Kuf @ (om * y)))


def theta_grad(family, sigma2, ell, n_ell, Xu, X, y, mu, Sigma, w, jitter, bound=False, one_dim=False, omega=None):
    """d f / d (sigma2, ell_1 .. ell_n_ell).  With dk = the derivative of a kernel value,
        df = w [ sum_pn dK_uf o ((R - Kinv) K_uf - mu y') + 1/2 sum H o dK_uu + 1/2 n dsigma2 ],   H = Kinv Psi2 Kinv,
        dk / dsigma2 = k / sigma2 (the jitter is no part of dK_uu),   dk / dell_d = -2 sigma2 kappa'(s) (a_d - b_d)^2 / ell_d^3.
    n_ell = 1: the single lengthscale's derivative is the sum over the dimensions (`one_dim`: the fault that takes dimension 0).
    `omega` (None: every weight 1): point p's terms -- its column of dK_uf o (..), of Psi2 and of the bound -- carry omega_p, and
    s_w = sum omega stands for n (`theta_objective`); integer weights are repeated points."""
    M, D = Xu.shape
    om = np.ones(len(y)) if omega is None else np.asarray(omega, dtype=np.float64)
    n = om.sum() if omega is not None else len(y)
    ell = full_ell(ell, D)
    s_uu, s_uf = sq_dist(ell, Xu, Xu), sq_dist(ell, Xu, X)
    Kuu, Kuf = sigma2 * kappa(family, s_uu), sigma2 * kappa(family, s_uf)
    Kj = Kuu + jitter * np.eye(M)
    Kinv = np.linalg.inv(Kj)
    R = Sigma + np.outer(mu, mu)
    Psi2 = (Kuf * om) @ Kuf.T
    H = Kinv @ Psi2 @ Kinv
    A = ((R - Kinv) @ Kuf - np.outer(mu, y)) * om
    dsu, dsf = -2.0 * sigma2 * dkappa_ds(family, s_uu), -2.0 * sigma2 * dkappa_ds(family, s_uf)
    d_uf = [Kuf / sigma2] + [dsf * (Xu[:, k:k + 1] - X[None, :, k]) ** 2 / ell[k] ** 3 for k in range(D)]
    d_uu = [Kuu / sigma2] + [dsu * (Xu[:, k:k + 1] - Xu[None, :, k]) ** 2 / ell[k] ** 3 for k in range(D)]
    full = np.array([np.sum(A * f) + 0.5 * np.sum(H * u) for f, u in zip(d_uf, d_uu)])
    full[0] += 0.5 * n
    fold = (lambda v: np.array([v[0], v[1] if one_dim else v[1:].sum()])) if n_ell == 1 else (lambda v: v)
    g = w * fold(full)
    if not bound:
        return g
    cond = float(np.linalg.cond(Kj))
    AK, AR = (np.abs(Kinv) @ np.abs(Kuf)) * om, (np.abs(R) @ np.abs(Kuf) + np.outer(np.abs(mu), np.abs(y))) * om
    b = np.array([cond * (np.sum(np.abs(f) * AK) + 0.5 * np.sum(np.abs(H) * np.abs(u))) + np.sum(np.abs(f) * AR)
                  for f, u in zip(d_uf, d_uu)])
    b[0] += 0.5 * n
    fold_b = (lambda v: np.array([v[0], v[1:].sum()])) if n_ell == 1 else (lambda v: v)
    return g, C_GRAD * EPS * w * fold_b(b)


def theta_objective_mp(family, p, n_ell, Xu, X, y, mu, Sigma, w, jitter, dps=50):
    """The same objective in mpmath at `dps` digits, as a function of p = (sigma2, ell...) for numerical differentiation."""
    import mpmath as mp
    mp.mp.dps = dps
    M, D = Xu.shape
    s2 = p[0]
    ell = [p[1]] * D if n_ell == 1 else list(p[1:])

    def k(a, b):
        s = sum(((mp.mpf(float(a[d])) - mp.mpf(float(b[d]))) / ell[d]) ** 2 for d in range(D))
        r = mp.sqrt(s)
        if family == "se":
            return s2 * mp.exp(-s / 2)
        if family == "matern12":
            return s2 * mp.exp(-r)
        if family == "matern32":
            return s2 * (1 + mp.sqrt(3) * r) * mp.exp(-mp.sqrt(3) * r)
        return s2 * (1 + mp.sqrt(5) * r + 5 * s / 3) * mp.exp(-mp.sqrt(5) * r)
    Kuu = mp.matrix(M, M)
    for i in range(M):
        for j in range(M):
            Kuu[i, j] = k(Xu[i], Xu[j]) + (mp.mpf(float(jitter)) if i == j else 0)
    Kuf = mp.matrix(M, len(y))
    for i in range(M):
        for j in range(len(y)):
            Kuf[i, j] = k(Xu[i], X[j])
    Kinv = mp.inverse(Kuu)
    Psi2 = Kuf * Kuf.T
    R = mp.matrix((Sigma + np.outer(mu, mu)).tolist())
    tr = lambda A, B: sum(A[i, j] * B[j, i] for i in range(M) for j in range(M))
    b = Kuf * mp.matrix([float(v) for v in y])
    mub = sum(mp.mpf(float(mu[i])) * b[i] for i in range(M))
    return mp.mpf(float(w)) / 2 * (s2 * len(y) - tr(Kinv, Psi2) + tr(R, Psi2)) - mp.mpf(float(w)) * mub


def theta_grad_mp(family, sigma2, ell, n_ell, Xu, X, y, mu, Sigma, w, jitter, dps=50):
    import mpmath as mp
    mp.mp.dps = dps
    p0 = [mp.mpf(float(sigma2))] + [mp.mpf(float(e)) for e in np.atleast_1d(ell)[:n_ell]]
    out = []
    for i in range(len(p0)):
        f = lambda t, i=i: theta_objective_mp(family, p0[:i] + [t] + p0[i + 1:], n_ell, Xu, X, y, mu, Sigma, w, jitter, dps)
        out.append(mp.diff(f, p0[i], h=mp.mpf(10) ** (-dps // 3)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Probit moment matching (classification_banana.ipynb cell 7; include/sgp_hip.h, sgp_train_likelihood)
# ---------------------------------------------------------------------------------------------------------------------------
def hazard(g):
    """r = phi(g) / Phi(g): sqrt(2 / pi) / erfcx(-g / sqrt 2) for g < 0 (no cancellation, no underflow), the quotient else."""
    g = np.asarray(g, dtype=np.float64)
    neg = g < 0.0
    gn, gp = np.where(neg, g, -1.0), np.where(neg, 1.0, g)
    return np.where(neg, math.sqrt(2.0 / math.pi) / erfcx(-gn / SQRT2),
                    np.exp(-0.5 * gp * gp) / math.sqrt(2.0 * math.pi) / (0.5 * erfc(-gp / SQRT2)))


def probit_moments(label, mz, vz, flip_sign=False):
    """(mean, variance, g, r) of q(f) for `y ~ Probit(f)` with the forward message N(f; mz, vz), label in {0, 1}."""
    label, mz = np.asarray(label, dtype=np.float64), np.asarray(mz, dtype=np.float64)
    s = 2.0 * label - 1.0
    if flip_sign:
        s = -s
    q = 1.0 / math.sqrt(1.0 + vz)
    g = s * mz * q
    r = hazard(g)
    return mz + s * vz * r * q, vz - vz * vz / (1.0 + vz) * r * (g + r), g, r


def probit_moments_mp(label, mz, vz, dps=60):
    """The same quantities by mpmath (lists of mpf): mean, variance."""
    import mpmath as mp
    mp.mp.dps = dps
    vz = mp.mpf(float(vz))
    q = 1 / mp.sqrt(1 + vz)
    mean, var = [], []
    for lab, m in zip(np.atleast_1d(label), np.atleast_1d(mz)):
        s, m = mp.mpf(2 * float(lab) - 1), mp.mpf(float(m))
        g = s * m * q
        r = mp.npdf(g) / mp.ncdf(g)
        mean.append(m + s * vz * r * q)
        var.append(vz - vz * vz / (1 + vz) * r * (g + r))
    return mean, var


def probit_bounds(label, mz, vz):
    """Per-point bounds (mean, variance) on a float64 evaluation of `probit_moments` (module docstring)."""
    _, _, g, r = probit_moments(label, mz, vz)
    q = 1.0 / math.sqrt(1.0 + vz)
    return (C_MEAN * EPS * (np.abs(mz) + vz * r * q), C_VAR * EPS * (vz + vz * vz / (1.0 + vz) * r * (np.abs(g) + r)))


# ---------------------------------------------------------------------------------------------------------------------------
# the run
# ---------------------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


FAULTS = ("no_grad_rescale", "gamma_half_window", "u_without_max", "bias_power_off_by_one", "no_sigmoid", "vf_not_in_syy",
          "label_sign", "reset_ignored", "n_ell_one_dim", "update_on_reject", "offset_minus_one")


class TrainRef:
    """One run.  `prior`: ("iso", variance) or ("meancov", mu0, Sigma0) -- what the setters left before `train_begin`; the
    isotropic variance `reset_prior` goes back to is `prior_var`.  `fault`: one of FAULTS, a one-line mutation (for the host file's
    demonstration that the GPU cases would see it)."""

    def __init__(self, X, y, Xu, theta_raw, *, family="se", jitter=0.0, eta=1e-3, beta=(0.9, 0.999), eps=1e-8, w=1.0,
                 likelihood="gaussian", gamma=None, prior=("iso", 50.0), prior_var=50.0, fault=None, grad_shift=0.0, grad_scale=1.0):
        self.X, self.y, self.Xu = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(Xu, dtype=np.float64)
        self.M, self.D = self.Xu.shape
        self.theta = np.array(theta_raw, dtype=np.float64)
        self.n_ell = len(self.theta) - 1
        self.family, self.jitter, self.eta, self.beta, self.eps = family, float(jitter), float(eta), tuple(beta), float(eps)
        self.m, self.u = np.zeros_like(self.theta), np.zeros_like(self.theta)
        self.bp = np.array(self.beta, dtype=np.float64)
        if fault == "bias_power_off_by_one":
            self.bp[0] *= self.beta[0]
        self.probit = likelihood == "probit"
        self.a, self.b = (float(gamma[0]), float(gamma[1])) if self.probit else (None, None)
        self.w = self.a / self.b if self.probit else float(w)
        self.prior_var = float(prior_var)
        if prior[0] == "iso":
            self.Lambda0, self.xi0 = np.eye(self.M) / float(prior[1]), np.zeros(self.M)
        else:
            self.Lambda0 = O.cholinv(np.asarray(prior[2], dtype=np.float64))
            self.xi0 = self.Lambda0 @ np.asarray(prior[1], dtype=np.float64)
        self.mu, self.Sigma = np.zeros(self.M), None
        self.steps = self.skipped = 0
        self.fault, self.grad_shift, self.grad_scale = fault, float(grad_shift), float(grad_scale)
        self.log = []                          # per step: what the tolerances are made of

    def kernel(self):
        p = O.softplus(self.theta)
        return float(p[0]), full_ell(p[1:], self.D)

    def step(self, offset, n, learn=True, reset_prior=False):
        if self.fault == "offset_minus_one":
            offset = max(offset - 1, 0)
        if reset_prior and self.fault != "reset_ignored":
            self.Lambda0, self.xi0 = np.eye(self.M) / self.prior_var, np.zeros(self.M)
        s2, ell = self.kernel()
        Xw, yw = self.X[offset:offset + n], self.y[offset:offset + n]
        rec = dict(offset=offset, n=n, theta=self.theta.copy(), ok=False)
        w = self.w
        if self.probit:
            mz = kernelmatrix(self.family, s2, ell, Xw, self.Xu) @ self.mu
            mf, vf, g, _ = probit_moments(yw, mz, 1.0 / w, flip_sign=self.fault == "label_sign")
            bm, bv = probit_bounds(yw, mz, 1.0 / w)
            rec.update(g=g, mz=mz, vf=vf, mf=mf, sum_vf_bound=float(np.sum(bv) + np.sum(2.0 * np.abs(mf) * bm)))
        else:
            mf, vf = yw, None
        Kuu = kernelmatrix(self.family, s2, ell, self.Xu, self.Xu) + self.jitter * np.eye(self.M)
        Kuf = kernelmatrix(self.family, s2, ell, self.Xu, Xw)
        syy = float(np.sum(mf * mf) + (0.0 if vf is None or self.fault == "vf_not_in_syy" else np.sum(vf)))
        stats = O.SuffStats(Kuf @ Kuf.T, (Kuf @ mf)[:, None], np.array([[syy]]), s2 * n, float(n))
        Lam = self.Lambda0 + w * stats.Psi2
        try:
            L = cholesky(Kuu, lower=True)
            cholesky(Lam, lower=True)
        except np.linalg.LinAlgError:
            # a rejected minibatch: counted, theta (and q(w)) left alone
            self.skipped += 1
            if self.fault == "update_on_reject" and learn:
                self._adamax(np.ones_like(self.theta))          # (whatever the gradient buffer held: any value moves theta)
            self.log.append(rec)
            return self.observables()
        mu, Sigma, _ = O.v_update(stats, w, Lambda0=self.Lambda0, xi0=self.xi0)
        sum_I1, sum_I2 = O.w_stats_trace(stats, L, mu, Sigma)
        self.Lambda0, self.xi0 = Lam, self.xi0 + w * stats.b[:, 0]                                  # the carry
        self.mu, self.Sigma = mu, Sigma
        cond_K, cond_L = float(np.linalg.cond(Kuu)), float(np.linalg.cond(Lam))
        rec.update(ok=True, w=w, sum_I1=sum_I1, sum_I2=sum_I2, cond_K=cond_K, cond_L=cond_L, s_kk=s2 * n,
                   tol_I1=50 * EPS * cond_K * s2 * n + 1e-12, tol_I2=max(1e-7, post_tol(cond_L)) * abs(sum_I2))
        gscale = 1.0
        if self.probit:
            n_gamma = float(n // 2) if self.fault == "gamma_half_window" else float(n)
            self.a, self.b = O.gamma_update(self.a, self.b, n_gamma, sum_I1, sum_I2)
            self.w = self.a / self.b
            if self.fault != "no_grad_rescale":
                gscale = self.w / w
        if learn:
            g, gb = theta_grad(self.family, s2, ell, self.n_ell, self.Xu, Xw, mf, mu, Sigma, w, self.jitter, bound=True,
                               one_dim=self.fault == "n_ell_one_dim")
            g = self.grad_scale * gscale * (g + self.grad_shift * gb)
            rec.update(grad=g, grad_bound=gscale * gb)
            self._adamax(g if self.fault == "no_sigmoid" else g * sigmoid(self.theta))
            self.steps += 1
        self.log.append(rec)
        return self.observables()

    def _adamax(self, g):
        b1, b2 = self.beta
        self.m = b1 * self.m + (1.0 - b1) * g
        self.u = b2 * self.u if self.fault == "u_without_max" else np.maximum(b2 * self.u, np.abs(g))
        self.theta = self.theta - (self.eta / (1.0 - self.bp[0])) * self.m / (self.u + self.eps)
        self.bp = self.bp * np.array(self.beta)

    def observables(self):
        s2, ell = self.kernel()
        return dict(theta=self.theta.copy(), steps=self.steps, skipped=self.skipped, mu=self.mu.copy(),
                    Sigma=None if self.Sigma is None else self.Sigma.copy(), gamma=(self.a, self.b),
                    kernel=dict(sigma2=s2, ell=ell, w=self.w))


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU cases: inputs from seeds, schedules of (offset, n, learn, reset_prior)
# ---------------------------------------------------------------------------------------------------------------------------
def _inputs(seed, N, M, D, labels=False):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    f = np.sin(X @ rng.normal(size=D) / math.sqrt(D) * 2.0)
    y = (f + 0.4 * rng.normal(size=N) > 0).astype(np.float64) if labels else f + 0.1 * rng.normal(size=N)
    return X, y, Xu


# name: N, M, D, n_ell, family, jitter, sigma2, ell, schedule.  Window sizes 1, 63, 255, 256, 257 and 1000 straddle k_train_window's
# 256-thread stride; odd offsets with odd D leave X + offset D and y + offset 8-byte aligned only; the last window is shorter than
# the first; reset_prior on the first and on one later step; four learning steps, then one without.
GAUSS = {
    "w1000_m130_d3_se": (1100, 130, 3, 3, "se", 1e-6, 1.0, 0.6,
                         [(1, 1000, True, True), (257, 256, True, False), (513, 257, True, True), (1037, 63, True, False),
                          (1099, 1, False, False)]),
    "m12_d1_iso_m32": (600, 12, 1, 1, "matern32", 0.0, 1.2, 0.5,
                       [(1, 255, True, True), (257, 256, True, False), (0, 63, True, True), (513, 87, True, False),
                        (599, 1, False, False)]),
    "m64_d16_iso_m52": (520, 64, 16, 1, "matern52", 0.0, 0.9, 4.0,
                        [(0, 257, True, True), (257, 255, True, False), (100, 256, True, True), (512, 8, True, False),
                         (3, 63, False, False)]),
    "m65_d32_ard_se": (400, 65, 32, 32, "se", 1e-6, 1.1, 5.0,
                       [(2, 256, True, True), (258, 142, True, False), (0, 1, True, True), (1, 63, True, False),
                        (64, 40, False, False)]),
    "m65_d5_iso_m12": (330, 65, 5, 1, "matern12", 1e-6, 1.0, 1.5,
                       [(1, 257, True, True), (257, 73, True, False), (3, 255, True, True), (259, 63, True, False),
                        (329, 1, False, False)]),
    "m12_d1_iso_m32_short": (150, 12, 1, 1, "matern32", 0.0, 1.2, 0.5,       # the first run of the reallocation test
                             [(1, 100, True, True), (101, 49, True, False)]),
}
GAUSS_W, ETA = 20.0, 0.01

# name: gamma, schedule.  One shape (N 400, M 20, D 2, SE ARD, jitter 1e-6); (1e-4, 1) gives vz = 1e4 on the first step.
PROBIT = {
    "g001": ((0.01, 0.01), [(0, 200, True, False), (200, 150, True, False), (350, 50, True, False)]),
    "g1": ((1.0, 1.0), [(1, 257, True, False), (258, 142, True, False)]),
    "g1e-4": ((1e-4, 1.0), [(0, 200, True, False), (200, 200, True, False), (0, 63, False, False)]),
    "g1_moments": ((1.0, 1.0), [(3, 255, False, False)]),
    "g1e-4_moments": ((1e-4, 1.0), [(0, 256, False, False)]),
    # (tests/test_gpu_sharded_train.py: over three ranks the first window is 1 / 1 / 0 points -- an empty rank on a learning step)
    "g1_empty": ((1.0, 1.0), [(0, 2, True, False), (2, 200, True, False)]),
}


@functools.lru_cache(maxsize=None)
def gauss_case(name):
    N, M, D, n_ell, family, jitter, s2, ell, sched = GAUSS[name]
    X, y, Xu = _inputs(100 + sorted(GAUSS).index(name), N, M, D)
    theta0 = O.invsoftplus(np.concatenate([[s2], ell * np.linspace(0.9, 1.1, n_ell)]))
    return dict(name=name, X=X, y=y, Xu=Xu, theta0=theta0, family=family, jitter=jitter, sched=sched, n_max=max(s[1] for s in sched),
                kw=dict(family=family, jitter=jitter, eta=ETA, w=GAUSS_W), prior=("iso", 50.0), likelihood="gaussian")


@functools.lru_cache(maxsize=None)
def probit_case(name):
    gamma, sched = PROBIT[name]
    X, y, Xu = _inputs(7, 400, 20, 2, labels=True)
    theta0 = O.invsoftplus(np.array([1.0, 0.8, 1.1]))
    return dict(name=name, X=X, y=y, Xu=Xu, theta0=theta0, family="se", jitter=1e-6, sched=sched, n_max=max(s[1] for s in sched),
                kw=dict(family="se", jitter=1e-6, eta=ETA, likelihood="probit", gamma=gamma), prior=("iso", 50.0),
                likelihood="probit", gamma=gamma)


FAR = 100.0          # |x| at which every SE kernel value against the inducing inputs underflows to exactly 0 (s = 4e4 at ell = 0.5)


@functools.lru_cache(maxsize=None)
def tail_case(name):
    """The deep tail through a mean / covariance prior set before `train_begin` (include/sgp_hip.h: the prior stays "as the setters
    left" it): mu_0 makes k(x)' mu_0 swing over +-70 on the second window and Sigma_0 = 1e-8 I holds q(v) there.  The first step's
    window lies at x = FAR, where k(x) = 0 exactly: zero forward message, no information on v, q(w) moves from Gamma(1, 1) to a
    mean near 1/2; the step carries mu_0.  The second step (no reset_prior) then sees g = s k' mu_0 / sqrt(1 + vz) over both tails:
    labels that contradict the carried mean (g <= -25) and labels that agree with it (g >= 8).  "mixed": the second window also holds
    points at x = FAR (mz exactly 0, g = 0, where the two branches of r join) and is 257 long."""
    rng = np.random.default_rng(11)
    M, n_far = 12, 7
    Xu = np.linspace(-1.7, 1.7, M)[:, None]
    Xn = rng.uniform(-1.6, 1.6, (300, 1))
    s2, ell = 1.0, 0.5
    mu0 = np.linalg.lstsq(kernelmatrix("se", s2, [ell], Xn, Xu), 70.0 * np.cos(2.5 * Xn[:, 0]), rcond=1e-10)[0]
    far = FAR + np.arange(n_far, dtype=np.float64)[:, None]
    lab_n = (rng.uniform(size=300) < 0.5).astype(np.float64)
    if name == "tail":
        X, y = np.concatenate([far, Xn]), np.concatenate([np.ones(n_far), lab_n])
        sched = [(0, n_far, True, False), (n_far, 300, True, False)]
    else:
        X = np.concatenate([far, Xn[:250], far[:n_far] + 50.0])
        y = np.concatenate([np.ones(n_far), lab_n[:250], np.array([1, 0, 1, 0, 1, 0, 1.0])])
        sched = [(0, n_far, True, False), (n_far, 257, name == "mixed", False)]
    theta0 = O.invsoftplus(np.array([s2, ell]))
    return dict(name=name, X=X, y=y, Xu=Xu, theta0=theta0, family="se", jitter=1e-6, sched=sched, n_max=300,
                kw=dict(family="se", jitter=1e-6, eta=ETA, likelihood="probit", gamma=(1.0, 1.0)),
                prior=("meancov", mu0, 1e-8 * np.eye(M)), likelihood="probit", gamma=(1.0, 1.0))


def rejected_case():
    """Four identical inducing inputs, jitter 0 and sigma2 = softplus(64) = 64 exactly: K_uu is singular and its second pivot is
    64 - 64 * 64 / 64 = 0 in any order of exact operations."""
    X, y, Xu = _inputs(31, 120, 12, 2)
    Xu[1:4] = Xu[0]
    theta0 = np.array([64.0, *O.invsoftplus(np.array([0.9, 1.1]))])
    return dict(name="rejected", X=X, y=y, Xu=Xu, theta0=theta0, family="se", jitter=0.0,
                sched=[(0, 100, True, True), (100, 20, False, False)], n_max=100,
                kw=dict(family="se", jitter=0.0, eta=ETA, w=GAUSS_W), prior=("iso", 50.0), likelihood="gaussian")


def get_case(name):
    if name in GAUSS:
        return gauss_case(name)
    if name in PROBIT:
        return probit_case(name)
    if name == "rejected":
        return rejected_case()
    return tail_case(name)


def run(case, fault=None, grad_shift=0.0, nsteps=None, **over):
    ref = TrainRef(case["X"], case["y"], case["Xu"], case["theta0"], prior=case["prior"], fault=fault, grad_shift=grad_shift,
                   **{**case["kw"], **over})
    out = None
    for off, n, learn, reset in case["sched"][:nsteps]:
        out = ref.step(off, n, learn, reset)
    out["log"] = ref.log
    return out


@functools.lru_cache(maxsize=None)
def reference(name, nsteps=None):
    """The case's reference run (its first `nsteps` steps) and its tolerances, computed once and shared (the arrays are not to be
    written to)."""
    case = get_case(name)
    out = run(case, nsteps=nsteps)
    log = out["log"]
    out["theta_tol"] = theta_tolerance(case, out, nsteps)
    last = log[-1]
    if last["ok"]:
        out["post_tol"] = post_tol(last["cond_L"])
        oks = [r for r in log if r["ok"]]
        out["rate_tol"] = 0.5 * sum(r["tol_I1"] + r["tol_I2"] + r.get("sum_vf_bound", 0.0) for r in oks)
        out["sum_I2_tol"] = last["tol_I2"] + last.get("sum_vf_bound", 0.0)
    return out


def theta_tolerance(case, out, nsteps=None):
    moved = np.zeros_like(out["theta"])
    for shift in (1.0, -1.0):
        moved = np.maximum(moved, np.abs(run(case, grad_shift=shift, nsteps=nsteps)["theta"] - out["theta"]))
    return 4.0 * moved + out["steps"] * 16 * EPS * (np.abs(out["theta"]) + case["kw"]["eta"])


PRED_POINTS = 7


def pred_points(case):
    """Where the kernel left behind is probed: from the middle of the set (the tail cases' ends lie where every kernel value is 0)."""
    h = len(case["X"]) // 2
    return case["X"][h:h + PRED_POINTS]


def pred_weights(M):
    return np.linspace(-1.0, 1.0, M)


def observed(case, out):
    """A reference run's outputs in the form a device run reports them (tests/test_gpu_train_step.py, device_run): what is
    observable after train_end, with the kernel the handle is left with seen through a prediction K(x, Xu; softplus(theta)) c."""
    got = dict(theta=out["theta"], steps=out["steps"], skipped=out["skipped"], gamma=out["gamma"])
    if not out["skipped"]:
        k = out["kernel"]
        K = kernelmatrix(case["family"], k["sigma2"], k["ell"], pred_points(case), case["Xu"])
        got.update(mu=out["mu"], Sigma=out["Sigma"], sum_I2=out["log"][-1]["sum_I2"], pred=K @ pred_weights(case["Xu"].shape[0]))
    return got


def compare_outputs(name, got, nsteps=None):
    """error / tolerance of every compared output of `got` (a device run, or `observed` of a faulted reference run) against the
    clean reference: the one comparison the GPU file asserts (every ratio < 1) and the host file's fault list measures (some
    ratio >= 1e3).  Exact comparisons (counts, shape, theta without a learning step or on rejected minibatches) give 0 or inf."""
    ref, case = reference(name, nsteps), get_case(name)
    exact = lambda a, b: 0.0 if np.array_equal(np.asarray(a), np.asarray(b)) else math.inf
    relF = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    r = dict(counts=exact((ref["steps"], ref["skipped"]), (got["steps"], got["skipped"])))
    if ref["steps"] == 0 or ref["skipped"]:
        r["theta"] = exact(case["theta0"] if ref["steps"] == 0 else ref["theta"], got["theta"])
    else:
        r["theta"] = float(np.max(np.abs(got["theta"] - ref["theta"]) / ref["theta_tol"]))
    if ref["skipped"] or got["skipped"]:
        return r
    r["mu"], r["Sigma"] = relF(got["mu"], ref["mu"]) / ref["post_tol"], relF(got["Sigma"], ref["Sigma"]) / ref["post_tol"]
    # the kernel left behind: a kernel value moves by at most (1 + s) of its size per unit of relative change in sigma2 or a
    # lengthscale, and the device's own evaluation is good to a few eps (1 + s)
    k = ref["kernel"]
    Xs = pred_points(case)
    K = kernelmatrix(case["family"], k["sigma2"], k["ell"], Xs, case["Xu"])
    smax = float(np.max(sq_dist(k["ell"], Xs, case["Xu"])))
    rel_theta = float(np.max(ref["theta_tol"] / O.softplus(ref["theta"]))) if ref["steps"] else 0.0
    tol_pred = (64 * EPS + 4.0 * rel_theta) * (1.0 + smax) * (np.abs(K) @ np.abs(pred_weights(K.shape[1])))
    r["kernel"] = float(np.max(np.abs(got["pred"] - K @ pred_weights(K.shape[1])) / tol_pred))
    if case["likelihood"] == "probit":
        a = case["gamma"][0]
        for _, n, _, _ in case["sched"][:nsteps]:
            a += 0.5 * n                                                    # the same float operations
        r["shape"] = max(exact(a, got["gamma"][0]), exact(ref["gamma"][0], got["gamma"][0]))
        r["rate"] = abs(got["gamma"][1] - ref["gamma"][1]) / ref["rate_tol"]
        r["sum_I2"] = abs(got["sum_I2"] - ref["log"][-1]["sum_I2"]) / ref["sum_I2_tol"]
    return r


def compared(name, fault=None, nsteps=None):
    """`compare_outputs` of the reference run mutated by `fault`."""
    case = get_case(name)
    return compare_outputs(name, observed(case, run(case, fault=fault, nsteps=nsteps)), nsteps)
