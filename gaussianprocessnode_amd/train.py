"""Streaming minibatch driver: the loop of `PerformInference` / `my_free_energy`
(experiments/regression_kin40k.ipynb:182-230) on the device path.

Per epoch the prior is reset to N(0, prior_var I) (:203-204); each minibatch runs one VMP sweep with the previous
minibatch's posterior as prior (:205-212), then one optimiser step on the kernel hyper-parameters with q(v) held fixed
(:213-222, `grad_llh_new!` + `Flux.Optimise.update!`).  Host logic only -- the numbers come from the engine (C ABI)."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np

from .distributions import MvNormalMeanCovariance
from .meta import set_engine_kernel, softplus, split2batch


@dataclass
class AdaMax:
    """Flux.AdaMax (eta = 0.001, beta = (0.9, 0.999), eps = 1e-8) -- the optimiser of the kin40k / banana notebooks."""
    eta: float = 1e-3
    beta: tuple = (0.9, 0.999)
    eps: float = 1e-8
    _state: dict = field(default_factory=dict, repr=False)
    _named: dict = field(default_factory=dict, repr=False)

    def update(self, x: np.ndarray, grad: np.ndarray) -> np.ndarray:
        st = self._state.setdefault(id(x), dict(m=np.zeros_like(x), u=np.zeros_like(x), bp=np.array(self.beta, dtype=float)))
        st["m"] = self.beta[0] * st["m"] + (1.0 - self.beta[0]) * grad
        st["u"] = np.maximum(self.beta[1] * st["u"], np.abs(grad))
        delta = (self.eta / (1.0 - st["bp"][0])) * st["m"] / (st["u"] + self.eps)
        st["bp"] = st["bp"] * np.array(self.beta)
        x -= delta
        return x

    def get_state(self, x: np.ndarray) -> np.ndarray:
        """The state kept for the array `x` as sgp_theta_descend lays it out, [m | u | beta1^t, beta2^t] (zero moments and the
        powers (beta1, beta2) for an array that has taken no step)."""
        st = self._state.get(id(x))
        if st is None:
            return np.concatenate([np.zeros(2 * x.size), np.array(self.beta, dtype=float)])
        return np.concatenate([np.ravel(st["m"]), np.ravel(st["u"]), np.ravel(st["bp"])]).astype(np.float64)

    def set_state(self, x: np.ndarray, flat) -> None:
        """Install a state in that layout as the state of `x`: the next `update(x, ...)` continues from it."""
        flat = np.asarray(flat, dtype=np.float64).reshape(-1)
        n = x.size
        if flat.size != 2 * n + 2:
            raise ValueError(f"AdaMax.set_state: {2 * n + 2} entries expected for {n} parameters, got {flat.size}")
        self._state[id(x)] = dict(m=flat[:n].reshape(x.shape).copy(), u=flat[n:2 * n].reshape(x.shape).copy(), bp=flat[2 * n:].copy())

    def get_named_state(self, key, n: int) -> np.ndarray:
        """The state kept under the name `key` for a vector of `n` parameters, in `get_state`'s layout (fresh -- zero moments, the
        powers (beta1, beta2) -- when none is kept).  Unlike `get_state` it does not depend on which array object holds the
        parameters.  A kept state of another size is an error, never a silent restart."""
        flat = self._named.get(key)
        if flat is None:
            return np.concatenate([np.zeros(2 * n), np.array(self.beta, dtype=float)])
        if flat.size != 2 * n + 2:
            raise ValueError(f"AdaMax: the state kept under {key!r} is for {(flat.size - 2) // 2} parameters, not {n}: "
                             f"use a fresh optimizer for another problem")
        return flat.copy()

    def set_named_state(self, key, flat) -> None:
        self._named[key] = np.array(flat, dtype=np.float64).reshape(-1)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def _set_family(engine, family):
    """The kernel family of a device-paced run (its sweeps set no kernel from the host); an engine without families is SE only."""
    if hasattr(engine, "set_kernel_family"):
        engine.set_kernel_family(family)
    elif family != "se":
        raise TypeError(f"the engine has no kernel families: cannot train with {family!r}")


def perform_inference(theta, xtrain, ytrain, Xu, engine, *, batch_size=500, epochs=1, w_val=1e4, prior_var=50.0,
                      jitter=0.0, optimizer=None, learn_theta=True, device_paced=None, family="se"):
    """Returns (q_v of the last minibatch, theta) like `PerformInference` (:196-230).  `theta` is the raw
    (pre-softplus) parameter vector of `kernel_gp` (:108); `engine` an SGPDevice sized for `batch_size` points.

    device_paced (default: whenever the engine offers `train_begin` and the optimizer is fresh): the training set, theta and
    the optimiser state stay on the device and the loop below only enqueues (sgp_train_* in include/sgp_hip.h); otherwise
    every minibatch goes through the setters, `theta_objective` and the host-side `AdaMax` (the same arithmetic,
    host-paced).  Device-paced, a minibatch whose K_uu or Lambda is not positive definite is skipped and counted; the
    LinAlgError is raised after the run, not at the failing minibatch.  `family`: the kernel family ("se", "matern12",
    "matern32", "matern52"; `meta.kernel_family(kernel)`), with theta mapped as for SE."""
    theta = np.array(theta, dtype=np.float64)
    xtrain = np.asarray(xtrain, dtype=np.float64).reshape(len(ytrain), -1)
    Xu = np.asarray(Xu, dtype=np.float64).reshape(-1, xtrain.shape[1])
    M = Xu.shape[0]
    optimizer = optimizer or AdaMax()
    if device_paced is None:
        # (the device-paced run starts AdaMax from zero state and does not write the moments back: an optimizer that has
        # already taken steps keeps to the host-paced loop, which continues where it left off)
        device_paced = hasattr(engine, "train_begin") and not optimizer._state
    if device_paced:
        return _perform_inference_device(theta, xtrain, ytrain, Xu, engine, batch_size, epochs, w_val, prior_var, jitter,
                                         optimizer, learn_theta, family)
    xb, yb = split2batch((xtrain, np.asarray(ytrain, dtype=np.float64)), batch_size)
    engine.set_inducing(Xu)
    engine.set_noise([[w_val]])
    device_carry = hasattr(engine, "carry_posterior")
    mu, Sigma = np.zeros(M), prior_var * np.eye(M)
    zero, Lam_prior = np.zeros(M), np.eye(M) / prior_var
    for _ in range(epochs):
        mu, Sigma = np.zeros(M), prior_var * np.eye(M)                     # :203-204
        if device_carry:
            engine.set_prior_precision(zero, Lam_prior)                    # dense form: the captured graphs stay valid
        for xi, yi in zip(xb, yb):
            p = softplus(theta)
            if not device_carry:
                engine.set_prior_meancov(mu, Sigma)
            engine.set_data(xi, yi)
            set_engine_kernel(engine, float(p[0]), p[1:], jitter, family)  # :183-184 (no jitter in training)
            engine.sweep()                                                 # :185-192  infer(iterations = 1)
            if device_carry:
                engine.carry_posterior()                                   # :212 without leaving the device
            else:
                mu, Sigma, _ = engine.posterior(want_uv=False)
            if learn_theta:
                _, g = engine.theta_objective(want_grad=True, n_ell=len(p) - 1)    # :214-221
                optimizer.update(theta, g * sigmoid(theta))                # chain rule through softplus; :222
    if device_carry:
        mu, Sigma, _ = engine.posterior(want_uv=False)
    return MvNormalMeanCovariance(mu, Sigma), theta


def _perform_inference_device(theta, xtrain, ytrain, Xu, engine, batch_size, epochs, w_val, prior_var, jitter, optimizer,
                              learn_theta, family="se"):
    """The same loop with the device pacing itself: one `train_step` per minibatch, an isotropic-prior reset per epoch
    (:203-204); the host waits once, at the end."""
    N = len(ytrain)
    if optimizer._state:
        raise ValueError("perform_inference(device_paced=True) starts AdaMax from zero state; pass a fresh optimizer")
    engine.set_inducing(Xu)
    engine.set_noise([[w_val]])
    engine.set_prior_isotropic(prior_var)                                  # :203-204, put back by reset_prior every epoch
    _set_family(engine, family)
    engine.train_begin(xtrain, ytrain, theta, jitter=jitter, eta=optimizer.eta, beta=optimizer.beta, eps=optimizer.eps)
    for _ in range(epochs):
        for o in range(0, N, batch_size):
            engine.train_step(o, min(batch_size, N - o), learn_theta, reset_prior=(o == 0))
    theta, _, skipped = engine.train_end()
    if skipped:
        raise np.linalg.LinAlgError(f"{skipped} minibatch(es) had a K_uu or Lambda that is not positive definite")
    mu, Sigma, _ = engine.posterior(want_uv=False)
    return MvNormalMeanCovariance(mu, Sigma), np.asarray(theta)


def probit_marginal(y, mz, vz):
    """q(f) for `y ~ Probit(f)` with the forward message N(f; mz, vz): the moment-matched product of the UniSGP :out
    message with ReactiveMP's Probit(:in) message for a PointMass output (y in {0, 1}).  Returns (mean, variance)."""
    from scipy.special import log_ndtr
    y = np.asarray(y, dtype=np.float64)
    mz = np.asarray(mz, dtype=np.float64)
    s = 2.0 * y - 1.0
    g = s * mz / np.sqrt(1.0 + vz)
    r = np.exp(-0.5 * g * g - 0.5 * np.log(2.0 * np.pi) - log_ndtr(g))        # phi(g) / Phi(g)
    return mz + s * vz * r / np.sqrt(1.0 + vz), vz - vz * vz / (1.0 + vz) * r * (g + r)


def _host_free_energy(engine, sc, prior_var, shape, rate, a, b, N, lik=0.0):
    """The free energy of sgp_vmp_run (include/sgp_hip.h) after one host-paced iteration, by the same formulas in NumPy: the node
    energy at the NEW q(w) = Gamma(a, b), the Probit factors' share `lik`, KL(q(v) || N(0, prior_var I)) and KL(q(w) || p(w))."""
    from scipy.special import digamma, gammaln
    mu, Sigma, _ = engine.posterior(want_uv=False)
    M, S = mu.size, sc.sum_I1 + sc.sum_I2
    elog = digamma(a) - np.log(b)
    t0 = 0.5 * ((a / b) * S - N * elog + N * np.log(2.0 * np.pi))
    t2 = 0.5 * (np.trace(Sigma) / prior_var + mu @ mu / prior_var - M + M * np.log(prior_var) + sc.logdet_lambda)
    t3 = (a - shape) * digamma(a) - gammaln(a) + gammaln(shape) + shape * (np.log(b) - np.log(rate)) + a * (rate - b) / b
    return ((t0 + lik) + t2) + t3


def _vmp_device(engine, likelihood, iterations, shape, rate, free_energy):
    """The iteration loop as one sgp_vmp_run; returns what the host-paced loops return (and the trace)."""
    values, _, gamma, _, _ = engine.vmp_run(iterations, likelihood=likelihood, gamma_prior=(shape, rate))
    mu, Sigma, _ = engine.posterior(want_uv=False)
    out = (MvNormalMeanCovariance(mu, Sigma), (float(gamma[0]), float(gamma[1])))
    return out + (values,) if free_energy else out


def _vmp_regression_t(engine, xtrain, ytrain, nu, iterations, prior_var, shape, rate, device_paced, free_energy):
    """vmp_regression's loop for the Student-t likelihood `y_i ~ N(f_i, 1 / (w tau_i)), tau_i ~ Gamma(nu / 2, nu / 2)` with
    q(tau_i) = Gamma((nu + 1) / 2, beta_i) (include/sgp_hip.h, sgp_vmp_run_t).  Device-paced: one sgp_vmp_run_t.  Host-paced, per
    iteration and from existing calls alone: the data again with the point weights omega_i = alpha / beta_i, one sweep for q(v), q(w)
    from its sums, r_i = I1_i + I2_i from w_stats, and beta_i = nu / 2 + mean(q_w) r_i / 2."""
    from scipy.special import digamma, gammaln
    N, alpha, hn = len(ytrain), 0.5 * (nu + 1.0), 0.5 * nu
    if device_paced:
        values, _, gamma, beta, _, _ = engine.vmp_run_t(iterations, nu, gamma_prior=(shape, rate))
        a, b = float(gamma[0]), float(gamma[1])
        trace = values
    else:
        a, b, beta, trace = float(shape), float(rate), np.full(N, alpha), []
        for _ in range(iterations):
            engine.set_data(xtrain, ytrain, weights=alpha / beta)
            engine.set_noise([[a / b]])
            engine.sweep()
            sc = engine.scalars()
            a, b = shape + 0.5 * N, rate + 0.5 * (sc.sum_I1 + sc.sum_I2)
            I1, I2 = engine.w_stats()
            r = I1 + I2
            beta = hn + 0.5 * (a / b) * r
            if free_energy:
                S = np.sum(alpha / beta * r)
                kl = ((alpha - hn) * digamma(alpha) - gammaln(alpha) + gammaln(hn) + hn * (np.log(beta) - np.log(hn))
                      + alpha * (hn - beta) / beta)
                lik = np.sum(kl - 0.5 * (digamma(alpha) - np.log(beta)))
                # (the node energy at the NEW weights: their sum stands where the sweep's own sums do for the Gaussian likelihood)
                trace.append(_host_free_energy(engine, dataclasses.replace(sc, sum_I1=S, sum_I2=0.0), prior_var, shape, rate, a, b,
                                               N, lik))
        trace = np.array(trace)
    mu, Sigma, _ = engine.posterior(want_uv=False)
    out = (MvNormalMeanCovariance(mu, Sigma), (a, b), beta)
    return out + (trace,) if free_energy else out


def vmp_regression(p, xtrain, ytrain, Xu, engine, *, iterations=7, prior_var=50.0, shape=1e-2, rate=1e-2, jitter=1e-8,
                   family="se", device_paced=False, free_energy=False, student_t=None):
    """The inner `infer(...)` of experiments/GPT_regression.ipynb's `my_free_energy` (cell 9; model cell 6:
    `v ~ MvNormal(0, 50 I); w ~ Gamma(1e-2, 1e-2); y[i] ~ UniSGP(x[i], v, w, theta)`, mean field q(v) q(w), q(w) initialised
    at its prior, 7 iterations) at the kernel parameters p = (sigma2, lengthscale...) -- BASELINE config 1.  Per iteration:
    one sweep for q(v) at mean(q_w), then q(w) = Gamma(shape + N/2, rate + (sum I1 + sum I2)/2) from that q(v)
    (GPnode/UniSGPnode.jl:56-73,196-238).  Returns (q_v, (shape, rate)).
    student_t = nu replaces the Gaussian likelihood by Student-t with nu degrees of freedom, as a Gamma scale mixture with one
    q(tau_i) per point (robust to displaced targets; the engine needs keep_kuf).  Returns (q_v, (shape, rate), tau_rate)."""
    xtrain = np.asarray(xtrain, dtype=np.float64).reshape(len(ytrain), -1)
    Xu = np.asarray(Xu, dtype=np.float64).reshape(-1, xtrain.shape[1])
    p = np.asarray(p, dtype=np.float64)
    a, b = float(shape), float(rate)
    engine.set_inducing(Xu)
    set_engine_kernel(engine, float(p[0]), p[1:], jitter, family)
    engine.set_prior_isotropic(prior_var)
    engine.set_data(xtrain, np.asarray(ytrain, dtype=np.float64))
    if student_t is not None:
        return _vmp_regression_t(engine, xtrain, np.asarray(ytrain, dtype=np.float64), float(student_t), iterations, prior_var,
                                 float(shape), float(rate), device_paced, free_energy)
    if device_paced:                                   # the loop below as one sgp_vmp_run: the host waits once
        return _vmp_device(engine, "gaussian", iterations, shape, rate, free_energy)
    trace = []
    for _ in range(iterations):
        engine.set_noise([[a / b]])
        engine.sweep()
        sc = engine.scalars()
        a, b = shape + 0.5 * len(ytrain), rate + 0.5 * (sc.sum_I1 + sc.sum_I2)
        if free_energy:
            trace.append(_host_free_energy(engine, sc, prior_var, shape, rate, a, b, len(ytrain)))
    mu, Sigma, _ = engine.posterior(want_uv=False)
    if free_energy:
        return MvNormalMeanCovariance(mu, Sigma), (a, b), np.array(trace)
    return MvNormalMeanCovariance(mu, Sigma), (a, b)


def vmp_classification(p, xtrain, ytrain, Xu, engine, *, iterations=30, prior_var=50.0, shape=1e-2, rate=1e-2, jitter=0.0,
                       family="se", device_paced=False, free_energy=False):
    """The inner `infer(...)` of experiments/GPT_classification.ipynb's `my_free_energy` (cell 9; model cell 7:
    `f[i] ~ UniSGP(x[i], v, w, theta); y[i] ~ Probit(f[i])`, mean field q(f) q(v) q(w), q(v) and q(w) initialised at their
    priors, 30 iterations, K_uu without jitter).  Per iteration: q(f_i) from the :out message N(k_i' mu_v, 1 / mean(q_w))
    and the Probit likelihood, one sweep for q(v) with q_out = q(f), then q(w).  Returns (q_v, (shape, rate))."""
    xtrain = np.asarray(xtrain, dtype=np.float64).reshape(len(ytrain), -1)
    ytrain = np.asarray(ytrain, dtype=np.float64)
    Xu = np.asarray(Xu, dtype=np.float64).reshape(-1, xtrain.shape[1])
    p = np.asarray(p, dtype=np.float64)
    a, b = float(shape), float(rate)
    mu = np.zeros(Xu.shape[0])
    engine.set_inducing(Xu)
    set_engine_kernel(engine, float(p[0]), p[1:], jitter, family)
    engine.set_prior_isotropic(prior_var)
    reuse = getattr(engine, "reuse_stats", False)
    if device_paced:                                   # the loop below as one sgp_vmp_run: the host waits once
        engine.set_data(xtrain, ytrain)
        return _vmp_device(engine, "probit", iterations, shape, rate, free_energy)
    trace = []
    for it in range(iterations):
        w = a / b
        mz = engine.predict(xtrain, mu)
        mf, vf = probit_marginal(ytrain, mz, 1.0 / w)
        if it > 0 and reuse:
            engine.set_targets(mf, vf)         # x is fixed: only q(f) moves (the sweep then reuses K_uf, Psi2 and the K_uu chain)
        else:
            engine.set_data(xtrain, mf, vf)
        engine.set_noise([[w]])
        engine.sweep()
        sc = engine.scalars()
        a, b = shape + 0.5 * len(ytrain), rate + 0.5 * (sc.sum_I1 + sc.sum_I2)
        mu = engine.posterior(want_cov=False, want_uv=False)[0]
        if free_energy:
            from scipy.special import log_ndtr
            g = (2.0 * ytrain - 1.0) * mz / np.sqrt(1.0 + 1.0 / w)
            lik = np.sum(-0.5 * np.log(2.0 * np.pi / w) - 0.5 * w * ((mf - mz) ** 2 + vf) - log_ndtr(g))
            trace.append(_host_free_energy(engine, sc, prior_var, shape, rate, a, b, len(ytrain), lik))
    mu, Sigma, _ = engine.posterior(want_uv=False)
    if free_energy:
        return MvNormalMeanCovariance(mu, Sigma), (a, b), np.array(trace)
    return MvNormalMeanCovariance(mu, Sigma), (a, b)


def perform_inference_classification(theta, xtrain, ytrain, Xu, engine, *, batch_size=200, epochs=1, prior_var=50.0,
                                     shape=0.01, rate=0.01, jitter=1e-8, optimizer=None, device_paced=None, family="se"):
    """`PerformInference` of experiments/classification_banana.ipynb (model `f[i] ~ UniSGP(x[i], v, w, theta);
    y[i] ~ Probit(f[i])`, mean-field q(f) q(v) q(w), one VMP iteration per minibatch, q(v) and q(w) carried over every
    minibatch and never reset).  Per minibatch:
      q(f_i)  from the :out message N(k_i mu_v, 1 / mean(q_w)) (GPnode/UniSGPnode.jl:96-104) and the Probit likelihood;
      q(v)    one sweep with q_out = q(f_i) (the classification :v rule, :161-173);
      q(w)    Gamma(a + n/2, b + (sum I1 + sum I2)/2) with the NEW q(v) and the `meta.Uv` its product hook just stored
              (:56-73, :219-238);
      theta   one optimiser step on neg_log_backwardmess_fast with y_data = mean(q_f), w = mean(new q_w).
    Returns (q_v, (shape, rate), theta).

    The order of the updates inside the single VMP iteration is the reference scheduler's business (RxInfer / ReactiveMP, no
    pinned version); this is the order in which `meta.Uv` is refreshed by the product hook before the :w messages read it.
    Other orders were measured (tests/scripts/banana_schedules.py, profiles/*_train_banana_schedules.jsonl): none reproduces the
    reference's saved end point, see DESIGN.md section 2.

    device_paced (default: whenever the engine offers `train_begin`): the whole loop -- Probit moment matching, the Gamma
    update and AdaMax included -- runs on the device (sgp_train_begin with SGP_LIKELIHOOD_PROBIT); the host only enqueues."""
    theta = np.array(theta, dtype=np.float64)
    xtrain = np.asarray(xtrain, dtype=np.float64).reshape(len(ytrain), -1)
    ytrain = np.asarray(ytrain, dtype=np.float64)
    Xu = np.asarray(Xu, dtype=np.float64).reshape(-1, xtrain.shape[1])
    M = Xu.shape[0]
    optimizer = optimizer or AdaMax()
    if device_paced is None:
        device_paced = hasattr(engine, "train_begin") and not optimizer._state
    if device_paced:
        return _perform_inference_classification_device(theta, xtrain, ytrain, Xu, engine, batch_size, epochs, prior_var, shape,
                                                        rate, jitter, optimizer, family)
    xb, yb = split2batch((xtrain, ytrain), batch_size)
    a, b = float(shape), float(rate)
    engine.set_inducing(Xu)
    engine.set_prior_precision(np.zeros(M), np.eye(M) / prior_var)
    mu = np.zeros(M)
    first = True
    for _ in range(epochs):
        for xi, yi in zip(xb, yb):
            p = softplus(theta)
            w0 = a / b
            set_engine_kernel(engine, float(p[0]), p[1:], jitter, family)
            mz = engine.predict(xi, mu if first else None)             # k_i' mu_v with the carried posterior mean
            mf, vf = probit_marginal(yi, mz, 1.0 / w0)
            engine.set_data(xi, mf, vf)
            engine.set_noise([[w0]])
            engine.sweep()
            sc = engine.scalars()
            a, b = a + 0.5 * len(yi), b + 0.5 * (sc.sum_I1 + sc.sum_I2)
            engine.carry_posterior()
            engine.set_noise([[a / b]])                                # grad_llh_new!(...; w = mean(qw))
            _, g = engine.theta_objective(want_grad=True, n_ell=len(p) - 1)
            optimizer.update(theta, g * sigmoid(theta))
            first = False
    mu, Sigma, _ = engine.posterior(want_uv=False)
    return MvNormalMeanCovariance(mu, Sigma), (a, b), theta


def _perform_inference_classification_device(theta, xtrain, ytrain, Xu, engine, batch_size, epochs, prior_var, shape, rate, jitter,
                                             optimizer, family="se"):
    """The same loop paced by the device: one `train_step` per minibatch (window of the resident set; the forward message, the
    Probit moments, the Gamma update and AdaMax are kernels between the sweep's own), the host waits once, at the end."""
    N = len(ytrain)
    engine.set_inducing(Xu)
    engine.set_prior_isotropic(prior_var)                                  # q(v) starts at its prior and is never reset
    _set_family(engine, family)
    engine.train_begin(xtrain, ytrain, theta, jitter=jitter, eta=optimizer.eta, beta=optimizer.beta, eps=optimizer.eps,
                       likelihood="probit", gamma=(shape, rate))
    for _ in range(epochs):
        for o in range(0, N, batch_size):
            engine.train_step(o, min(batch_size, N - o), True, reset_prior=False)
    theta, _, skipped = engine.train_end()
    if skipped:
        raise np.linalg.LinAlgError(f"{skipped} minibatch(es) had a K_uu or Lambda that is not positive definite")
    a, b = engine.train_gamma()
    mu, Sigma, _ = engine.posterior(want_uv=False)
    return MvNormalMeanCovariance(mu, Sigma), (a, b), np.asarray(theta)


def _descend(theta, engine, steps, opt, exact=None):
    """`steps` device-paced AdaMax steps on `engine` (SGPDevice.theta_descend; `exact` = (means, covs, Y): theta_descend_psi on the
    exact statistics of those Gaussian inputs) with `opt`'s state for `theta` carried in and out; theta is updated in place."""
    kw = dict(eta=opt.eta, beta=opt.beta, eps=opt.eps, state=opt.get_state(theta))
    if exact is not None:
        th, _, _, state = engine.theta_descend_psi(*exact, theta, steps, **kw)
    else:
        th, _, _, state = engine.theta_descend(theta, steps, **kw)
    theta[...] = th.reshape(theta.shape)
    opt.set_state(theta, state)
    return theta


def optimize_theta_multi(theta, y_data, q_ins, q_v, q_w, meta, *, steps: int = 100, optimizer=None, grad_fn=None,
                         device_paced: bool = False, psi: str = "cubature"):
    """The inner loop of the pendulum's `PerformInference` (experiments/Pendulum_Wishart_2d.ipynb, cell 16): `steps` times
    grad_llh_multi! at the current theta with q(x), q(v) and q(W) held, then Flux.Optimise.update!(AdaMax, theta, grad).
    theta (raw, as meta.kernel maps it) is updated in place and returned.  The objective's inputs go to the device once; each
    step is one set_kernel and one sgp_theta_objective (multisgp.theta_objective_multi).  `grad_fn(theta) -> (value, grad)`
    replaces the device objective (a host restatement, for comparisons).  The optimiser runs on the host.

    device_paced=True: the same inputs are loaded the same way, then ONE sgp_theta_descend call takes all the steps on the
    device -- softplus map, objective, gradient and AdaMax -- and the host waits once.  The optimiser's moments for `theta` are
    read from and written back to `optimizer`, so successive calls continue one optimiser, host-paced or device-paced in any
    mix.  It needs meta.kernel.softplus_params (the device maps theta through softplus): ValueError otherwise.

    psi="exact": the objective over the closed-form Psi-statistics of the Gaussian inputs q_ins instead of their cubature points
    (SE kernel only): sgp_theta_objective_psi host-paced, sgp_theta_descend_psi device-paced."""
    from .multisgp import exact_theta_inputs, load_theta_objective_multi, theta_objective_multi
    theta = np.asarray(theta, dtype=np.float64)
    opt = optimizer if optimizer is not None else AdaMax()
    if device_paced:
        if grad_fn is not None:
            raise ValueError("optimize_theta_multi: device_paced=True evaluates the device objective; it takes no grad_fn")
        if not bool(getattr(meta.kernel, "softplus_params", False)):
            raise ValueError("optimize_theta_multi: device_paced=True maps theta through softplus on the device; "
                             "meta.kernel must have softplus_params set")
        from .meta import kernel_family
        eng, D_in = load_theta_objective_multi(y_data, q_ins, q_v, q_w, meta, psi)
        if theta.ndim != 1 or theta.size - 1 not in (1, D_in):
            raise ValueError(f"optimize_theta_multi: theta must be (sigma2, 1 or {D_in} lengthscales), got {theta.size} entries")
        sigma2, ell = meta.kernel(theta)
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))     # jitter and family of the descent
        return _descend(theta, eng, int(steps), opt, exact_theta_inputs(y_data, q_ins, meta) if psi == "exact" else None)
    evaluate = grad_fn if grad_fn is not None else theta_objective_multi(y_data, q_ins, q_v, q_w, meta, psi)
    for _ in range(int(steps)):
        _, g = evaluate(theta)
        opt.update(theta, np.asarray(g, dtype=np.float64))
    return theta


def optimize_theta(theta, engine, *, steps: int = 100, optimizer=None):
    """The UniSGP form of the same loop: `steps` device-paced AdaMax steps on neg_log_backwardmess_fast over an `engine`
    (SGPDevice) that has data, noise, a kernel (its family and jitter are kept; its values are replaced by softplus(theta)) and
    a swept q(v), all held.  theta (raw, pre-softplus, sigma2 first) is updated in place and returned; `optimizer`'s moments
    for it are carried in and out as in `optimize_theta_multi`."""
    theta = np.asarray(theta, dtype=np.float64)
    opt = optimizer if optimizer is not None else AdaMax()
    return _descend(theta, engine, int(steps), opt)


INDUCING_STATE = "optimize_inducing"      # the name `optimize_inducing(device_paced=True)` keeps its joint state under (AdaMax.get_named_state)


def optimize_inducing(theta, Xu, engine, *, q_v, steps: int = 100, optimizer=None, learn_theta: bool = True, jitter: float = 0.0,
                      psi: str = "cubature", inputs=None, device_paced: bool = False):
    """`steps` host-paced AdaMax steps on the objective of `theta_objective` in the inducing inputs -- on [theta | vec Xu] together,
    or on Xu alone with learn_theta=False -- over an `engine` (SGPDevice) that has data, noise and a kernel family, with q(v) held
    for the whole call.  theta is raw (pre-softplus, sigma2 first, 1 or D lengthscales); Xu is (M, D); q_v is (mu_v, Uv) as
    `set_posterior` takes them, or a distribution with `mean_cov()` (Uv = chol(Sigma_v + mu mu').U is then formed here).

    Per step: set_kernel(softplus(theta), jitter), set_inducing(Xu), one `theta_objective_xu` (value, d/d(sigma2, ell), d/dXu),
    the chain rule through softplus for theta, one optimiser update of the joint vector.  `set_inducing` withdraws the handle's
    finished-sweep mark, and with it the q(v) the objective would use (sgp_theta_objective then refuses), so q_v is installed
    again with `set_posterior` after every `set_inducing`.  Returns (theta, Xu, values): new arrays, values[k] the objective at
    step k's parameters; the engine is left at the LAST EVALUATED parameters, one update behind the returned ones.

    With q(v) held, moving z_m reinterprets v_m as the function value at the new location: the objective is a function of Xu only
    through that reading, and q(v) is no longer the posterior of any sweep once Xu has moved.  The intended use is alternation --
    a few steps here, then sweeps at the new Xu to refit q(v).  The reference never moves Xu; there is no counterpart of this
    loop in it.

    psi="exact" with inputs=(mean, cov, y_mean) as `theta_objective_psi` takes them: the same loop on the objective over the exact
    Psi-statistics of the Gaussian inputs (SE kernel only), one `theta_objective_psi_xu` per step; no resident data are needed.

    device_paced=True: set_kernel, set_inducing and set_posterior run ONCE, then one `inducing_descend` (psi="exact":
    `inducing_descend_psi`) call takes all the steps on the device and the host waits once.  The same (theta, Xu, values) come
    back (new arrays), but the engine ends AT the returned parameters, whereas the host-paced engine ends one update behind them.
    The optimiser's state for the joint vector x = [theta | vec Xu] (vec Xu with learn_theta=False) is read from and written back
    to `optimizer` under the name INDUCING_STATE (`optimizer.get_named_state(INDUCING_STATE, x.size)`), so successive device-paced
    calls with one optimizer continue one optimiser whatever array objects carry theta and Xu; an optimizer that holds such a
    state for another number of parameters raises ValueError.  To continue on the host, install it for the joint array:
    `optimizer.set_state(x, optimizer.get_named_state(INDUCING_STATE, x.size))`; to hand host-paced moments to the device,
    `optimizer.set_named_state(INDUCING_STATE, optimizer.get_state(x))`."""
    if psi not in ("cubature", "exact"):
        raise ValueError(f"optimize_inducing: psi must be 'cubature' or 'exact', got {psi!r}")
    if psi == "exact":
        if inputs is None:
            raise ValueError("optimize_inducing: psi='exact' needs inputs=(mean, cov, y_mean)")
        if getattr(engine, "kernel_family", "se") != "se":
            raise ValueError("optimize_inducing: psi='exact' exists for the SE kernel only")
    theta = np.array(theta, dtype=np.float64).reshape(-1)
    Xu = np.array(Xu, dtype=np.float64)
    if Xu.ndim != 2:
        raise ValueError(f"optimize_inducing: Xu must be (M, D), got shape {Xu.shape}")
    M, D = Xu.shape
    if theta.size - 1 not in (1, D):
        raise ValueError(f"optimize_inducing: theta must be (sigma2, 1 or {D} lengthscales), got {theta.size} entries")
    if hasattr(q_v, "mean_cov"):
        mu_v, Sigma_v = q_v.mean_cov()
        mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
        Uv = np.linalg.cholesky(np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v)).T
    else:
        mu_v, Uv = q_v
    opt = optimizer if optimizer is not None else AdaMax()
    nt = theta.size if learn_theta else 0
    x = np.concatenate([theta[:nt], Xu.ravel()])
    if device_paced:
        kw = dict(learn_theta=learn_theta, eta=opt.eta, beta=opt.beta, eps=opt.eps, state=opt.get_named_state(INDUCING_STATE, x.size))
        p = softplus(theta)
        engine.set_kernel(float(p[0]), p[1:], jitter)
        engine.set_inducing(Xu)
        engine.set_posterior(mu_v, Uv)
        if psi == "exact":
            th, Z, values, _, state = engine.inducing_descend_psi(*inputs, theta, Xu, int(steps), **kw)
        else:
            th, Z, values, _, state = engine.inducing_descend(theta, Xu, int(steps), **kw)
        opt.set_named_state(INDUCING_STATE, state)
        return (np.array(th, dtype=np.float64).reshape(-1) if learn_theta else theta), np.array(Z, dtype=np.float64).reshape(M, D), values
    values = np.empty(max(int(steps), 0))
    for k in range(int(steps)):
        th = x[:nt] if learn_theta else theta
        p = softplus(th)
        engine.set_kernel(float(p[0]), p[1:], jitter)
        engine.set_inducing(x[nt:].reshape(M, D))
        engine.set_posterior(mu_v, Uv)
        if psi == "exact":
            values[k], g, gxu = engine.theta_objective_psi_xu(*inputs, want_grad=True)
        else:
            values[k], g, gxu = engine.theta_objective_xu(want_grad=True)
        grad = np.concatenate([(np.asarray(g) * sigmoid(th))[:nt], np.asarray(gxu, dtype=np.float64).ravel()])
        opt.update(x, grad)
    return (x[:nt].copy() if learn_theta else theta), x[nt:].reshape(M, D).copy(), values


def select_inducing(X, m, theta, engine, *, family="se", tol=0.0, min_var=1e-12, install=True):
    """A starting Xu for `engine` (SGPDevice): the `m` candidates among the rows of X (n, D) that greedy conditional-variance
    selection picks at the kernel of raw theta (pre-softplus, sigma2 first, 1 or D lengthscales) -- `engine.select_inducing`, the
    partial pivoted Cholesky factorisation of K_ff.  The kernel is set as `optimize_inducing` sets it, set_kernel(softplus(theta))
    with `family` and jitter 0 (the selection uses no jitter; the caller's next set_kernel brings its own); with install=True the
    picks are installed with set_inducing(X[idx]).  Targets, q(v) and the resident data play no part.

    Returns (Xu, idx, trace): Xu = X[idx] (m, D), trace[j] = tr(K_ff - Q_ff) of the first j picks (trace[0] = n sigma2).  The
    engine takes exactly engine.M inducing inputs: m != engine.M, or a selection that a stop rule (tol, min_var: duplicates and
    candidates inside the span of the picks are never taken) ended short of m, raises ValueError and installs nothing."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(f"select_inducing: X must be (n, D), got shape {X.shape}")
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if theta.size - 1 not in (1, X.shape[1]):
        raise ValueError(f"select_inducing: theta must be (sigma2, 1 or {X.shape[1]} lengthscales), got {theta.size} entries")
    if int(m) != engine.M:
        raise ValueError(f"select_inducing: the engine holds M = {engine.M} inducing inputs, m = {m} were asked for")
    p = softplus(theta)
    engine.set_kernel(float(p[0]), p[1:], 0.0, family=family)
    idx, trace = engine.select_inducing(X, int(m), tol=tol, min_var=min_var)
    if len(idx) != engine.M:
        raise ValueError(f"select_inducing: the selection stopped after {len(idx)} of {engine.M} picks (tol = {tol}, min_var = "
                         f"{min_var}; residual trace {trace[-1]:.3e} of {trace[0]:.3e}): use a smaller engine or looser stop rules")
    Xu = X[idx].copy()
    if install:
        engine.set_inducing(Xu)
    return Xu, idx, trace


# ------------------------------------------------------------------------------------------------
# the GP state-space model: `pendulum_GP` of experiments/Pendulum_Wishart_2d.ipynb (cells 12-16)
# ------------------------------------------------------------------------------------------------
def wishart_mean_logdet(nu: float, invscale) -> float:
    """E[logdet W] of WishartFast(nu, invscale): sum_i digamma((nu + 1 - i) / 2) + d log 2 - logdet(invscale)."""
    from scipy.special import digamma
    invscale = np.atleast_2d(np.asarray(invscale, dtype=np.float64))
    d = invscale.shape[0]
    return float(sum(digamma(0.5 * (nu - i)) for i in range(d)) + d * np.log(2.0) - np.linalg.slogdet(invscale)[1])


def _gauss_kl(m, S, m0, S0) -> float:
    """KL(N(m, S) || N(m0, S0))."""
    d = len(m)
    S0inv = np.linalg.inv(S0)
    dm = m - m0
    return float(0.5 * (np.trace(S0inv @ S) + dm @ S0inv @ dm - d + np.linalg.slogdet(S0)[1] - np.linalg.slogdet(S)[1]))


def _wishart_kl(nu, invS, nu0, invS0) -> float:
    """KL(Wishart(nu, invS^-1) || Wishart(nu0, invS0^-1)), both given by their inverse scales."""
    from scipy.special import multigammaln
    d = invS.shape[0]
    V = np.linalg.inv(invS)
    return float(0.5 * nu0 * (np.linalg.slogdet(invS)[1] - np.linalg.slogdet(invS0)[1]) + 0.5 * nu * (np.trace(invS0 @ V) - d)
                 + multigammaln(0.5 * nu0, d) - multigammaln(0.5 * nu, d)
                 + 0.5 * (nu - nu0) * (wishart_mean_logdet(nu, invS) - d * np.log(2.0) + np.linalg.slogdet(invS)[1]))


def vmp_regression_multi(theta, X, Y, meta, *, iterations=10, v_prior_var=50.0, w_prior=None, device_paced=True, free_energy=True,
                         q_ins=None):
    """`infer(iterations = K, free_energy = true)` of multi-output regression with a learned full noise precision:
        y_t ~ MultiSGP(x_t, v, W, theta),   v ~ N(0, v_prior_var I),   W ~ Wishart(nu0, invscale^-1),   mean field q(v) q(W).
    theta is raw, as meta.kernel maps it; Y is (T, d), d = 2 .. 4; w_prior = (nu0, inverse scale), default (d + 2, I); q(W) starts at
    its prior.  The inputs are the rows of X as PointMass, or q_ins: Gaussians held fixed, which enter through meta.method's cubature
    points as weighted data (steps 4-5 of `vmp_gpssm` at a held q(x)).  Per iteration: q(v) from one sweep at mean(q_W) and
    E[logdet W], then q(W) = Wishart(nu0 + T, prior + sum_t (I1_t + I2_t)); the free energy is the summed average energy at the new
    q(W) plus KL(q(v) || p(v)) and KL(q(W) || p(W)).
    device_paced: one `SGPDevice.vmp_run_w` (sgp_vmp_run_w), the host waits once.  Otherwise the host-paced loop of existing calls:
    `multisgp.sweep`, `multisgp.rule_w_summed`, `multisgp.average_energy_summed` and the KL helpers of this module.
    Returns (q_v, q_W) or, with free_energy, (q_v, q_W, free energies [iterations])."""
    from . import multisgp as MS
    from .distributions import MvNormalWeightedMeanPrecision, PointMass, WishartFast
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or not 2 <= Y.shape[1] <= 4:
        raise ValueError("vmp_regression_multi: Y must be (T, d) with d = 2 .. 4")
    T, d = Y.shape
    if q_ins is None:
        q_ins = [PointMass(x) for x in np.asarray(X, dtype=np.float64).reshape(T, -1)]
    if len(q_ins) != T:
        raise ValueError(f"vmp_regression_multi: {len(q_ins)} inputs for {T} targets")
    q_outs = [PointMass(y) for y in Y]
    nu0, R0 = (d + 2.0, np.eye(d)) if w_prior is None else (float(w_prior[0]), np.asarray(w_prior[1], dtype=np.float64))
    Q = d * np.asarray(meta.Xu).shape[0]
    q_theta = PointMass(np.asarray(theta, dtype=np.float64))
    v_prior = MvNormalWeightedMeanPrecision(np.zeros(Q), np.eye(Q) / v_prior_var)
    q_w = WishartFast(nu0, R0)
    q_v = MvNormalMeanCovariance(np.zeros(Q), v_prior_var * np.eye(Q))   # (iterations = 0: the prior, nothing is swept)
    if int(iterations) <= 0:
        return (q_v, q_w, np.zeros(0)) if free_energy else (q_v, q_w)
    if device_paced:
        eng = MS.load(meta, q_outs, q_ins, q_w, q_theta, v_prior, E_logdet_W=wishart_mean_logdet(nu0, R0))
        trace, _, q_w, _, _ = eng.vmp_run_w(int(iterations), wishart_prior=(nu0, R0))
        mu, Sigma, _ = eng.posterior(want_uv=False)
        q_v = MvNormalMeanCovariance(mu, Sigma)
    else:
        trace = []
        for _ in range(int(iterations)):
            W_old, el_old = q_w.mean(), wishart_mean_logdet(q_w.nu, q_w.invS)
            q_v = MS.sweep(meta, q_outs, q_ins, q_w, q_theta, v_prior, E_logdet_W=el_old)
            q_w = MS.rule_w_summed(meta, nu0, R0, T)
            if free_energy:
                energy_old = MS.average_energy_summed(meta)   # at the q(W) the sweep ran at
                # the node energy is linear in (W_bar, E[logdet W]): moved to the NEW q(W), where sgp_vmp_run_w evaluates it
                S = q_w.invS - R0
                energy = energy_old + 0.5 * (np.sum((q_w.mean() - W_old) * S) - T * (wishart_mean_logdet(q_w.nu, q_w.invS) - el_old))
                trace.append(energy + _gauss_kl(q_v.m, q_v.S, np.zeros(Q), v_prior_var * np.eye(Q)) + _wishart_kl(q_w.nu, q_w.invS, nu0, R0))
        trace = np.array(trace)
    return (q_v, q_w, trace) if free_energy else (q_v, q_w)


def gpssm_host_energy(y, Pobs, q_x, q_v, q_w, x0_prior, v_prior_var, w_prior) -> float:
    """The host's share of the GP-SSM free energy: the observation factors' average energies, KL(q(x_0) || prior), minus the
    entropies of q(x_1..T), KL(q(v) || N(0, v_prior_var I)) and KL(q(W) || prior).  The MultiSGP factors' average energies
    (`multisgp.average_energy_summed`) complete it."""
    y = np.asarray(y, dtype=np.float64)
    d = y.shape[1]
    Pinv = np.linalg.inv(Pobs)
    ldP = float(np.linalg.slogdet(Pobs)[1])
    total = _gauss_kl(q_x[0].m, q_x[0].S, np.asarray(x0_prior[0], dtype=np.float64), np.asarray(x0_prior[1], dtype=np.float64))
    for t in range(1, len(q_x)):
        r = y[t - 1] - q_x[t].m
        total += 0.5 * (d * np.log(2.0 * np.pi) + ldP + r @ Pinv @ r + np.trace(Pinv @ q_x[t].S))
        total -= 0.5 * (d * (1.0 + np.log(2.0 * np.pi)) + np.linalg.slogdet(q_x[t].S)[1])
    mu, Sig = q_v.mean_cov()
    Q = len(mu)
    total += 0.5 * ((np.trace(Sig) + mu @ mu) / v_prior_var - Q + Q * np.log(v_prior_var) - np.linalg.slogdet(Sig)[1])
    total += _wishart_kl(q_w.nu, q_w.invS, float(w_prior[0]), np.asarray(w_prior[1], dtype=np.float64))
    return float(total)


def gpssm_initial_marginals(T: int, d: int, Q: int, x0_prior, v_prior_var: float, w_prior):
    """The notebook's `@initialization` (cell 14): q(x_t) = N(0, 50 I) for t = 1..T, q(v) = N(0, v_prior_var I), q(W) = the prior.
    x_prev (x_0) is not named there: q(x_0) starts at its prior."""
    from .distributions import WishartFast
    q_x = [MvNormalMeanCovariance(np.array(x0_prior[0], dtype=np.float64), np.array(x0_prior[1], dtype=np.float64))]
    q_x += [MvNormalMeanCovariance(np.zeros(d), 50.0 * np.eye(d)) for _ in range(T)]
    return q_x, MvNormalMeanCovariance(np.zeros(Q), v_prior_var * np.eye(Q)), WishartFast(float(w_prior[0]), np.array(w_prior[1], dtype=np.float64))


def _proper_gaussian(q, floor: float = 1e-10):
    """q itself when cov(q) has a Cholesky factor; otherwise the same mean with the covariance's eigenvalues raised to
    floor * max(1, largest).  A moment-matched covariance whose closure values single out one cubature point is singular to
    rounding, and the next step takes its cubature points through a Cholesky factor; ReactiveMP factors such a matrix with a
    forced-positive Cholesky (`cholsqrt`), which has the same purpose and not the same values."""
    try:
        np.linalg.cholesky(q.S)
        return q
    except np.linalg.LinAlgError:
        w, V = np.linalg.eigh(0.5 * (q.S + q.S.T))
        w = np.maximum(w, floor * max(1.0, float(w[-1])))
        return MvNormalMeanCovariance(q.m, (V * w) @ V.T)


def vmp_gpssm(theta, y, meta, *, P, x0_prior, v_prior_var=50.0, w_prior=None, iterations=10, init=None, free_energy=False,
              rule_out_fn=None, psi="cubature", in_psi="cubature"):
    """The inner `infer(...)` of the pendulum GP-SSM (experiments/Pendulum_Wishart_2d.ipynb cells 12-16):
        x_0 ~ N(m0, P0);   x_t ~ MultiSGP(x_{t-1}, v, W, theta);   y_t ~ N(x_t, P),   t = 1..T,
        v ~ N(0, v_prior_var I),   W ~ Wishart(nu0, invscale^-1),   mean field q(x_0) .. q(x_T) q(v) q(W).
    theta is raw, as meta.kernel maps it; y is (T, d); x0_prior = (m0, P0); w_prior = (nu0, inverse scale), default (100, I).
    The marginals start at the notebook's `@initialization` (`gpssm_initial_marginals`), or at init = (q_x, q_v, q_W).

    Every iteration is a fixed Jacobi schedule: each step's messages are computed from the marginals the previous step left.
      1. the forward messages out_t = MultiSGP(:out) at q(x_{t-1}), t = 1..T: `multisgp.rule_out_batch`, ONE device call;
      2. left_t = out_t x N(y_t, P) for t >= 1 (a d x d Gaussian product on the host), left_0 = N(m0, P0);
      3. q(x_t), t = 0..T-1 = left_t x the :in message of node t + 1, whose closure uses q_out = q(x_{t+1}) of the previous
         iteration: `multisgp.marginal_in_batch`, ONE device call (with the reference's NaN fallback; a covariance that is singular to
         rounding has its eigenvalues floored, `_proper_gaussian`); q(x_T) = left_T;
      4. q(v): `multisgp.sweep` over all nodes with the new q(x), one sweep;
      5. q(W) = Wishart(nu0 + T, prior + sum_t (I1_t + I2_t)): `multisgp.rule_w_summed`.
    free_energy: after step 4, at (new q(x), new q(v), the q(W) of steps 1-4), the free energy is the MultiSGP factors' average
    energies from the sweep (`multisgp.average_energy_summed`) plus the Gaussian and Wishart terms of `gpssm_host_energy`.
    What stays on the host per iteration: the cubature points of 2 T Gaussians, T products of d x d Gaussians, the NaN test.

    This is a schedule of the same messages; ReactiveMP's reactive update order is NOT claimed to be reproduced, and no fixture
    pins it: the notebook's data come from Julia's MersenneTwister(124), so its q(x) cannot be regenerated here.

    psi: "cubature" (default) takes the Psi-statistics of steps 1 and 4 over meta.method's cubature points; "exact" takes them in
    closed form (`cubature.ExactSE`: `SGPDevice.psi_stats` for step 1, `sweep_local_psi` for step 4; SE kernel only).  Steps 2, 3
    and 5 are the same either way: the :in closure of step 3 is no expectation of the kernel and stays on cubature points.
    in_psi: "cubature" (default) is step 3 as above; "exact" (SE kernel only) replaces it by one natural-gradient step of every
    q(x_t), t = 0..T-1, from the previous iteration's q(x_t), on L_t(q) = KL(q || left_t) + U_{t+1}(q) with U the closed-form energy of
    node t + 1 in its input (`multisgp.marginal_in_exact_batch`, `SGPDevice.psi_in_grad`): the functional psi="exact" sweeps on.  L_t
    does not rise at any node; the simultaneous update of all nodes does not make the global free energy monotone.
    rule_out_fn(q_ins, q_v, q_w, q_theta, meta) replaces step 1's batch function (timing comparisons against the per-node loop).
    Returns (q_x [T + 1], q_v, q_W, free energies [iterations] or [])."""
    from . import multisgp as MS
    from .distributions import MvNormalWeightedMeanPrecision, PointMass
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("vmp_gpssm: y must be (T, d)")
    T, d = y.shape
    Pobs = np.asarray(P, dtype=np.float64).reshape(d, d)
    Pinv = np.linalg.inv(Pobs)
    m0, P0 = np.asarray(x0_prior[0], dtype=np.float64), np.asarray(x0_prior[1], dtype=np.float64)
    w_prior = (100.0, np.eye(d)) if w_prior is None else (float(w_prior[0]), np.asarray(w_prior[1], dtype=np.float64))
    Q = d * np.asarray(meta.Xu).shape[0]
    q_theta = PointMass(np.asarray(theta, dtype=np.float64))
    q_x, q_v, q_w = init if init is not None else gpssm_initial_marginals(T, d, Q, (m0, P0), v_prior_var, w_prior)
    q_x = list(q_x)
    v_prior = MvNormalWeightedMeanPrecision(np.zeros(Q), np.eye(Q) / v_prior_var)
    rule_out_fn = rule_out_fn or MS.rule_out_batch
    if psi not in ("cubature", "exact"):
        raise ValueError(f"vmp_gpssm: psi must be 'cubature' or 'exact', got {psi!r}")
    if in_psi not in ("cubature", "exact"):
        raise ValueError(f"vmp_gpssm: in_psi must be 'cubature' or 'exact', got {in_psi!r}")
    if in_psi == "exact":
        from .cubature import require_se
        from .meta import kernel_family
        require_se(kernel_family(meta.kernel))

    run_meta = meta
    if psi == "exact":
        # one meta for the whole run whose method is the marker: steps 1 and 4 dispatch on it, step 3 names its own cubature rule.
        # It shares the caller's engine and hands back the one it ends with.
        import dataclasses
        from .cubature import ExactSE
        run_meta = dataclasses.replace(meta, method=ExactSE())
    try:
        return _vmp_gpssm_loop(run_meta, y, q_x, q_v, q_w, q_theta, v_prior, rule_out_fn, int(iterations), free_energy,
                               (m0, P0), Pobs, Pinv, v_prior_var, w_prior, in_psi)
    finally:
        meta.engine = run_meta.engine


def _vmp_gpssm_loop(meta, y, q_x, q_v, q_w, q_theta, v_prior, rule_out_fn, iterations, free_energy, x0_prior, Pobs, Pinv,
                    v_prior_var, w_prior, in_psi="cubature"):
    """The iterations of `vmp_gpssm` (its docstring numbers the steps) on the meta whose method says how steps 1 and 4 take their
    Psi-statistics; in_psi says how step 3 updates q(x)."""
    from . import multisgp as MS
    T = len(y)
    m0, P0 = x0_prior
    fe = []
    for _ in range(iterations):
        W = q_w.mean()
        outs = rule_out_fn(q_x[:-1], q_v, q_w, q_theta, meta)                                   # 1
        S = np.linalg.inv(W + Pinv)                                                             # 2 (every out_t carries precision W)
        S = 0.5 * (S + S.T)
        lefts = [MvNormalMeanCovariance(m0, P0)] + [MvNormalMeanCovariance(S @ (W @ outs[t].m + Pinv @ y[t]), S) for t in range(T)]
        if in_psi == "exact":                                                                   # 3
            q_x = MS.marginal_in_exact_batch(q_x[1:], lefts[:-1], q_x[:-1], q_v, q_w, q_theta, meta)[0] + [lefts[-1]]
        else:
            q_x = [_proper_gaussian(q) for q in MS.marginal_in_batch(q_x[1:], lefts[:-1], q_v, q_w, q_theta, meta)] + [lefts[-1]]
        q_v = MS.sweep(meta, q_x[1:], q_x[:-1], q_w, q_theta, v_prior, E_logdet_W=wishart_mean_logdet(q_w.nu, q_w.invS))   # 4
        if free_energy:
            fe.append(MS.average_energy_summed(meta) + gpssm_host_energy(y, Pobs, q_x, q_v, q_w, (m0, P0), v_prior_var, w_prior))
        q_w = MS.rule_w_summed(meta, w_prior[0], w_prior[1], T)                                 # 5
    return q_x, q_v, q_w, fe


def perform_inference_gpssm(theta, y, meta, *, P, x0_prior, epochs, vmp_iterations=10, theta_steps=100, device_paced=True,
                            v_prior_var=50.0, w_prior=None, optimizer=None, free_energy=True, psi="cubature",
                            theta_psi="cubature", in_psi="cubature"):
    """`PerformInference` of experiments/Pendulum_Wishart_2d.ipynb cell 16.  Per epoch: `vmp_gpssm` from the initialisation at
    the current theta (step 1), then `optimize_theta_multi` -- theta_steps AdaMax steps on neg_log_backwardmess_multi -- at the held
    q(x), q(v), q(W), with the targets mean(q(x_t)) and the inputs q(x_{t-1}), t = 1..T, as the notebook passes them (step 2).
    One optimiser is carried across the epochs (the notebook creates its Flux.AdaMax() once): `optimizer`, or a fresh AdaMax;
    device_paced passes its state through sgp_theta_descend's opt_state.  theta (raw) is updated in place.
    theta_psi="exact": step 2 descends on the objective over the exact Psi-statistics of q(x_{t-1}) (`optimize_theta_multi(psi=
    "exact")`) -- with psi="exact" the objective the sweeps of step 1 minimise; the default loads the cubature points as before.
    Returns (theta, free energies [epochs] (the last iteration's of every epoch, or []), (q_x, q_v, q_W) of the last epoch)."""
    theta = np.array(theta, dtype=np.float64)
    opt = optimizer if optimizer is not None else AdaMax()
    fe_values, post = [], None
    for _ in range(int(epochs)):
        q_x, q_v, q_w, fe = vmp_gpssm(theta, y, meta, P=P, x0_prior=x0_prior, v_prior_var=v_prior_var, w_prior=w_prior,
                                      iterations=vmp_iterations, free_energy=free_energy, psi=psi, in_psi=in_psi)
        if fe:
            fe_values.append(fe[-1])
        y_data = np.stack([q.m for q in q_x[1:]])
        optimize_theta_multi(theta, y_data, q_x[:-1], q_v, q_w, meta, steps=theta_steps, optimizer=opt, device_paced=device_paced,
                             psi=theta_psi)
        post = (q_x, q_v, q_w)
    return theta, fe_values, post


def sample_posterior(meta, Xstar, n_samples, rng, *, q_v, q_theta, q_w=None, noise=False, sample_jitter=None):
    """Whole functions from the posterior: n_samples joint draws of the latent f (noise=True: of the observation, + mean(q_w)^-1 per
    point) at the test inputs Xstar (ns, D), at kernel(q_theta) and the explicit q_v -- ONE `SGPDevice.sample_f` call on meta's
    engine (UniSGPMeta or MultiSGPMeta).  The standard normals come from `rng` (a numpy.random.Generator): the library holds no
    random state, so a seeded generator reproduces the draws bitwise.  sample_jitter (default 1e-9 sigma2) is added to the joint
    covariance's diagonal before it is factored; nearly coincident test points need more.  Returns (mean (ns, d_out), samples
    (n_samples, ns, d_out)); ns * d_out is limited to SGP_JOINT_MAX_ROWS = 8192."""
    from . import multisgp as MS
    from . import unisgp as US
    from .meta import kernel_family, set_engine_kernel
    Xu = np.asarray(meta.Xu)
    M, D = Xu.shape
    X = np.asarray(Xstar, dtype=np.float64).reshape(-1, D)
    ns, n_samples = X.shape[0], int(n_samples)
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    d_out = mu_v.size // M
    multi = isinstance(meta, MS.MultiSGPMeta)
    eng = MS._engine(meta, 1, d_out) if multi else US._engine(meta, 1)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    if noise:
        if q_w is None:
            raise ValueError("sample_posterior: noise=True needs q_w")
        if multi:
            eng.set_noise(MS._mean_W(q_w))
        else:
            eng.set_noise([[US._mean_w(q_w)]], US._elog_w(q_w))
    eps = rng.standard_normal((ns * d_out, n_samples))
    jit = 1e-9 * float(sigma2) if sample_jitter is None else float(sample_jitter)
    mean, smp = eng.sample_f(X, eps, jit, mu_v, np.asarray(Sigma_v, dtype=np.float64), noise=noise)
    return np.asarray(mean).reshape(ns, d_out), smp.T.reshape(n_samples, d_out, ns).transpose(0, 2, 1).copy()


MATERN_NU2 = {"matern12": 1, "matern32": 3, "matern52": 5}       # 2 nu of the Matern families


def path_features(family, D, L, rng):
    """Random Fourier features of a kernel family on 1 / ell-scaled inputs, as `SGPDevice.sample_path` takes them: (omega (D, L),
    phase (L,)), so that E[phi(x)' phi(x')] = k(x, x') for phi_l(x) = sqrt(2 sigma2 / L) cos(phase_l + omega[:, l] . x / ell).  SE:
    omega[:, l] ~ N(0, I).  Matern-nu: N(0, I) / sqrt(g_l / (2 nu)) with one g_l ~ chi2(2 nu) per feature -- the multivariate
    Student-t with 2 nu degrees of freedom, the spectral measure of the families as `sgp_set_kernel_family` defines them.  phase ~
    U[0, 2 pi).  Drawn from `rng` in the order omega's normals, g, phase."""
    from ._lib import family_id, KERNEL_FAMILIES
    name = {v: k for k, v in KERNEL_FAMILIES.items()}[family if isinstance(family, (int, np.integer)) else family_id(family)]
    D, L = int(D), int(L)
    omega = rng.standard_normal((D, L))
    if name != "se":
        nu2 = MATERN_NU2[name]
        omega = omega / np.sqrt(rng.chisquare(nu2, L) / nu2)
    return omega, rng.uniform(0.0, 2.0 * np.pi, L)


def _path_engine(meta, q_v, q_theta):
    """(engine at kernel(q_theta), family, mu_v (Q,), Sigma_v (Q, Q), d_out) for the pathwise samplers"""
    from . import multisgp as MS
    from . import unisgp as US
    from .meta import kernel_family, set_engine_kernel
    M = np.asarray(meta.Xu).shape[0]
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    d_out = mu_v.size // M
    eng = MS._engine(meta, 1, d_out) if isinstance(meta, MS.MultiSGPMeta) else US._engine(meta, 1)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    family = kernel_family(meta.kernel)
    set_engine_kernel(eng, sigma2, ell, meta.jitter, family)
    return eng, family, mu_v, np.asarray(Sigma_v, dtype=np.float64), d_out


def _noise_factor(meta, q_w, d_out, what):
    """the lower factor of mean(q_w)^-1 (d_out x d_out)"""
    from . import multisgp as MS
    from . import unisgp as US
    if q_w is None:
        raise ValueError(f"{what}: noise=True needs q_w")
    W = MS._mean_W(q_w) if isinstance(meta, MS.MultiSGPMeta) else np.array([[US._mean_w(q_w)]])
    if W.shape != (d_out, d_out):
        raise ValueError(f"{what}: mean(q_w) must be {d_out} x {d_out}, got {W.shape}")
    return np.linalg.cholesky(np.linalg.inv(W))


def sample_paths(meta, Xstar, n_samples, rng, *, q_v, q_theta, features=1024, q_w=None, noise=False):
    """Whole functions from the posterior by pathwise (Matheron) sampling over `features` random Fourier features: n_samples draws
    of the latent f (noise=True: of the observation, + mean(q_w)^-1 noise per point, added on the host) at the test inputs Xstar
    (ns, D), at kernel(q_theta) and the explicit q_v -- ONE `SGPDevice.sample_path` call on meta's engine.  Unlike
    `sample_posterior` the cost is linear in ns and ns is not limited; the prior part of a draw is its random-feature approximation.
    Everything random comes from `rng`, in the order path_features, feat_w, eps_v, noise: a seeded generator reproduces the draws
    bitwise.  Returns samples (n_samples, ns, d_out)."""
    eng, family, mu_v, Sigma_v, d_out = _path_engine(meta, q_v, q_theta)
    D = np.asarray(meta.Xu).shape[1]
    X = np.asarray(Xstar, dtype=np.float64).reshape(-1, D)
    n_samples, L = int(n_samples), int(features)
    factor = _noise_factor(meta, q_w, d_out, "sample_paths") if noise else None
    omega, phase = path_features(family, D, L, rng)
    feat_w = rng.standard_normal((L, d_out, n_samples))
    eps_v = rng.standard_normal((mu_v.size, n_samples))
    smp = eng.sample_path(X, omega, phase, feat_w, eps_v, mu_v, Sigma_v).transpose(2, 0, 1).copy()
    if noise:
        smp += rng.standard_normal(smp.shape) @ factor.T
    return smp


def rollout_gpssm_paths(q_x0, steps, n_paths, rng, *, q_v, q_w, q_theta, meta, features=1024, noise=True):
    """Roll the GP-SSM transition forward along sampled dynamics: n_paths functions f^(j) are drawn ONCE (pathwise samples of the
    posterior over the transition, d_out must equal D), x_0^(j) ~ q_x0 (one Gaussian), and x_{k+1}^(j) = f^(j)(x_k^(j)) (+ mean(q_W)^-1
    noise with noise=True) -- the same function at every step, which `forecast_gpssm`'s moment matching cannot express.  Each step is
    ONE `SGPDevice.sample_path` call that evaluates all paths at the n_paths current states; path j takes its own state's value (the
    diagonal).  Everything random comes from `rng`.  Returns the trajectories (steps + 1, n_paths, D)."""
    from .cubature import gaussian_inputs
    eng, family, mu_v, Sigma_v, d_out = _path_engine(meta, q_v, q_theta)
    D = np.asarray(meta.Xu).shape[1]
    if d_out != D:
        raise ValueError(f"rollout_gpssm_paths: the transition maps D = {D} inputs to d_out = {d_out} outputs; a rollout needs d_out = D")
    steps, n_paths, L = int(steps), int(n_paths), int(features)
    factor = _noise_factor(meta, q_w, d_out, "rollout_gpssm_paths") if noise else None
    m0, S0 = gaussian_inputs([q_x0], D)
    m0, S0 = np.asarray(m0, dtype=np.float64).reshape(D), np.asarray(S0, dtype=np.float64).reshape(D, D)
    omega, phase = path_features(family, D, L, rng)
    feat_w = rng.standard_normal((L, d_out, n_paths))
    eps_v = rng.standard_normal((mu_v.size, n_paths))
    traj = np.empty((steps + 1, n_paths, D))
    traj[0] = m0 + rng.standard_normal((n_paths, D)) @ np.linalg.cholesky(S0).T if np.any(S0) else np.broadcast_to(m0, (n_paths, D))
    own = np.arange(n_paths)
    for k in range(steps):
        f = eng.sample_path(traj[k], omega, phase, feat_w, eps_v, mu_v, Sigma_v)         # (state, output, path)
        traj[k + 1] = f[own, :, own]
        if noise:
            traj[k + 1] += rng.standard_normal((n_paths, D)) @ factor.T
    return traj


def linearize_step(mean, jac, var, S):
    """One linearised (EKF-style) step through the GP for B Gaussians N(m_b, S_b): `predict_grad`'s mean (B, d_out), jac
    (B, d_out, D) and var (B, d_out, d_out) at the m_b give (mean, Jac S Jac' + var), every covariance exactly symmetric."""
    jac = np.asarray(jac, dtype=np.float64)
    P = np.einsum("bid,bde,bje->bij", jac, np.asarray(S, dtype=np.float64), jac)
    return np.asarray(mean, dtype=np.float64), 0.5 * (P + P.transpose(0, 2, 1)) + np.asarray(var, dtype=np.float64)


def forecast_gpssm(q_x, steps, q_v, q_w, q_theta, meta, noise=True, method="exact"):
    """Roll the GP-SSM transition x_{k+1} ~ MultiSGP(x_k, v, W, theta) forward from q_x -- one Gaussian, or a list of B of them (a
    batch of trajectories) -- in closed form (SE kernel only; d_out must equal D).  Each step is ONE `SGPDevice.psi_predict` call over
    the B current Gaussians: Gaussian in, moment-matched Gaussian out, x_{k+1} ~ N(mean, C_f + mean(q_W)^-1) (noise=False leaves the
    process noise out: the latent f alone).  No cubature points are formed.  q(v) is installed through `set_posterior` on the
    auxiliary engine once.  Returns (means (steps, B, D), covariances (steps, B, D, D)).
    method="linearize" propagates through the Jacobian of the posterior mean instead (EKF-style), for the SE, Matern-3/2 and
    Matern-5/2 kernels: each step is ONE `SGPDevice.predict_grad` call over the B current means, m' = mean(m),
    S' = Jac S Jac' + C_f(m) (+ mean(q_W)^-1 with noise=True), with the explicit q(v)."""
    from . import multisgp as MS
    from .cubature import gaussian_inputs, require_se
    from .device import potrf
    from .meta import kernel_family, set_engine_kernel
    if method not in ("exact", "linearize"):
        raise ValueError(f"forecast_gpssm: method must be 'exact' or 'linearize', not {method!r}")
    if method == "exact":
        require_se(kernel_family(meta.kernel))
    q0 = list(q_x) if isinstance(q_x, (list, tuple)) else [q_x]
    D = np.asarray(meta.Xu).shape[1]
    W = MS._mean_W(q_w)
    if W.shape[0] != D:
        raise ValueError(f"forecast_gpssm: the transition maps D = {D} inputs to d_out = {W.shape[0]} outputs; a rollout needs d_out = D")
    steps = int(steps)
    m, S = gaussian_inputs(q0, D)
    means, covs = np.empty((steps, len(q0), D)), np.empty((steps, len(q0), D, D))
    if not q0 or steps < 1:
        return means, covs
    eng = MS._aux_engine_out(meta, D)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    eng.set_noise(W)
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    if method == "linearize":
        Sigma_v = np.asarray(Sigma_v, dtype=np.float64)
        for k in range(steps):
            mean, jac, var, _, _ = eng.predict_grad(m, mu_v, Sigma_v, noise=noise, var=True, var_grad=False)
            m, S = linearize_step(mean, jac, var, S)
            means[k], covs[k] = m, S
        return means, covs
    eng.set_posterior(mu_v, potrf(np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v), meta.device).T)
    for k in range(steps):
        m, S, _ = eng.psi_predict(m, S, noise=noise)
        S = np.asarray(S, dtype=np.float64).reshape(len(q0), D, D)
        means[k], covs[k] = m, S
    return means, covs
