"""Host-side mirror of the `MultiSGP` factor node (GPnode/MultiSGPnode.jl): D_out outputs sharing one kernel, uncertain
(Gaussian) inputs handled by cubature, Wishart-distributed noise precision.

The reference evaluates, per time step, cubature Psi-statistics (5 Gram columns + 5 rank-1 M x M updates), a
`kron(W, Psi2)` message and a DM x DM Gaussian product.  Here the cubature points of ALL steps go to the device as weighted
data in one call; the summed statistics give q(v), the Wishart inverse scale and the average energy in one sweep
(eq. M).  Per-step rule functions are provided for interface parity (they run the same device
kernels on one step).

What runs where: Gram matrices, Psi-statistics, every factorisation / inverse, q(v), the Wishart inverse scale, the energy
and the per-point quadratic forms come from `meta.engine` and the device building blocks (C ABI); there is no CPU
fallback for them.  What stays in NumPy is bookkeeping of a few d_out x d_out or M x M operands that are arguments of
those calls, not results of the node's algebra: cubature points and weights of q_in (cubature.py), `slogdet` of the
d_out x d_out mean(q_w) when q_w has no `mean_logdet` (:83), the block contraction S = sum_ij W_ij Rv[i][j] and
s = sum_d mu_v^(d) (mu_y' W)_d of `_second_moment_contraction`, a trace, and the Laplace step of `rule_in` (L-BFGS and a
finite-difference Hessian in d_in dimensions around the device-evaluated closure; the reference uses ForwardDiff).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from .distributions import (MvNormalMeanCovariance, MvNormalMeanPrecision, MvNormalWeightedMeanPrecision, PointMass,
                            WishartFast)
from .cubature import gaussian_inputs, is_exact, require_se
from .meta import MultiSGPMeta, kernel_family, set_engine_kernel
from .unisgp import load_batch


class MultiSGP:
    """Node tag: `@node MultiSGP Stochastic [out, in, v, w, theta]` (GPnode/MultiSGPnode.jl:47-49)."""
    interfaces = ("out", "in", "v", "w", "theta")


def _mean_W(q_w):
    W = q_w.mean() if hasattr(q_w, "mean") else q_w
    return np.atleast_2d(np.asarray(W, dtype=np.float64))


def _cov_of(q):
    return None if isinstance(q, PointMass) else np.atleast_2d(np.asarray(q.cov(), dtype=np.float64))


def _engine(meta: MultiSGPMeta, n_points: int, d_out: int):
    Xu = np.asarray(meta.Xu, dtype=np.float64)
    M, D = Xu.shape
    eng = meta.engine
    if eng is None or eng.n_max < n_points or eng.d_out != d_out:
        from .device import SGPDevice
        if eng is not None:
            eng.close()
        eng = SGPDevice(max(n_points, 1), M, D, d_out, device=meta.device, reuse_stats=True)
        eng.set_inducing(Xu)
        meta.engine = eng
    return eng


def _expand(meta: MultiSGPMeta, q_ins: Sequence, q_outs: Sequence):
    """All steps' cubature points as weighted data (approximate_kernel_expectation!, GPnode/MultiSGPnode.jl:11-35)."""
    pts, wts, ys, cov_sum = [], [], [], None
    for q_in, q_out in zip(q_ins, q_outs):
        if isinstance(q_in, PointMass):
            p, w = np.atleast_2d(np.asarray(q_in.mean(), dtype=np.float64)), np.ones(1)
        else:
            m, P = q_in.mean_cov()
            p, w = meta.method.points_weights(m, P)
        y = np.asarray(q_out.mean(), dtype=np.float64).ravel()
        pts.append(p)
        wts.append(w)
        ys.append(np.repeat(y[None, :], len(w), axis=0))
        c = _cov_of(q_out)
        if c is not None:
            cov_sum = c.copy() if cov_sum is None else cov_sum + c
    return np.concatenate(pts), np.concatenate(wts), np.concatenate(ys), cov_sum


def load(meta: MultiSGPMeta, q_outs: Sequence, q_ins: Sequence, q_w, q_theta: PointMass, prior, E_logdet_W=None):
    """What `sweep` puts on the engine in front of its sweep: the steps' cubature points as weighted data with the output
    covariance sum (not with exact Psi-statistics, whose local phase takes the inputs itself), the kernel, the noise and the
    prior.  Returns the engine."""
    W = _mean_W(q_w)
    d_out = W.shape[0]
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    if is_exact(meta.method):
        # the statistics in closed form (SGPDevice.sweep_local_psi): the setters first, the local phase reads them
        require_se(kernel_family(meta.kernel))
        eng = _engine(meta, 1, d_out)
    else:
        pts, wts, ys, cov_sum = _expand(meta, q_ins, q_outs)
        eng = _engine(meta, len(wts), d_out)
        load_batch(eng, pts, ys, None, wts, n_nodes=len(q_ins))
        if cov_sum is not None:
            eng.set_output_cov_sum(cov_sum)
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    if E_logdet_W is None:
        E_logdet_W = q_w.mean_logdet() if hasattr(q_w, "mean_logdet") else float(np.linalg.slogdet(W)[1])
    eng.set_noise(W, E_logdet_W)
    if isinstance(prior, MvNormalMeanCovariance):
        eng.set_prior_meancov(prior.m, prior.S)
    elif isinstance(prior, MvNormalWeightedMeanPrecision):
        eng.set_prior_precision(prior.xi, prior.W)
    elif isinstance(prior, MvNormalMeanPrecision):
        eng.set_prior_precision(prior.W @ prior.m, prior.W)
    else:
        raise TypeError(f"unsupported prior type {type(prior).__name__}")
    return eng


def sweep(meta: MultiSGPMeta, q_outs: Sequence, q_ins: Sequence, q_w, q_theta: PointMass, prior, E_logdet_W=None):
    """One VMP update of q(v) from all steps' `:v` messages (GPnode/MultiSGPnode.jl:290-328) folded with the prior.
    Returns the marginal MvNormalMeanCovariance; the Wishart statistics and the energy are then available through
    `rule_w_summed` / `average_energy_summed`."""
    eng = load(meta, q_outs, q_ins, q_w, q_theta, prior, E_logdet_W)
    if is_exact(meta.method):
        means, covs = gaussian_inputs(q_ins, np.asarray(meta.Xu).shape[1])
        Y = np.stack([np.asarray(q.mean(), dtype=np.float64).ravel() for q in q_outs])
        eng.sweep_local_psi(means, covs, Y)
        out_covs = [c for c in map(_cov_of, q_outs) if c is not None]
        if out_covs:
            eng.set_output_cov_sum(sum(out_covs))
        eng.sweep_finish()
    else:
        eng.sweep()
    mu, Sigma, _ = eng.posterior(want_uv=False)
    return MvNormalMeanCovariance(mu, Sigma)


def _exact_out_means(q_ins, q_v, q_theta, meta, eng):
    """Psi1_t' mu_v^(d) of every input in closed form (SGPDevice.psi_stats), (T, d_out)."""
    require_se(kernel_family(meta.kernel))
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    means, covs = gaussian_inputs(q_ins, np.asarray(meta.Xu).shape[1])
    return eng.psi_stats(means, covs, None, np.asarray(q_v.mean(), dtype=np.float64), want_psi1=False, want_psi2=False,
                         want_out=True)[2]


def rule_w_summed(meta: MultiSGPMeta, prior_nu: float, prior_invscale, n_nodes: int) -> WishartFast:
    """q(W) = prior x all `:w` messages WishartFast(D + 2, I1_t + I2_t) (GPnode/MultiSGPnode.jl:367-444):
    inverse scales add, degrees of freedom nu0 + N."""
    S = meta.engine.wishart_invscale()
    return WishartFast(prior_nu + n_nodes, np.asarray(prior_invscale, dtype=np.float64) + S)


def average_energy_summed(meta: MultiSGPMeta) -> float:
    """Sum over the steps of @average_energy MultiSGP (GPnode/MultiSGPnode.jl:544-632)."""
    return meta.engine.scalars().energy


def rule_out(q_in, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta) -> MvNormalMeanPrecision:
    """@rule MultiSGP(:out) (GPnode/MultiSGPnode.jl:90-120): mean_d = Psi1 . mu_v^(d), precision mean(q_w)."""
    W = _mean_W(q_w)
    d_out = W.shape[0]
    if is_exact(meta.method):
        return MvNormalMeanPrecision(_exact_out_means([q_in], q_v, q_theta, meta, _engine(meta, 1, d_out))[0], W)
    if isinstance(q_in, PointMass):
        p, w = np.atleast_2d(np.asarray(q_in.mean(), dtype=np.float64)), np.ones(1)
    else:
        p, w = meta.method.points_weights(*q_in.mean_cov())
    eng = _engine(meta, len(w), d_out)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    f = np.atleast_2d(eng.predict(p, np.asarray(q_v.mean(), dtype=np.float64)))      # (S, d_out)
    if f.shape[0] != len(w):
        f = f.T
    return MvNormalMeanPrecision(w @ f, W)


def rule_out_batch(q_ins, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta):
    """`rule_out(q_ins[t], q_v, q_w, q_theta, meta)` for every t in ONE device call (GPnode/MultiSGPnode.jl:90-120): the forward
    messages a GP-SSM needs from all its time steps in every VMP iteration.  A PointMass input is one point of weight 1, a
    Gaussian one meta.method's cubature points; all of them go to `SGPDevice.out_message` with the explicit mean(q_v), and the
    device returns the node sums Psi1' mu_v^(d).  Returns a list of MvNormalMeanPrecision(mean_t, mean(q_w)).  The values are
    those of the `rule_out` loop up to the order of the node sums (the device's lanes and tree against the host's dot product)."""
    from .unisgp import _rule_out_batch
    W = _mean_W(q_w)
    if is_exact(meta.method):
        q_ins = list(q_ins)
        if not q_ins:
            return []
        mean = _exact_out_means(q_ins, q_v, q_theta, meta, _engine(meta, 1, W.shape[0]))
        return [MvNormalMeanPrecision(mean[t].copy(), W) for t in range(len(q_ins))]
    return _rule_out_batch(
        q_ins, q_v, q_theta, meta,
        points_weights_of=lambda q_in: ((q_in.mean(), np.ones(1)) if isinstance(q_in, PointMass)
                                        else meta.method.points_weights(*q_in.mean_cov())),
        engine_of=lambda: _engine(meta, 1, W.shape[0]),
        make_message=lambda mean: MvNormalMeanPrecision(mean.copy(), W))


def exact_predict_inputs(x, D: int):
    """The inputs of `predictive(psi="exact")` as (means (T, D), covs (T, D, D) or None, single): a Gaussian or PointMass is one
    node (single: the caller returns one mean and covariance), a plain array its rows with S = 0, a list one node per entry."""
    def is_dist(q):
        return not isinstance(q, (np.ndarray, list, tuple, float, int)) and hasattr(q, "mean")
    if is_dist(x):
        means, covs = gaussian_inputs([x], D)
        return means, covs, True
    if isinstance(x, (list, tuple)) and len(x) and all(is_dist(q) for q in x):
        means, covs = gaussian_inputs(list(x), D)
        return means, covs, False
    return np.asarray(x, dtype=np.float64).reshape(-1, D), None, False


def exact_predictive(eng, x, q_v, D: int, noise: bool, device: int):
    """ONE `SGPDevice.psi_predict` call over the inputs of `exact_predict_inputs` with the explicit q_v installed through
    `set_posterior`, as `marginal_in_exact_batch` installs it; kernel and noise are already the engine's.  Returns (mean (T, d_out),
    cov as the device returns it, single)."""
    from .device import potrf
    means, covs, single = exact_predict_inputs(x, D)
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    Uv = potrf(np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v), device).T
    eng.set_posterior(mu_v, Uv)
    m, C, _ = eng.psi_predict(means, covs, noise=noise)
    return m, C, single


def predictive(Xstar_or_q_in, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, noise: bool = True, psi: str = "cubature",
               joint: bool = False, grad: bool = False):
    """Predictive means and covariances of the d_out latent outputs (noise=False) or of the observation (noise=True: +
    mean(q_w)^-1) at kernel(q_theta) and the explicit q_v (sgp_predict_var).  Test inputs (ns, D) give means (ns, d_out) and
    covariances (ns, d_out, d_out); a PointMass or an uncertain input q(x*) gives one mean (d_out,) and covariance (d_out,
    d_out) -- the latter by one device call over meta.method's cubature points and the law of total variance in matrix form.
    psi="exact" (SE kernel only) takes a Gaussian, a PointMass, a plain array or a list of inputs through ONE closed-form
    `SGPDevice.psi_predict` call instead -- no cubature points; a list gives stacked means (T, d_out) and covariances.
    joint=True (point inputs (ns, D) only) returns the means (ns, d_out) and the JOINT (ns d_out, ns d_out) covariance over all
    test points instead (`SGPDevice.predict_joint`: row i ns + s is output i at point s).  grad=True (point inputs or a PointMass)
    returns (means (ns, d_out), covariances (ns, d_out, d_out), Jacobians (ns, d_out, D), covariance gradients (ns, d_out, d_out, D)):
    the prediction with its derivatives with respect to the test input (`SGPDevice.predict_grad`; SE, Matern-3/2, Matern-5/2)."""
    from .unisgp import _test_points, combine_total_variance, joint_points
    _check_psi(psi, "predictive")
    W = _mean_W(q_w)
    d_out = W.shape[0]
    D = np.asarray(meta.Xu).shape[1]
    if joint and grad:
        raise ValueError("predictive: pass joint=True or grad=True, not both")
    if grad:
        X = joint_points(Xstar_or_q_in, psi, D, "grad")
        eng = _engine(meta, 1, d_out)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise(W)
        mu_v, Sigma_v = q_v.mean_cov()
        m, jac, var, vg, _ = eng.predict_grad(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
        return m, var, jac, vg
    if joint:
        X = joint_points(Xstar_or_q_in, psi, D)
        eng = _engine(meta, 1, d_out)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise(W)
        mu_v, Sigma_v = q_v.mean_cov()
        m, C = eng.predict_joint(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
        return np.asarray(m, dtype=np.float64).reshape(-1, d_out), C
    if psi == "exact":
        require_se(kernel_family(meta.kernel))
        eng = _aux_engine_out(meta, d_out)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise(W)
        m, C, single = exact_predictive(eng, Xstar_or_q_in, q_v, D, noise, meta.device)
        C = np.asarray(C, dtype=np.float64).reshape(-1, d_out, d_out)
        return (m[0], C[0]) if single else (m, C)
    X, wts = _test_points(Xstar_or_q_in, meta.method, D)
    eng = _engine(meta, 1, d_out)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    if noise:
        eng.set_noise(W)
    mu_v, Sigma_v = q_v.mean_cov()
    m, C = eng.predict_var(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
    m, C = np.asarray(m, dtype=np.float64).reshape(-1, d_out), np.asarray(C, dtype=np.float64).reshape(-1, d_out, d_out)
    if wts is not None:
        return combine_total_variance(wts, m, C)
    if isinstance(Xstar_or_q_in, PointMass):
        return m[0], C[0]
    return m, C


def rule_v(q_out, q_in, q_w, q_theta: PointMass, meta: MultiSGPMeta) -> MvNormalWeightedMeanPrecision:
    """@rule MultiSGP(:v) for ONE step (GPnode/MultiSGPnode.jl:290-328): the message itself, xi = vcat(Psi1 (mu_y' W)_d),
    Lambda = kron(W, Psi2), with Psi1 / Psi2 from the device statistics of that step."""
    W = _mean_W(q_w)
    d_out = W.shape[0]
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    if is_exact(meta.method):
        require_se(kernel_family(meta.kernel))
        eng = _engine(meta, 1, d_out)
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        psi1, Psi2, _ = eng.psi_stats(*gaussian_inputs([q_in], np.asarray(meta.Xu).shape[1]))
        Psi1 = psi1[0]
    else:
        pts, wts, ys, _ = _expand(meta, [q_in], [q_out])
        eng = _engine(meta, len(wts), d_out)
        load_batch(eng, pts, np.ones((len(wts), d_out)), None, wts, n_nodes=1)
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        eng.sweep_local()
        Psi2, B, _ = eng.stats()
        Psi1 = B[:, 0]
    row = np.asarray(q_out.mean(), dtype=np.float64).ravel() @ W                      # :307
    xi = np.concatenate([Psi1 * row[d] for d in range(d_out)])
    return MvNormalWeightedMeanPrecision(xi, np.kron(W, Psi2))                         # :306


def _aux_engine(meta: MultiSGPMeta, n: int):
    """A single-output device object for stand-alone closure evaluations (it replaces data and posterior, so it is not the
    engine that holds the last swept sequence)."""
    Xu = np.asarray(meta.Xu, dtype=np.float64)
    M, D = Xu.shape
    eng = getattr(meta, "_aux_engine", None)
    if eng is None or eng.n_max < n:
        from .device import SGPDevice
        if eng is not None:
            eng.close()
        eng = SGPDevice(max(n, 64), M, D, 1, device=meta.device, keep_kuf=True)
        eng.set_inducing(Xu)
        meta._aux_engine = eng
    return eng


def _aux_engine_out(meta: MultiSGPMeta, d_out: int):
    """A d_out-output device object without data for the closed-form prediction: `set_posterior` replaces its q(v), so it is not
    the engine that holds the last swept sequence."""
    Xu = np.asarray(meta.Xu, dtype=np.float64)
    M, D = Xu.shape
    eng = getattr(meta, "_aux_engine_out", None)
    if eng is None or eng.d_out != d_out:
        from .device import SGPDevice
        if eng is not None:
            eng.close()
        eng = SGPDevice(1, M, D, d_out, device=meta.device)
        eng.set_inducing(Xu)
        meta._aux_engine_out = eng
    return eng


def rule_in(q_out, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, q_in=None):
    """@rule MultiSGP(:in) (GPnode/MultiSGPnode.jl:162-184 Gaussian output, :186-208 point-mass output): the log-pdf closure
        x -> -1/2 tr(W) I1(x) + s . k(x) - 1/2 k(x)' S k(x),      I1(x) = k(x,x) - k' Kuu^-1 k,
        s = sum_d mu_v^(d) (mu_y' W)_d  (sum_diagonal_M),   S = sum_ij W_ij Rv_blk[i][j]  (create_blockmatrix), Rv = Sigma_v + mu mu'.
    Both quadratic forms are per-point quantities the device already produces: with the pseudo-posterior (mean s, factor
    chol(S).U) and pseudo-observations y = 1, sgp_w_stats returns I1(x) and I2(x) = 1 - 2 s.k + k' S k, so the closure is
    -1/2 tr(W) I1 - 1/2 (I2 - 1) -- one device pass for any number of inputs (K_uu chain, K_uf, the two quadratic forms).
    K_uu^-1 is the device's own at (theta, meta.jitter); the reference reads the copy stored in its meta (:168), made the same way.
    With `q_in` given and point-mass q_out / q_w (:210-236) the closure is fitted by a Gaussian at its mode (Laplace): see
    `rule_in_laplace`."""
    if q_in is not None:
        return rule_in_laplace(q_out, q_in, q_v, q_w, q_theta, meta)
    from .unisgp import LogPdfClosure
    from .device import potrf
    Xu = np.asarray(meta.Xu, dtype=np.float64)
    M, D_in = Xu.shape
    W = _mean_W(q_w)
    s_vec, S = _second_moment_contraction(q_out, q_v, W, M)                             # :176-179
    US = potrf(S, meta.device).T                                                        # upper factor: |US k|^2 = k' S k
    trW = float(np.trace(W))
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))

    def log_backwardmess(x):
        X = np.asarray(x, dtype=np.float64).reshape(-1, D_in)
        eng = _aux_engine(meta, len(X))
        eng.set_data(X, np.ones(len(X)), None)
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        eng.sweep_local()
        eng.set_posterior(s_vec, US)
        I1, I2 = eng.w_stats()
        val = -0.5 * trW * I1 - 0.5 * (I2 - 1.0)                                        # :181
        return float(val[0]) if np.ndim(x) == 1 else val
    closure = LogPdfClosure(log_backwardmess, multivariate=True)
    closure.in_node = (q_out, q_v, q_w, q_theta, meta)          # what `prod_logpdf` hands to the batched device path
    return closure


def marginal_in_batch(q_outs, lefts, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, reference_fallback: bool = True):
    """q(x_t) of T MultiSGP nodes in ONE device call: `prod_logpdf(lefts[t], rule_in(q_outs[t], q_v, q_w, q_theta, meta))` for
    every t (GPnode/MultiSGPnode.jl:37-44 over :162-208) -- the loop a GP-SSM runs over its time steps in every VMP iteration.
    The srcubature points of every left message go to `SGPDevice.in_message` with the explicit q_v and mean(q_w); the device
    returns the closure values and, per node, the moments of N(x) exp(logpdf(x)) shifted by the node's largest closure value.
    reference_fallback (default): a node whose unshifted moments are NaN in the reference (`reference_moments_are_nan`,
    decided on the host from the returned closure values) gets its left message back, as the reference returns it; False
    returns the shifted moments there too.  Returns a list of MvNormalMeanCovariance (or left messages)."""
    from .cubature import srcubature
    from .unisgp import _marginal_in_batch
    rule = srcubature()
    return _marginal_in_batch(
        q_outs, lefts, q_v, q_theta, meta, reference_fallback,
        points_weights_of=lambda left: rule.points_weights(*left.mean_cov()),
        y_of=lambda q: q.mean(),
        engine_of=lambda: _engine(meta, 1, _mean_W(q_w).shape[0]),
        set_noise=lambda eng: eng.set_noise(_mean_W(q_w)),
        make_marginal=lambda mean, cov: MvNormalMeanCovariance(np.array(mean, dtype=np.float64), np.array(cov, dtype=np.float64)))


def prod_logpdf(left, right, reference_fallback: bool = True):
    """ReactiveMP.prod(GenericProd, MultivariateGaussian, ContinuousMultivariateLogPdf) (GPnode/MultiSGPnode.jl:37-44): the
    moments of N(x) exp(logpdf(x)) over srcubature's points; NaN moments return the Gaussian unchanged.  A closure that came
    from `rule_in` is a one-node call of `marginal_in_batch` (the device evaluates the closure and takes the moments); any other
    closure is evaluated point by point and the same shifted moments are taken on the host."""
    node = getattr(right, "in_node", None)
    if node is not None:
        q_out, q_v, q_w, q_theta, meta = node
        return marginal_in_batch([q_out], [left], q_v, q_w, q_theta, meta, reference_fallback)[0]
    from .cubature import srcubature
    from .unisgp import reference_moments_are_nan, shifted_moments
    pts, wts = srcubature().points_weights(*left.mean_cov())
    lp = np.array([float(right.logpdf(p)) for p in pts])
    if reference_fallback and reference_moments_are_nan(lp):
        return left
    _, mean, cov = shifted_moments(pts, wts, lp)
    return MvNormalMeanCovariance(mean, cov)


def rule_in_laplace(q_out, q_in, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, iterations: int = 20):
    """@rule MultiSGP(:in) with q_out::PointMass, q_in Gaussian, q_w::PointMass (GPnode/MultiSGPnode.jl:210-236): minimise the
    negative closure from mean(q_in) with L-BFGS (20 iterations, :229) and return N(m_z, W_z^-1) in weighted-mean form, W_z
    the Hessian at the minimiser (:231-233).  The reference differentiates with ForwardDiff / Zygote; here gradient and
    Hessian are central differences of the device-evaluated closure, every stencil one device pass."""
    from scipy.optimize import minimize
    closure = rule_in(q_out, q_v, q_w, q_theta, meta)
    x0 = np.asarray(q_in.mean(), dtype=np.float64).ravel()
    D_in = len(x0)
    h = 1e-5

    def neg_and_grad(x):
        pts = np.vstack([x] + [x + h * e for e in np.eye(D_in)] + [x - h * e for e in np.eye(D_in)])
        f = -np.asarray(closure.logpdf(pts))
        return float(f[0]), (f[1:1 + D_in] - f[1 + D_in:]) / (2 * h)
    res = minimize(neg_and_grad, x0, jac=True, method="L-BFGS-B", options={"maxiter": iterations})
    m_z = res.x
    hh = 1e-4
    E = np.eye(D_in)
    pts, idx = [m_z], {}
    for a in range(D_in):
        for b in range(a, D_in):
            idx[(a, b)] = len(pts)
            pts += [m_z + hh * (E[a] + E[b]), m_z + hh * (E[a] - E[b]), m_z - hh * (E[a] - E[b]), m_z - hh * (E[a] + E[b])]
    f = -np.asarray(closure.logpdf(np.vstack(pts)))
    W_z = np.zeros((D_in, D_in))
    for (a, b), k in idx.items():
        W_z[a, b] = W_z[b, a] = (f[k] - f[k + 1] - f[k + 2] + f[k + 3]) / (4 * hh * hh)
    return MvNormalWeightedMeanPrecision(W_z @ m_z, W_z)                                # :235


def damped_newton_batch(evaluate, x0, iterations: int = 20, gtol: float = 1e-6):
    """Minimise f_t = -logpdf_t for T independent nodes together.  evaluate(X (T, D)) -> (logpdf (T,), grad (T, D), hess
    (T, D, D)) of logpdf, one point per node (one device call).  From x0, every round steps each unfinished node by
    (H + lambda_t I) delta = -g for f (H = -hess, g = -grad), lambda_t >= 0 raised until the matrix is positive definite; the
    trial point is accepted only if f decreased, otherwise lambda_t grows and the node retries in the next round.  A node is
    finished when |g|_inf <= thr_t = gtol max(1, |g(x0)|_inf).  At most iterations + 1 calls of `evaluate`.  Returns x (T, D), f, g,
    H at the last accepted points, thr (T,), converged (T,), rounds (T,): the calls each node took a step in."""
    x = np.array(x0, dtype=np.float64)
    T, D = x.shape
    lp, gr, he = evaluate(x)
    f, g, H = -np.asarray(lp, dtype=np.float64), -np.asarray(gr, dtype=np.float64), -np.asarray(he, dtype=np.float64)
    thr = gtol * np.maximum(1.0, np.max(np.abs(g), axis=1))
    lam = np.zeros(T)
    rounds = np.zeros(T, dtype=np.int64)
    done = np.max(np.abs(g), axis=1) <= thr
    for _ in range(iterations):
        if done.all():
            break
        trial = x.copy()
        for t in np.flatnonzero(~done):
            w, V = np.linalg.eigh(H[t])
            scale = max(float(np.max(np.abs(w))), 1e-300)
            if w[0] <= 1e-8 * scale:                  # not positive definite: the most negative direction is flipped, w_0 + lambda = |w_0|
                lam[t] = max(lam[t], 2.0 * abs(float(w[0])) + 1e-3 * scale)
            trial[t] = x[t] - V @ ((V.T @ g[t]) / (w + lam[t]))
        lp, gr, he = evaluate(trial)
        for t in np.flatnonzero(~done):
            rounds[t] += 1
            if np.isfinite(lp[t]) and -lp[t] < f[t]:
                x[t], f[t], g[t], H[t] = trial[t], -lp[t], -gr[t], -he[t]
                lam[t] *= 0.25
                done[t] = np.max(np.abs(g[t])) <= thr[t]
            else:
                lam[t] = max(4.0 * lam[t], 1e-3 * max(float(np.max(np.abs(np.diag(H[t])))), 1e-300))
    return x, f, g, H, thr, done, rounds


def rule_in_laplace_batch(q_outs, q_ins, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, iterations: int = 20,
                          gtol: float = 1e-6):
    """The Laplace form of @rule MultiSGP(:in) (GPnode/MultiSGPnode.jl:210-236) for T nodes together: the batched replacement of
    a loop over `rule_in_laplace`.  Every node's negative closure is minimised from mean(q_in) by the damped Newton iteration of
    `damped_newton_batch`, whose every round is ONE `SGPDevice.in_message_grad` call with one point per node (closure value,
    analytic gradient and Hessian; the D x D systems are solved on the host): at most iterations + 1 device calls in all,
    against hundreds of K_uu chains for the finite differences of the per-node form.  Returns (marginals, records):
    marginals[t] = MvNormalWeightedMeanPrecision(W_z m_z, W_z) with W_z the analytic Hessian of the negative closure at m_z,
    records[t] = dict(converged, rounds, grad_inf, threshold, proper, mode = m_z).  A node whose W_z is not positive definite is returned as
    the reference would return it (the improper precision), with proper = False; a node that has not met its threshold after
    `iterations` rounds is returned where it stands, with converged = False."""
    q_outs, q_ins = list(q_outs), list(q_ins)
    if len(q_outs) != len(q_ins):
        raise ValueError("rule_in_laplace_batch: one q_in per node")
    if not q_ins:
        return [], []
    W = _mean_W(q_w)
    D_in = np.asarray(meta.Xu).shape[1]
    x0 = np.stack([np.asarray(q.mean(), dtype=np.float64).ravel() for q in q_ins]).reshape(len(q_ins), D_in)
    y = np.stack([np.asarray(q.mean(), dtype=np.float64).ravel() for q in q_outs])
    eng = _engine(meta, 1, W.shape[0])
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    eng.set_noise(W)
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v, Sigma_v = np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64)
    start = np.arange(len(q_ins) + 1, dtype=np.int64)
    x, _, g, H, thr, done, rounds = damped_newton_batch(lambda X: eng.in_message_grad(X, start, y, mu_v, Sigma_v), x0, iterations, gtol)
    marginals, records = [], []
    for t in range(len(q_ins)):
        try:
            np.linalg.cholesky(H[t])
            proper = True
        except np.linalg.LinAlgError:
            proper = False
        marginals.append(MvNormalWeightedMeanPrecision(H[t] @ x[t], H[t].copy()))        # :235
        records.append(dict(converged=bool(done[t]), rounds=int(rounds[t]), grad_inf=float(np.max(np.abs(g[t]))),
                            threshold=float(thr[t]), proper=proper, mode=x[t].copy()))
    return marginals, records


def natural_gradient_in(evaluate, left_m, left_S, m, S, iterations: int = 1, halvings: int = 8):
    """Natural-gradient steps of T independent Gaussians q_t = N(m_t, S_t) on L_t(q) = KL(q || N(left_m_t, left_S_t)) + U_t(q).
    evaluate(idx, m (n, D), S (n, D, D)) -> (U (n,), gamma = dU/dm (n, D), Gamma = dU/dS (n, D, D)) of the nodes `idx`, one call.
    With Sl = left_S the stationary point has precision Sl^-1 + 2 Gamma and weighted mean Sl^-1 ml + 2 Gamma m - gamma, so from the
    current q the step is (Lambda, xi) <- (1 - rho)(Lambda, xi) + rho (Lambda*, xi*), from rho = 1; rho is halved per node until
    Lambda is positive definite (decided on the host) and L_t has not risen (one `evaluate` of all the nodes still trying per
    round).  A node that has used `halvings` halvings keeps its current q.  Returns (m, S, records) with records = dict(before,
    after (T,): L_t at the start and at the end, rho (T,): the last accepted step length or 0, halved (T,): halvings taken)."""
    m, S = np.array(m, dtype=np.float64), np.array(S, dtype=np.float64)
    left_m, left_S = np.asarray(left_m, dtype=np.float64), np.asarray(left_S, dtype=np.float64)
    T, D = m.shape
    Sl_inv = np.linalg.inv(left_S)
    Sl_inv = 0.5 * (Sl_inv + Sl_inv.transpose(0, 2, 1))
    ld_left = np.linalg.slogdet(left_S)[1]

    def free(idx, mm, SS, U):
        dm = mm - left_m[idx]
        kl = 0.5 * (np.einsum("tab,tba->t", Sl_inv[idx], SS) + np.einsum("ta,tab,tb->t", dm, Sl_inv[idx], dm) - D + ld_left[idx]
                    - np.linalg.slogdet(SS)[1])
        return kl + U

    everyone = np.arange(T)
    U, gam, Gam = (np.array(a, dtype=np.float64) for a in evaluate(everyone, m, S))
    L = free(everyone, m, S, U)
    before = L.copy()
    rho_taken, halved = np.zeros(T), np.zeros(T, dtype=np.int64)
    for _ in range(int(iterations)):
        Lam0 = np.linalg.inv(S)
        xi0 = np.einsum("tab,tb->ta", Lam0, m)
        Lam1 = Sl_inv + 2.0 * Gam
        xi1 = np.einsum("tab,tb->ta", Sl_inv, left_m) + 2.0 * np.einsum("tab,tb->ta", Gam, m) - gam
        rho, used = np.ones(T), np.zeros(T, dtype=np.int64)
        pending = everyone
        while pending.size:
            idx, tm, tS = [], [], []
            for t in pending:
                while used[t] <= halvings:
                    Lam = (1.0 - rho[t]) * Lam0[t] + rho[t] * Lam1[t]
                    Lam = 0.5 * (Lam + Lam.T)
                    try:
                        np.linalg.cholesky(Lam)
                        break
                    except np.linalg.LinAlgError:
                        rho[t] *= 0.5
                        used[t] += 1
                if used[t] > halvings:
                    continue
                St = np.linalg.inv(Lam)
                St = 0.5 * (St + St.T)
                idx.append(t)
                tS.append(St)
                tm.append(St @ ((1.0 - rho[t]) * xi0[t] + rho[t] * xi1[t]))
            if not idx:
                break
            idx, tm, tS = np.array(idx), np.array(tm), np.array(tS)
            U2, g2, G2 = (np.asarray(a, dtype=np.float64) for a in evaluate(idx, tm, tS))
            L2 = free(idx, tm, tS, U2)
            ok = np.isfinite(L2) & (L2 <= L[idx])
            acc = idx[ok]
            m[acc], S[acc], U[acc], gam[acc], Gam[acc], L[acc] = tm[ok], tS[ok], U2[ok], g2[ok], G2[ok], L2[ok]
            rho_taken[acc] = rho[acc]
            pending = idx[~ok]
            rho[pending] *= 0.5
            used[pending] += 1
        halved += np.minimum(used, halvings)
    return m, S, dict(before=before, after=L, rho=rho_taken, halved=halved)


def marginal_in_exact_batch(q_outs, lefts, q_ins, q_v, q_w, q_theta: PointMass, meta: MultiSGPMeta, iterations: int = 1,
                            halvings: int = 8):
    """q(x_t) of T MultiSGP nodes on the closed-form objective (SE kernel only): from q_ins[t] = N(m, S), `iterations`
    natural-gradient steps (`natural_gradient_in`) on L_t(q) = KL(q || lefts[t]) + U_t(q), U_t the part of the node's average energy
    that depends on its input -- the expectation under q of what `marginal_in_batch` evaluates at cubature points, with the targets
    mean(q_outs[t]).  Every evaluation round is ONE `SGPDevice.psi_in_grad` call over the nodes still trying.  q(v) is installed
    with `set_posterior` and W = mean(q_w) with `set_noise`, as `load_theta_objective_multi(psi="exact")` installs them.  L_t does
    not rise at any node; simultaneous updates of all nodes do not make the global free energy monotone.  Returns (marginals
    [MvNormalMeanCovariance], records of `natural_gradient_in`)."""
    from .device import potrf
    q_outs, lefts, q_ins = list(q_outs), list(lefts), list(q_ins)
    if not (len(q_outs) == len(lefts) == len(q_ins)):
        raise ValueError("marginal_in_exact_batch: one q_out, one left message and one q_in per node")
    require_se(kernel_family(meta.kernel))
    if not q_ins:
        return [], dict(before=np.zeros(0), after=np.zeros(0), rho=np.zeros(0), halved=np.zeros(0, dtype=np.int64))
    W = _mean_W(q_w)
    M, D_in = np.asarray(meta.Xu).shape
    y = np.stack([np.asarray(q.mean(), dtype=np.float64).ravel() for q in q_outs])
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    Uv = potrf(np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v), meta.device).T
    eng = _engine(meta, len(q_ins), W.shape[0])
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    eng.set_noise(W, float(np.linalg.slogdet(W)[1]))
    eng.set_posterior(mu_v, Uv)
    m0, S0 = gaussian_inputs(q_ins, D_in)
    lm, lS = gaussian_inputs(lefts, D_in)
    m, S, rec = natural_gradient_in(lambda idx, mm, SS: eng.psi_in_grad(mm, SS, y[idx]), lm, lS, m0, S0, iterations, halvings)
    return [MvNormalMeanCovariance(m[t].copy(), S[t].copy()) for t in range(len(q_ins))], rec


def _second_moment_contraction(q_out, q_v, W, M):
    """s = sum_d mu_v^(d) (mu_y' W)_d and S = sum_ij W_ij Rv_blk[i][j] -- what the :in and :theta closures keep of q(v)."""
    mu_y = np.asarray(q_out.mean(), dtype=np.float64).ravel()
    d_out = len(mu_y)
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    Rv = np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v)
    row = mu_y @ W
    s_vec = sum(mu_v[d * M:(d + 1) * M] * row[d] for d in range(d_out))
    S = sum(Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] * W[i, j] for i in range(d_out) for j in range(d_out))
    return s_vec, 0.5 * (S + S.T)


def rule_theta(q_out, q_in, q_v, q_w, meta: MultiSGPMeta):
    """@rule MultiSGP(:theta) (GPnode/MultiSGPnode.jl:447-466): theta -> -1/2 tr(W) (Psi0 - tr(Kuu^-1 Psi2')) + Psi1 . s
    - 1/2 tr(Psi2' S), Psi2' = Psi2 + 1e-7 I (:458), Kuu(theta) without jitter (:455), Psi by meta.method's cubature over q_in.
    Per cubature point this is the :in closure, so one device pass per theta (K_uu chain at theta, K_uf for the points, the
    two per-point quadratic forms); the 1e-7 I term adds 1e-7 (tr(W) tr(Kuu^-1) - tr(S)) / 2, with Kuu^-1 from the device
    (sgp_kernelmatrix + sgp_potri); the host only takes its trace."""
    from .unisgp import LogPdfClosure
    from .device import kernelmatrix, potri, potrf
    if meta.method is None:
        raise ValueError("MultiSGP(:theta) needs meta.method (a cubature rule)")
    Xu = np.asarray(meta.Xu, dtype=np.float64)
    M = Xu.shape[0]
    W = _mean_W(q_w)
    s_vec, S = _second_moment_contraction(q_out, q_v, W, M)
    US = potrf(S, meta.device).T
    trW, trS = float(np.trace(W)), float(np.trace(S))
    m_in, P_in = q_in.mean_cov()
    pts, wts = meta.method.points_weights(m_in, P_in)
    pts, wts = np.atleast_2d(np.asarray(pts, dtype=np.float64)), np.asarray(wts, dtype=np.float64)

    def log_backwardmess(theta):
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(theta, dtype=np.float64)))
        eng = _aux_engine(meta, len(pts))
        eng.set_data(pts, np.ones(len(pts)), None)
        set_engine_kernel(eng, sigma2, ell, 0.0, kernel_family(meta.kernel))
        eng.sweep_local()
        eng.set_posterior(s_vec, US)
        I1, I2 = eng.w_stats()
        Kuu = kernelmatrix(Xu, Xu, sigma2, ell, meta.device, family=kernel_family(meta.kernel))
        tr_kinv = float(np.trace(potri(Kuu, meta.device)))
        return float(wts @ (-0.5 * trW * I1 - 0.5 * (I2 - 1.0)) + 0.5e-7 * (trW * tr_kinv - trS))
    return LogPdfClosure(log_backwardmess, multivariate=True)


# ------------------------------------------------------------------------------------------------
# the hyper-parameter objective: neg_log_backwardmess_multi / grad_llh_multi! (helper_functions/derivative_helper.jl:92-115)
# ------------------------------------------------------------------------------------------------
def _check_psi(psi, what):
    if psi not in ("cubature", "exact"):
        raise ValueError(f"{what}: psi must be 'cubature' or 'exact', got {psi!r}")


def load_theta_objective_multi(y_data, q_ins: Sequence, q_v, q_w, meta: MultiSGPMeta, psi: str = "cubature"):
    """Load the inputs of neg_log_backwardmess_multi on `meta.engine` -- what `theta_objective_multi` evaluates and
    `train.optimize_theta_multi(device_paced=True)` descends on -- and return (engine, D_in).

    psi="exact": the objective over the closed-form Psi-statistics of the Gaussian inputs (SE kernel only; SGPDevice.
    theta_objective_psi / theta_descend_psi).  No points are formed or loaded: only W and q(v) are installed as below; the inputs
    those calls take come from `exact_theta_inputs`.

    The points are meta.method's cubature points of every q_in (a PointMass input is its own point), each node's target
    y_data[i] repeated over its points (the reference passes y_data = mean.(qx)); W = mean(q_w); q(v) is installed with
    `set_posterior` (mu_v and chol(Sigma_v + mu mu').U, factored on the device), so the device forms S = sum_ij W_ij Rv[i][j]
    and the linear term itself.  The kernel family is meta.kernel's; the kernel values are the caller's to set."""
    from .device import potrf
    _check_psi(psi, "theta_objective_multi")
    W = _mean_W(q_w)
    d_out = W.shape[0]
    if d_out < 2:
        raise ValueError("theta_objective_multi: MultiSGP needs d_out >= 2 (a d_out x d_out mean(q_w)); use the UniSGP objective")
    q_ins = list(q_ins)
    Y = np.asarray(y_data, dtype=np.float64)
    if Y.ndim == 1 and len(q_ins) == 1:
        Y = Y[None, :]
    if Y.ndim != 2 or Y.shape != (len(q_ins), d_out):
        raise ValueError(f"theta_objective_multi: y_data must be {len(q_ins)} x {d_out} (one target per node), got {Y.shape}")
    M, D_in = np.asarray(meta.Xu).shape
    if psi == "exact":
        from .cubature import require_se
        require_se(kernel_family(meta.kernel))
    elif meta.method is None and not all(isinstance(q, PointMass) for q in q_ins):
        raise ValueError("theta_objective_multi: uncertain inputs need meta.method (a cubature rule)")
    else:
        pts, wts, ys, _ = _expand(meta, q_ins, [PointMass(y) for y in Y])
    mu_v, Sigma_v = q_v.mean_cov()
    mu_v = np.asarray(mu_v, dtype=np.float64).ravel()
    if mu_v.shape != (d_out * M,):
        raise ValueError(f"theta_objective_multi: q_v must have d_out * M = {d_out * M} entries, got {mu_v.size}")
    Uv = potrf(np.asarray(Sigma_v, dtype=np.float64) + np.outer(mu_v, mu_v), meta.device).T
    eng = _engine(meta, len(q_ins) if psi == "exact" else len(wts), d_out)
    if psi != "exact":
        load_batch(eng, pts, ys, None, wts, n_nodes=len(q_ins))
    sign, logdet = np.linalg.slogdet(W)
    eng.set_noise(W, float(logdet))
    eng.set_posterior(mu_v, Uv)
    return eng, D_in


def exact_theta_inputs(y_data, q_ins: Sequence, meta: MultiSGPMeta):
    """(means (T, D), covs (T, D, D), Y (T, d_out)): the Gaussian inputs and targets as SGPDevice.theta_objective_psi and
    theta_descend_psi take them (a PointMass input has S = 0), for an engine loaded by `load_theta_objective_multi(psi="exact")`."""
    from .cubature import gaussian_inputs
    q_ins = list(q_ins)
    means, covs = gaussian_inputs(q_ins, np.asarray(meta.Xu).shape[1])
    return means, covs, np.asarray(y_data, dtype=np.float64).reshape(len(q_ins), -1)


def theta_objective_multi(y_data, q_ins: Sequence, q_v, q_w, meta: MultiSGPMeta, psi: str = "cubature"):
    """Load the objective's inputs on `meta.engine` once (`load_theta_objective_multi`) and return `evaluate(theta) -> (value,
    grad)`, value and gradient of neg_log_backwardmess_multi at the raw theta that `meta.kernel` maps
    (derivative_helper.jl:92-106).

    K_uu^-1 is taken at meta.jitter (the reference adds 1e-12 I).  Each call of `evaluate` is one
    `set_kernel` and one `sgp_theta_objective`: value and analytic gradient w.r.t. (sigma2, ell...), then the chain rule
    through softplus (d softplus / dx = sigmoid) when meta.kernel has softplus_params set.  A kernel callable without
    `softplus_params` is taken to map theta to (theta[0], theta[1:]) unchanged.

    psi="exact": the same objective over the closed-form Psi-statistics of the Gaussian inputs (`load_theta_objective_multi`);
    each call is one `set_kernel` and one `sgp_theta_objective_psi`."""
    eng, D_in = load_theta_objective_multi(y_data, q_ins, q_v, q_w, meta, psi)
    exact = exact_theta_inputs(y_data, q_ins, meta) if psi == "exact" else None
    softplus_params = bool(getattr(meta.kernel, "softplus_params", False))
    family = kernel_family(meta.kernel)

    def evaluate(theta):
        th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
        sigma2, ell = meta.kernel(th)
        ell = np.atleast_1d(np.asarray(ell, dtype=np.float64))
        if th.size != 1 + ell.size or ell.size not in (1, D_in):
            raise ValueError(f"theta_objective_multi: theta must be (sigma2, 1 or {D_in} lengthscales), got {th.size} entries")
        set_engine_kernel(eng, sigma2, ell, meta.jitter, family)
        if exact is not None:                                                       # (psi="exact": sgp_theta_objective_psi)
            value, grad = eng.theta_objective_psi(*exact, want_grad=True)
        else:
            value, grad = eng.theta_objective(want_grad=True, n_ell=ell.size)
        grad = np.asarray(grad, dtype=np.float64)
        if softplus_params:
            grad = grad / (1.0 + np.exp(-th))                                       # d softplus(x) / dx = sigmoid(x)
        return float(value), grad
    return evaluate


def grad_llh_multi(theta, y_data, q_ins: Sequence, q_v, q_w, meta: MultiSGPMeta):
    """grad_llh_multi! (helper_functions/derivative_helper.jl:108-115) on the device: (value, gradient) of
    neg_log_backwardmess_multi at the raw theta of meta.kernel, with y_data (n_nodes x d_out), the inputs q_ins, q(v) and
    mean(q_w) held fixed.  See `theta_objective_multi` for what is loaded; the reference's sumRv_Wbar, tr_W and v are formed
    from q_v and q_w on the device."""
    return theta_objective_multi(y_data, q_ins, q_v, q_w, meta)(theta)
