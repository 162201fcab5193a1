"""Host-side mirror of the `UniSGP` factor node (GPnode/UniSGPnode.jl): same rule names, argument meaning and
error behaviour, batched on the device.

The reference's rules run once per data point and the N-fold Gaussian product folds N rank-1 M x M messages
(GPnode/UniSGPnode.jl:62-73,144-173).  Here the per-point `:v` rule returns an O(1) token and the product runs
ONE device sweep when the N-th token is folded -- the same `counter == N` hook the reference uses to refresh
`meta.Uv` (:64-71).  The PointMass-input rules (`q_in::PointMass`) are the hot path; the uncertain-input variants run on
the device as cubature-weighted data: `:v` (:125-140) and `:out` (:85-93) inside the sweep, the per-node clamped `:w` /
average-energy variants (:177-192,290-313,390-409), the `:in` closure (:107-122) and the `:theta` closures (:242-287)
as stand-alone per-point evaluations at whatever q_v / meta.Uv the caller passes.

What runs where: Gram matrices, Psi-statistics, the factorisations, q(v), `meta.Uv`, the :w / energy sums and the
per-point quadratic forms come from `meta.engine` (`SGPDevice`, the C ABI); without the HIP library and a gfx950 GPU the
first sweep raises -- there is no CPU fallback.  What stays on the host is message bookkeeping: the token counter,
cubature points and weights of an uncertain input (cubature.py), scalar arithmetic on the returned sums (Gamma shape and
rate, the energy's constants), and the conversion of a caller-supplied q_v into the (mean, upper factor) pair the cold
rules upload -- that factor is taken on the device too (`potrf`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .distributions import (GammaShapeRate, MvNormalMeanCovariance, MvNormalMeanPrecision,
                            MvNormalWeightedMeanPrecision, NormalMeanPrecision, NormalMeanVariance, PointMass)
from .cubature import gaussian_inputs, is_exact, require_se
from .meta import UniSGPMeta, kernel_family, set_engine_kernel

LOG2PI = math.log(2.0 * math.pi)


class UniSGP:
    """Node tag: `@node UniSGP Stochastic [out, in, v, w, theta]` (GPnode/UniSGPnode.jl:76-78)."""
    interfaces = ("out", "in", "v", "w", "theta")


@dataclass
class BufferUniSGP:
    """Message wrapper of the `:v` rule (GPnode/UniSGPnode.jl:56-59).  `qv` is an O(1) token here (the index of the
    point in the pending batch), not an M x M message."""
    qv: object
    meta: UniSGPMeta


@dataclass
class PendingMarginal:
    """What the product returns before the N-th message has been folded (the reference returns the partial
    Gaussian product, which nothing consumes before the fold completes)."""
    prior: object
    folded: int


def _is_pointmass(q):
    return isinstance(q, PointMass)


def _mean_w(q_w):
    return float(q_w.mean()) if hasattr(q_w, "mean") else float(q_w)


def _elog_w(q_w):
    if isinstance(q_w, GammaShapeRate):
        return q_w.mean_log()
    w = _mean_w(q_w)
    return math.log(w) if w > 0.0 else float("nan")      # only the average energy uses it


def _engine(meta: UniSGPMeta, n: int):
    """The device object behind a meta; created on first use (raises without the HIP library / a GPU)."""
    M, D = meta.Xu.shape
    eng = meta.engine
    if eng is None or getattr(eng, "n_max", 0) < n:
        from .device import SGPDevice
        if eng is not None:
            eng.close()
        eng = SGPDevice(max(n, meta.N, 1), M, D, 1, device=meta.device, keep_kuf=True, reuse_stats=True)
        meta.engine = eng
        meta._batch.pop("inducing_set", None)
    if not meta._batch.get("inducing_set"):
        eng.set_inducing(meta.Xu)
        meta._batch["inducing_set"] = True
    return eng


def load_batch(eng, X, y, y_var=None, weights=None, n_nodes=None):
    """Put one VMP iteration's batch on a node mirror's engine.  Between the iterations of one `infer` call only the targets
    move (q_out; the inputs do not): when X, the weights and n_nodes equal what is resident on an engine that reuses its
    statistics (`SGPDevice(reuse_stats=True)`), only the targets go over (`set_targets`) and the next sweep keeps K_uf, Psi2
    and the K_uu chain; otherwise -- and always for engines without `reuse_stats` -- `set_data`."""
    res = getattr(eng, "_resident_inputs", None)
    if (getattr(eng, "reuse_stats", False) and res is not None and res[2] == n_nodes and np.array_equal(res[0], X)
            and (res[1] is None) == (weights is None) and (weights is None or np.array_equal(res[1], weights))):
        eng.set_targets(y, y_var)
        return
    eng._resident_inputs = None
    eng.set_data(X, y, y_var, weights, n_nodes=n_nodes)
    eng._resident_inputs = (np.array(X, dtype=np.float64), None if weights is None else np.array(weights, dtype=np.float64),
                            n_nodes)


# ------------------------------------------------------------------------------------------------
# :v  (GPnode/UniSGPnode.jl:144-158 regression, :161-173 classification)
# ------------------------------------------------------------------------------------------------
def rule_v(q_out, q_in, q_w, q_theta, meta: UniSGPMeta) -> BufferUniSGP:
    if not _is_pointmass(q_theta):
        raise TypeError("q_theta must be a PointMass")
    mu_y = float(q_out.mean())
    v_y = 0.0 if _is_pointmass(q_out) else float(q_out.var())
    if not _is_pointmass(q_in):
        # uncertain input (GPnode/UniSGPnode.jl:125-140): the Psi-statistics are cubature sums, i.e. the same
        # statistics over the cubature points with their weights; the rule also adds 1e-8 I to every Psi2 (:135)
        if meta.method is None:
            raise ValueError("UniSGP(:v) with an uncertain input needs meta.method (a cubature rule)")
        if is_exact(meta.method):
            # closed-form statistics: the node keeps its Gaussian, `prod` hands all of them to SGPDevice.sweep_local_psi
            require_se(kernel_family(meta.kernel))
            x = gaussian_inputs([q_in], meta.Xu.shape[1])
        else:
            pts, wts = meta.method.points_weights(q_in.mean(), q_in.var())
            x = (np.asarray(pts, dtype=np.float64), np.asarray(wts, dtype=np.float64))
        meta._batch["uncertain"] = True
    else:
        x = np.atleast_1d(np.asarray(q_in.mean(), dtype=np.float64))
        if meta._pending and meta._batch.get("uncertain"):
            raise NotImplementedError("PointMass and uncertain inputs mixed in one graph")
    w = _mean_w(q_w)
    theta = np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64))
    if meta._pending and (meta._batch.get("w") != w or not np.array_equal(meta._batch.get("theta"), theta)):
        raise ValueError("all UniSGP nodes of one graph share q_w and q_theta")
    if not meta._pending:
        meta._batch.update(w=w, theta=theta, E_logw=_elog_w(q_w), classification=False,
                           uncertain=not _is_pointmass(q_in))
    if not _is_pointmass(q_out):
        meta._batch["classification"] = True
    meta._pending.append((x, mu_y, v_y))
    return BufferUniSGP(len(meta._pending) - 1, meta)


# ------------------------------------------------------------------------------------------------
# prod(GenericProd, left::Normal, right::BufferUniSGP)   (GPnode/UniSGPnode.jl:62-73)
# ------------------------------------------------------------------------------------------------
def prod(left, right: BufferUniSGP):
    meta = right.meta
    if isinstance(left, PendingMarginal):
        prior = left.prior
    else:
        prior = left
    meta.counter += 1
    if meta.counter == 1:
        meta._prior = prior
    if meta.counter < meta.N:
        return PendingMarginal(meta._prior, meta.counter)
    if len(meta._pending) != meta.N:
        raise RuntimeError(f"meta.N = {meta.N} but {len(meta._pending)} UniSGP(:v) messages were produced; meta.N must "
                           "equal the number of UniSGP nodes in the graph (experiments/regression_kin40k.ipynb:155)")
    # ---- the N-th message: one device sweep for the whole batch
    uncertain = bool(meta._batch.get("uncertain"))
    extra_precision = 0.0
    exact = uncertain and is_exact(meta.method)
    if exact:
        X = np.concatenate([p[0][0] for p in meta._pending])               # the means (N, D) ...
        covs = np.concatenate([p[0][1] for p in meta._pending])            # ... and covariances (N, D, D)
        y = np.array([p[1] for p in meta._pending])
        vy = wts = None
        extra_precision = 1e-8 * meta._batch["w"] * meta.N
    elif uncertain:
        X = np.concatenate([p[0][0] for p in meta._pending])
        wts = np.concatenate([p[0][1] for p in meta._pending])
        y = np.concatenate([np.full(len(p[0][1]), p[1]) for p in meta._pending])
        vy = None
        extra_precision = 1e-8 * meta._batch["w"] * meta.N             # N messages, each with Psi2 + 1e-8 I (:135,138)
    else:
        X = np.stack([p[0] for p in meta._pending])
        y = np.array([p[1] for p in meta._pending])
        vy = np.array([p[2] for p in meta._pending]) if meta._batch["classification"] else None
        wts = None
    eng = _engine(meta, len(y))
    sigma2, ell = meta.kernel(meta._batch["theta"])
    if not exact:
        load_batch(eng, X, y, vy, wts, n_nodes=meta.N)
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    eng.set_noise([[meta._batch["w"]]], meta._batch["E_logw"])
    prior = meta._prior
    if extra_precision:
        from .device import potri
        if isinstance(prior, MvNormalMeanCovariance):
            L0 = potri(prior.S, meta.device)
            prior = MvNormalWeightedMeanPrecision(L0 @ prior.m, L0)
        elif isinstance(prior, MvNormalMeanPrecision):
            prior = MvNormalWeightedMeanPrecision(prior.W @ prior.m, prior.W)
        prior = MvNormalWeightedMeanPrecision(prior.xi, prior.W + extra_precision * np.eye(len(prior.xi)))
    if isinstance(prior, MvNormalMeanCovariance):
        eng.set_prior_meancov(prior.m, prior.S)
    elif isinstance(prior, MvNormalWeightedMeanPrecision):
        eng.set_prior_precision(prior.xi, prior.W)
    elif isinstance(prior, MvNormalMeanPrecision):
        eng.set_prior_precision(prior.W @ prior.m, prior.W)
    else:
        raise TypeError(f"unsupported prior type {type(prior).__name__}")
    if exact:
        eng.sweep_local_psi(X, covs, y)
        eng.sweep_finish()
    else:
        eng.sweep()
    mu_v, Sigma_v, Uv = eng.posterior()            # raises PosDefException like cholesky() in the reference
    meta.Uv = Uv                                   # :69
    meta.KuuL = eng.kuu_chol()
    meta.counter = 0                               # :70
    index = {} if uncertain else {x.tobytes(): i for i, x in enumerate(X)}
    meta._batch.update(X=X, y=y, vy=vy, index=index, I=None, mu_v=mu_v)
    meta._pending = []
    return MvNormalMeanCovariance(mu_v, Sigma_v)


def _aux_engine(meta: UniSGPMeta, n: int):
    """A second device object for stand-alone rule evaluations (it replaces data and posterior, so it must not be the
    engine that holds the last swept batch)."""
    M, D = meta.Xu.shape
    eng = meta._batch.get("aux_engine")
    if eng is None or eng.n_max < n:
        from .device import SGPDevice
        if eng is not None:
            eng.close()
        eng = SGPDevice(max(n, 64), M, D, 1, device=meta.device, keep_kuf=True)
        eng.set_inducing(meta.Xu)
        meta._batch["aux_engine"] = eng
    return eng


def _stats_at(meta: UniSGPMeta, theta, X, y, vy, mu_v, Uv):
    """Per-point (I1_n, I2_n) of GPnode/UniSGPnode.jl:196-238 for arbitrary points, at kernel(theta) and at the q(v) given by
    (mu_v, Uv = chol(Sigma_v + mu mu').U): K_uu chain and K_uf on the device, then the per-point quadratic forms."""
    X = np.asarray(X, dtype=np.float64).reshape(len(y), -1)
    eng = _aux_engine(meta, len(y))
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(theta, dtype=np.float64)))
    eng.set_data(X, y, vy)
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    eng.sweep_local()
    eng.set_posterior(mu_v, Uv)
    return eng.w_stats()


def _uv_of(q_v, meta: UniSGPMeta):
    """chol(Sigma_v + mu mu').U of an explicit q_v, factored on the device."""
    from .device import potrf
    mu, Sig = q_v.mean_cov()
    mu = np.asarray(mu, dtype=np.float64)
    return potrf(np.asarray(Sig, dtype=np.float64) + np.outer(mu, mu), meta.device).T


def _node_I(q_out, q_in, mu_v, Uv, theta, meta: UniSGPMeta, jitter_psi2: float, clamp: bool):
    """(I1, I2) of ONE node whose input is uncertain: Psi-statistics by meta.method's cubature, Psi2 + jitter_psi2 I, clamped
    like the reference (GPnode/UniSGPnode.jl:186-190)."""
    if meta.method is None:
        raise ValueError("an uncertain input needs meta.method (a cubature rule)")
    if is_exact(meta.method):
        raise NotImplementedError("ExactSE covers UniSGP's uncertain-input :v / :out pair; the per-node :w rule and energy need a "
                                  "cubature rule (the summed forms, rule_w_summed, read the sweep's scalars and work with either)")
    pts, wts = meta.method.points_weights(q_in.mean(), q_in.var())
    wts = np.asarray(wts, dtype=np.float64)
    mu_y = float(q_out.mean())
    v_y = 0.0 if _is_pointmass(q_out) else float(q_out.var())
    I1q, I2q = _stats_at(meta, theta, pts, np.full(len(wts), mu_y), None, mu_v, Uv)
    I1 = float(wts @ I1q)
    I2 = float(wts @ I2q) + mu_y * mu_y * (1.0 - float(wts.sum())) + v_y
    if jitter_psi2:
        from .device import potri
        KuuL = np.asarray(meta.KuuL, dtype=np.float64)
        I1 -= jitter_psi2 * float(np.trace(potri(KuuL @ KuuL.T, meta.device)))     # tr(Kuu^-1 (jitter I))
        I2 += jitter_psi2 * float(np.sum(np.asarray(Uv) ** 2))                      # tr(Uv'Uv (jitter I))
    if clamp:
        I1, I2 = min(max(I1, 1e-12), 1e12), min(max(I2, 1e-12), 1e12)
    return I1, I2


def _point_stats(q_out, q_in, q_v, q_theta, meta: UniSGPMeta):
    """(I1_n, I2_n) of one PointMass-input node: from the per-point pass over the last swept batch when the point and q_v
    belong to it, else evaluated stand-alone at (q_v, meta.Uv) like the reference's rule would."""
    x = np.atleast_1d(np.asarray(q_in.mean(), dtype=np.float64))
    mu_v = np.asarray(q_v.mean(), dtype=np.float64)
    b = meta._batch
    if "index" in b and x.tobytes() in b["index"] and np.allclose(mu_v, b["mu_v"], rtol=1e-12, atol=0):
        if b["I"] is None:
            b["I"] = meta.engine.w_stats()
        i = b["index"][x.tobytes()]
        return float(b["I"][0][i]), float(b["I"][1][i])
    v_y = None if _is_pointmass(q_out) else np.array([float(q_out.var())])
    I1, I2 = _stats_at(meta, q_theta.mean(), x[None, :], np.array([float(q_out.mean())]), v_y, mu_v, meta.Uv)
    return float(I1[0]), float(I2[0])


# ------------------------------------------------------------------------------------------------
# :w  (GPnode/UniSGPnode.jl:196-216 regression, :219-238 classification, :177-192 uncertain input)
# ------------------------------------------------------------------------------------------------
def rule_w(q_out, q_in, q_v, q_theta, meta: UniSGPMeta) -> GammaShapeRate:
    if _is_pointmass(q_in):
        I1, I2 = _point_stats(q_out, q_in, q_v, q_theta, meta)
    else:
        I1, I2 = _node_I(q_out, q_in, np.asarray(q_v.mean(), dtype=np.float64), meta.Uv, q_theta.mean(), meta, 1e-8, True)
    return GammaShapeRate(1.5, 0.5 * (I1 + I2))


def rule_w_summed(meta: UniSGPMeta, prior: GammaShapeRate) -> GammaShapeRate:
    """q(w) = prior x all N messages, from the sweep's reduced statistics (no per-point pass):
    shape a0 + N/2, rate b0 + (sum I1 + sum I2)/2."""
    sc = meta.engine.scalars()
    return GammaShapeRate(prior.a + 0.5 * meta.N, prior.b + 0.5 * (sc.sum_I1 + sc.sum_I2))


# ------------------------------------------------------------------------------------------------
# :out  (GPnode/UniSGPnode.jl:96-104)
# ------------------------------------------------------------------------------------------------
def rule_out(q_in, q_v, q_w, q_theta, meta: UniSGPMeta) -> NormalMeanPrecision:
    if not _is_pointmass(q_in) and is_exact(meta.method):
        return NormalMeanPrecision(float(_exact_out_means([q_in], q_v, q_theta, meta)[0, 0]), _mean_w(q_w))
    if not _is_pointmass(q_in):
        # GPnode/UniSGPnode.jl:85-93: Psi1 = sum_s omega_s K(Xu, x_s), mean = Psi1 . mu_v
        pts, wts = meta.method.points_weights(q_in.mean(), q_in.var())
        f = predict(np.asarray(pts, dtype=np.float64), q_v, q_theta, meta)
        return NormalMeanPrecision(float(np.dot(wts, f)), _mean_w(q_w))
    m = predict(np.atleast_2d(np.asarray(q_in.mean(), dtype=np.float64)), q_v, q_theta, meta)[0]
    return NormalMeanPrecision(float(m), _mean_w(q_w))


def _exact_out_means(q_ins, q_v, q_theta, meta: UniSGPMeta):
    """Psi1_t . mu_v of every input in closed form (SGPDevice.psi_stats), (T, 1); a PointMass input has S = 0."""
    require_se(kernel_family(meta.kernel))
    eng = _engine(meta, 1)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    means, covs = gaussian_inputs(q_ins, meta.Xu.shape[1])
    return eng.psi_stats(means, covs, None, np.asarray(q_v.mean(), dtype=np.float64), want_psi1=False, want_psi2=False,
                         want_out=True)[2]


def _rule_out_batch(q_ins, q_v, q_theta, meta, *, points_weights_of, engine_of, make_message):
    """What `unisgp.rule_out_batch` and `multisgp.rule_out_batch` share: the points and weights of every input
    (points_weights_of(q_in) -> (points, weights)) go to `SGPDevice.out_message` of engine_of() in one call, at the kernel of
    q_theta and the explicit mean(q_v); node t gets make_message(mean_t), mean_t the d_out node sums."""
    q_ins = list(q_ins)
    if not q_ins:
        return []
    pw = [points_weights_of(q_in) for q_in in q_ins]
    X = np.concatenate([np.asarray(p, dtype=np.float64).reshape(len(w), -1) for p, w in pw])
    wts = np.concatenate([np.asarray(w, dtype=np.float64) for _, w in pw])
    start = np.concatenate([[0], np.cumsum([len(w) for _, w in pw])]).astype(np.int64)
    eng = engine_of()
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    mean = eng.out_message(X, start, wts, np.asarray(q_v.mean(), dtype=np.float64))
    return [make_message(mean[t]) for t in range(len(q_ins))]


def rule_out_batch(q_ins, q_v, q_w, q_theta, meta: UniSGPMeta):
    """`rule_out(q_ins[t], q_v, q_w, q_theta, meta)` for every t in ONE device call (`SGPDevice.out_message`): a PointMass input
    is one point of weight 1, a Gaussian one meta.method's cubature points (GPnode/UniSGPnode.jl:85-93).  Returns a list of
    NormalMeanPrecision(mean_t, mean(q_w)); the values are those of the `rule_out` loop up to the order of the node sums."""
    w_bar = _mean_w(q_w)
    if is_exact(meta.method):
        q_ins = list(q_ins)
        mean = _exact_out_means(q_ins, q_v, q_theta, meta) if q_ins else []
        return [NormalMeanPrecision(float(mean[t, 0]), w_bar) for t in range(len(q_ins))]
    return _rule_out_batch(
        q_ins, q_v, q_theta, meta,
        points_weights_of=lambda q_in: ((q_in.mean(), np.ones(1)) if _is_pointmass(q_in)
                                        else meta.method.points_weights(q_in.mean(), q_in.var())),
        engine_of=lambda: _engine(meta, 1),
        make_message=lambda mean: NormalMeanPrecision(float(mean[0]), w_bar))


def predict(Xstar, q_v, q_theta, meta: UniSGPMeta) -> np.ndarray:
    """Batched `@call_rule UniSGP(:out)` (the 30 000-call loop of experiments/regression_kin40k.ipynb:288-304)."""
    Xstar = np.asarray(Xstar, dtype=np.float64)
    if Xstar.ndim == 1:
        Xstar = Xstar[:, None]
    eng = _engine(meta, 1)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    return eng.predict(Xstar, np.asarray(q_v.mean(), dtype=np.float64))


def _test_points(x, method, D: int):
    """(points (S, D), cubature weights or None) of an array of test inputs, a PointMass, or an uncertain input q(x*) (by
    meta.method's cubature, as `rule_out` takes them)."""
    if _is_pointmass(x):
        return np.atleast_1d(np.asarray(x.mean(), dtype=np.float64)).reshape(1, D), None
    if not isinstance(x, (np.ndarray, list, tuple, float, int)) and hasattr(x, "mean"):
        if method is None:
            raise ValueError("an uncertain test input needs meta.method (a cubature rule)")
        m, P = x.mean_cov() if hasattr(x, "mean_cov") else (x.mean(), x.var())
        pts, wts = method.points_weights(m, P)
        return np.asarray(pts, dtype=np.float64).reshape(-1, D), np.asarray(wts, dtype=np.float64)
    X = np.asarray(x, dtype=np.float64)
    return X.reshape(-1, D), None


def combine_total_variance(wts, m, var):
    """Law of total variance over cubature points s: mean = sum w_s m_s, var = sum w_s (var_s + m_s^2) - mean^2.  Scalar
    outputs: m, var (S,); matrix outputs: m (S, d), var (S, d, d) -> (d,), (d, d) with m_s m_s' in place of m_s^2."""
    wts, m, var = np.asarray(wts, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(var, dtype=np.float64)
    mean = wts @ m
    if m.ndim == 1:
        return float(mean), float(wts @ (var + m * m) - mean * mean)
    second = np.einsum("s,sij->ij", wts, var + m[:, :, None] * m[:, None, :])
    return mean, second - np.outer(mean, mean)


def joint_points(Xstar, psi: str, D: int, what: str = "joint"):
    """The test inputs of predictive(..., joint=True) or (..., grad=True): a plain (ns, D) array (a PointMass gives its point) --
    joint covariances and derivatives at Gaussian inputs are not covered (their per-point counterpart is psi="exact")."""
    if psi != "cubature":
        raise ValueError(f"predictive: {what}=True takes point inputs (ns, D) only (psi must be 'cubature')")
    if what == "grad" and type(Xstar).__name__ == "PointMass":
        Xstar = Xstar.mean()
    try:
        return np.asarray(Xstar, dtype=np.float64).reshape(-1, D)
    except (TypeError, ValueError):
        raise ValueError(f"predictive: {what}=True takes point inputs (ns, D) only") from None


def predictive(Xstar_or_q_in, q_v, q_w, q_theta, meta: UniSGPMeta, noise: bool = True, psi: str = "cubature", joint: bool = False,
               grad: bool = False):
    """Predictive mean and variance of the latent f (noise=False) or of the observation y (noise=True: + 1 / mean(q_w)) at
    kernel(q_theta) and the explicit q_v (`q_v.mean_cov()` goes to the device, sgp_predict_var).  Test inputs (ns, D) give
    per-point arrays (ns,), (ns,); a PointMass or an uncertain input q(x*) gives two floats -- the latter by one device call over
    meta.method's cubature points and the law of total variance on the host.  `rule_out` is unchanged (the reference's
    message carries precision mean(q_w) only).  psi="exact" (SE kernel only) takes a Gaussian, a PointMass, a plain array or a
    list of inputs through ONE closed-form `SGPDevice.psi_predict` call on the auxiliary engine instead -- no cubature points; a
    list gives per-input arrays (T,), (T,).  joint=True (point inputs (ns, D) only) returns the mean (ns,) and the JOINT (ns, ns)
    covariance over all test points instead (`SGPDevice.predict_joint`; the noise enters its diagonal).  grad=True (point inputs
    or a PointMass) returns (mean (ns,), var (ns,), dmean (ns, D), dvar (ns, D)): the prediction with its derivatives with respect to
    the test input (`SGPDevice.predict_grad`; SE, Matern-3/2 and Matern-5/2)."""
    D = meta.Xu.shape[1]
    if psi not in ("cubature", "exact"):
        raise ValueError(f"predictive: psi must be 'cubature' or 'exact', got {psi!r}")
    if joint and grad:
        raise ValueError("predictive: pass joint=True or grad=True, not both")
    if grad:
        X = joint_points(Xstar_or_q_in, psi, D, "grad")
        eng = _engine(meta, 1)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise([[_mean_w(q_w)]], _elog_w(q_w))
        mu_v, Sigma_v = q_v.mean_cov()
        m, jac, var, vg, _ = eng.predict_grad(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
        return m[:, 0].copy(), var[:, 0, 0].copy(), jac[:, 0, :].copy(), vg[:, 0, 0, :].copy()
    if joint:
        X = joint_points(Xstar_or_q_in, psi, D)
        eng = _engine(meta, 1)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise([[_mean_w(q_w)]], _elog_w(q_w))
        mu_v, Sigma_v = q_v.mean_cov()
        return eng.predict_joint(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
    if psi == "exact":
        from .multisgp import exact_predictive
        require_se(kernel_family(meta.kernel))
        eng = _aux_engine(meta, 1)
        sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
        set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
        if noise:
            eng.set_noise([[_mean_w(q_w)]], _elog_w(q_w))
        m, v, single = exact_predictive(eng, Xstar_or_q_in, q_v, D, noise, meta.device)
        return (float(m[0, 0]), float(v[0])) if single else (m[:, 0].copy(), v)
    X, wts = _test_points(Xstar_or_q_in, meta.method, D)
    eng = _engine(meta, 1)
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    if noise:
        eng.set_noise([[_mean_w(q_w)]], _elog_w(q_w))
    mu_v, Sigma_v = q_v.mean_cov()
    m, v = eng.predict_var(X, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64), noise=noise)
    if wts is not None:
        return combine_total_variance(wts, m, v)
    if _is_pointmass(Xstar_or_q_in):
        return float(m[0]), float(v[0])
    return m, v


def probit_predictive(Xstar_or_q_in, q_v, q_w, q_theta, meta: UniSGPMeta):
    """P(y = 1) of the classification model (`f ~ UniSGP(x, v, w, theta); y ~ Probit(f)`, experiments/classification_banana.ipynb):
    Phi(m / sqrt(1 + var_f + 1 / mean(q_w))), with (m, var_f + 1 / mean(q_w)) from `predictive(..., noise=True)`."""
    from scipy.special import ndtr
    m, v = predictive(Xstar_or_q_in, q_v, q_w, q_theta, meta, noise=True)
    p = ndtr(np.asarray(m, dtype=np.float64) / np.sqrt(1.0 + np.asarray(v, dtype=np.float64)))
    return float(p) if np.ndim(p) == 0 else p


# ------------------------------------------------------------------------------------------------
# @average_energy  (GPnode/UniSGPnode.jl:337-359 Gamma w; :363-387 classification; :411-436 PointMass w)
# ------------------------------------------------------------------------------------------------
def average_energy(q_out, q_in, q_v, q_w, q_theta, meta: UniSGPMeta) -> float:
    if _is_pointmass(q_in):
        I1, I2 = _point_stats(q_out, q_in, q_v, q_theta, meta)
    elif isinstance(q_w, GammaShapeRate):
        # :290-313 -- meta.KuuL / meta.Uv, Psi2 + 1e-8 I, clamped
        I1, I2 = _node_I(q_out, q_in, np.asarray(q_v.mean(), dtype=np.float64), meta.Uv, q_theta.mean(), meta, 1e-8, True)
    else:
        # :390-409 (q_w::PointMass) -- Sigma_v + mu mu' from q_v itself.  The reference also adds 1e-8 to EVERY ENTRY of
        # Kuu, Psi1 and Psi2 there (`.+ 1e-8`); that quirk moves the result by < 1e-6 (GPtest.jl:337-348 tests it against
        # the clean formula at 1e-6) and is not reproduced.
        I1, I2 = _node_I(q_out, q_in, np.asarray(q_v.mean(), dtype=np.float64), _uv_of(q_v, meta), q_theta.mean(), meta, 0.0, True)
    w_bar = _mean_w(q_w)
    return 0.5 * (I1 * w_bar - _elog_w(q_w) + LOG2PI + I2 * w_bar)


def average_energy_summed(meta: UniSGPMeta) -> float:
    """Sum over the N nodes, from the sweep's scalars (w and E[log w] as given to the sweep)."""
    return meta.engine.scalars().energy


# ------------------------------------------------------------------------------------------------
# :in and :theta return log-density closures (ContinuousUnivariateLogPdf / ContinuousMultivariateLogPdf in ReactiveMP);
# here a callable whose every evaluation is one batched device pass
# ------------------------------------------------------------------------------------------------
class LogPdfClosure:
    def __init__(self, fn, multivariate: bool = False):
        self.fn = fn
        self.multivariate = multivariate

    def logpdf(self, x):
        return self.fn(x)

    __call__ = logpdf


def rule_in(q_out, q_v, q_w, q_theta, meta: UniSGPMeta) -> LogPdfClosure:
    """GPnode/UniSGPnode.jl:107-122: x -> -w/2 A(x) + w mu_y B(x).mu_v - w/2 |Uv B(x)|^2 with A(x) = k(x,x) - |KuuL^-1 B(x)|^2
    = -w/2 (I1(x) + I2(x) - mu_y^2).  Accepts a scalar or an array of inputs (one device pass for all of them)."""
    w_bar, mu_y = _mean_w(q_w), float(q_out.mean())
    mu_v = np.asarray(q_v.mean(), dtype=np.float64)
    theta, Uv = q_theta.mean(), meta.Uv

    def log_backwardmess(x):
        xs = np.atleast_1d(np.asarray(x, dtype=np.float64))
        X = xs.reshape(-1, meta.Xu.shape[1])
        I1, I2 = _stats_at(meta, theta, X, np.full(len(X), mu_y), None, mu_v, Uv)
        val = -0.5 * w_bar * (I1 + I2 - mu_y * mu_y)
        return float(val[0]) if np.ndim(x) == 0 or (meta.Xu.shape[1] > 1 and np.ndim(x) == 1) else val
    return LogPdfClosure(log_backwardmess)


def rule_theta(q_out, q_in, q_v, q_w, meta: UniSGPMeta) -> LogPdfClosure:
    """GPnode/UniSGPnode.jl:242-287: theta -> w mu_y Psi1(theta).mu_v - w/2 (Psi0(theta) + tr(Psi2(theta) (Rv - Kuu^-1(theta))))
    = -w/2 (sum_q omega_q (I1_q + I2_q) - mu_y^2 sum_q omega_q), Rv from q_v itself.  The batch-summed version of this is
    the hyper-parameter objective `SGPDevice.theta_objective` (helper_functions/derivative_helper.jl:23-39)."""
    if not _is_pointmass(q_in) and meta.method is None:
        raise ValueError("UniSGP(:theta) with an uncertain input needs meta.method (a cubature rule)")
    w_bar, mu_y = _mean_w(q_w), float(q_out.mean())
    mu_v = np.asarray(q_v.mean(), dtype=np.float64)
    Uv = _uv_of(q_v, meta)
    if _is_pointmass(q_in):
        pts, wts = np.atleast_1d(np.asarray(q_in.mean(), dtype=np.float64))[None, :], np.ones(1)
    else:
        pts, wts = meta.method.points_weights(q_in.mean(), q_in.var())
    wts = np.asarray(wts, dtype=np.float64)

    def log_backwardmess(theta):
        I1, I2 = _stats_at(meta, theta, pts, np.full(len(wts), mu_y), None, mu_v, Uv)
        return float(-0.5 * w_bar * (wts @ (I1 + I2) - mu_y * mu_y * wts.sum()))
    return LogPdfClosure(log_backwardmess, multivariate=True)


def prod_logpdf(left, right):
    """ReactiveMP.prod(GenericProd, Gaussian, ContinuousUnivariateLogPdf) and its mirror image (GPnode/UniSGPnode.jl:39-54):
    moments of N(x) exp(logpdf(x)) by ghcubature(21); `v + 1e-6` only when the Gaussian is on the left; NaN moments return
    the Gaussian unchanged."""
    from .cubature import ghcubature
    gauss, closure, pad = (left, right, 1e-6) if isinstance(right, LogPdfClosure) else (right, left, 0.0)
    pts, wts = ghcubature(21).points_weights(gauss.mean(), gauss.var())
    g = np.exp(np.asarray(closure.logpdf(pts[:, 0]), dtype=np.float64))
    Z = float(wts @ g)
    m = float(wts @ (pts[:, 0] * g)) / Z if Z != 0.0 else float("nan")
    v = float(wts @ ((pts[:, 0] - m) ** 2 * g)) / Z if Z != 0.0 else float("nan")
    if math.isnan(m) or math.isnan(v):
        return gauss
    return NormalMeanVariance(m, v + pad)


# ------------------------------------------------------------------------------------------------
# batched :in messages and their moment-matched marginals (sgp_in_message)
# ------------------------------------------------------------------------------------------------
def reference_moments_are_nan(logpdf) -> bool:
    """Whether the reference's products (GPnode/UniSGPnode.jl:39-54, GPnode/MultiSGPnode.jl:37-44) return their Gaussian
    argument for a node with these closure values: they exponentiate unshifted, so the moments are NaN when some exp overflows
    (logpdf > log(DBL_MAX): Inf / Inf) or every exp underflows (0 / 0)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(np.asarray(logpdf, dtype=np.float64))
    return bool(np.any(np.isinf(e)) or np.any(np.isnan(e)) or not np.any(e > 0.0))


def shifted_moments(pts, wts, logpdf):
    """(log_norm, mean, cov) of the weighted points under exp(logpdf), shifted by the largest logpdf among the points of
    positive weight (what sgp_in_message computes on the device): g = w exp(logpdf - a), mean = sum g x / sum g, cov about that
    mean; a point of weight 0 takes no part."""
    pts = np.asarray(pts, dtype=np.float64).reshape(len(wts), -1)
    lp = np.asarray(logpdf, dtype=np.float64)
    w = np.asarray(wts, dtype=np.float64)
    a = float(lp[w > 0].max()) if np.any(w > 0) else float(lp.max())
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(w > 0, w * np.exp(lp - a), 0.0)
    Z = float(g.sum())
    mean = (g @ pts) / Z
    d = pts - mean
    return a + math.log(Z), mean, (d * g[:, None]).T @ d / Z


def _marginal_in_batch(q_outs, lefts, q_v, q_theta, meta, reference_fallback, *, points_weights_of, y_of, engine_of, set_noise,
                       make_marginal):
    """What `unisgp.marginal_in_batch` and `multisgp.marginal_in_batch` share: the cubature points of every left message
    (points_weights_of(left) -> (points, weights)) and the rows y_of(q_out) go to `SGPDevice.in_message` of engine_of() in one
    call, at the kernel of q_theta, the noise set_noise(engine) installs and the explicit q_v; node t gets
    make_marginal(mean_t, cov_t), or its left message back under the reference's NaN fallback."""
    q_outs, lefts = list(q_outs), list(lefts)
    if len(q_outs) != len(lefts):
        raise ValueError("marginal_in_batch: one left message per node")
    if not lefts:
        return []
    pw = [points_weights_of(left) for left in lefts]
    X = np.concatenate([np.asarray(p, dtype=np.float64).reshape(len(w), -1) for p, w in pw])
    wts = np.concatenate([np.asarray(w, dtype=np.float64) for _, w in pw])
    start = np.concatenate([[0], np.cumsum([len(w) for _, w in pw])]).astype(np.int64)
    y = np.stack([np.asarray(y_of(q), dtype=np.float64).ravel() for q in q_outs])
    eng = engine_of()
    sigma2, ell = meta.kernel(np.atleast_1d(np.asarray(q_theta.mean(), dtype=np.float64)))
    set_engine_kernel(eng, sigma2, ell, meta.jitter, kernel_family(meta.kernel))
    set_noise(eng)
    mu_v, Sigma_v = q_v.mean_cov()
    lp, _, mean, cov = eng.in_message(X, start, y, wts, np.asarray(mu_v, dtype=np.float64), np.asarray(Sigma_v, dtype=np.float64))
    return [left if reference_fallback and reference_moments_are_nan(lp[start[t]:start[t + 1]]) else make_marginal(mean[t], cov[t])
            for t, left in enumerate(lefts)]


def marginal_in_batch(q_outs, lefts, q_v, q_w, q_theta, meta: UniSGPMeta, reference_fallback: bool = True):
    """q(x_t) of T UniSGP nodes in ONE device call: `prod_logpdf(lefts[t], rule_in(q_outs[t], ...))` for every t
    (GPnode/UniSGPnode.jl:39-46 over :107-122).  The ghcubature(21) points of every left message go to `SGPDevice.in_message`
    with the explicit q_v; the device returns the closure values and the shifted moments, and `v + 1e-6` is added as
    `prod_logpdf` adds it for a Gaussian on the left.  reference_fallback (default): a node whose unshifted moments are NaN
    in the reference (`reference_moments_are_nan`, decided from the returned closure values) gets its left message back;
    False returns the shifted moments there too.  Returns a list of NormalMeanVariance (or left messages)."""
    from .cubature import ghcubature
    if meta.Xu.shape[1] != 1:
        raise ValueError("unisgp.marginal_in_batch: the Gauss-Hermite product needs a one-dimensional input")
    rule = ghcubature(21)
    return _marginal_in_batch(
        q_outs, lefts, q_v, q_theta, meta, reference_fallback,
        points_weights_of=lambda left: rule.points_weights(left.mean(), left.var()),
        y_of=lambda q: [float(q.mean())],
        engine_of=lambda: _engine(meta, 1),
        set_noise=lambda eng: eng.set_noise([[_mean_w(q_w)]], _elog_w(q_w)),
        make_marginal=lambda mean, cov: NormalMeanVariance(float(np.ravel(mean)[0]), float(np.ravel(cov)[0]) + 1e-6))
