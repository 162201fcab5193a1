"""Call sequences on one handle (helper, no tests): every state-changing call in front of every reader.

The handle keeps a record of what its device buffers belong to (StatsRecord in csrc/sgp_api.hip, the comment table "Entry point ->
effect").  This module holds what tests/test_gpu_call_sequences.py and tests/test_call_sequences_host.py share:

  PROBLEMS   `uni` and `multi`, the smallest problems that still cross the paths the record governs;
  MUTATORS   name -> Op: one entry per row of the table plus the variants the table distinguishes, each with the kind of the next
             sgp_sweep on a SGP_FLAG_REUSE_STATS handle -- written by hand from the documentation of sgp_sweep_kind in
             include/sgp_hip.h and from the table, never read from the library;
  READERS    name -> Op returning a tuple of arrays, or ("refused", status);
  Shadow     the handle's normal form in plain Python: the setter values in force at the last sweep, what kind of sweep it was, and
             what has changed since.  A fresh handle is brought to it with `build` (public setters, one sweep, the changed setters);
  ENTRY_POINTS   the classification of every exported sgp_* name (the ledger of the host test).

A call that moves theta or X_u on the device enters the model as its host equivalent -- set_kernel(softplus(theta)) and
set_inducing(Xu) + set_posterior(the held q(v)) with the values the call returned -- and flags the history "device-set": the host's
softplus is not the device's to the last bit, so such a history is compared to bounds, not bitwise.
"""
import functools
import math
import re

import numpy as np

FULL, TARGETS, REUSED = 0, 1, 2
JITTER = 1e-6
ERR_ARG = -1


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def invsoftplus(p):
    p = np.asarray(p, dtype=np.float64)
    return p + np.log(-np.expm1(-p))


# ---- the two problems -------------------------------------------------------------------------------------------------------
def _grid_xu(rng, M, D):
    """per-dimension permutations of a grid, as tests/inducing_descend_ref.point_case"""
    return np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)


def _gaussians(rng, T, D, d_out):
    mean = rng.uniform(-1.5, 1.5, (T, D))
    A = 0.15 * rng.normal(size=(T, D, D))
    cov = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(D)
    Yn = np.sin(mean @ rng.normal(size=(D, d_out)) / math.sqrt(D)) + 0.05 * rng.normal(size=(T, d_out))
    return mean, cov, Yn


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs of a problem (arrays not to be written to)."""
    if name == "uni":
        d_out, D, M, N, T = 1, 2, 70, 200, 30            # two tile columns, the second padded; four 64-point blocks, the last ragged
        rng = np.random.default_rng(101)
        X = rng.uniform(-1.7, 1.7, (N, D))
        Y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
        vy = rng.uniform(0.05, 0.3, N)                   # point variances
        wts, n_nodes = None, None
        mean, cov, Yn = _gaussians(rng, T, D, d_out)
    else:
        d_out, D, M, T = 2, 2, 48, 30                    # 30 nodes x 5 weighted points: the same nodes as Gaussians and as points
        rng = np.random.default_rng(102)
        mean, cov, Yn = _gaussians(rng, T, D, d_out)
        L = np.linalg.cholesky(cov)
        # the mean (weight 0.2) and 2 D spherical-radial points scaled so that the weighted points have mean and covariance (mean, cov)
        dirs = math.sqrt(D / 0.8) * np.concatenate([np.eye(D), -np.eye(D)])
        X = np.concatenate([mean[:, None, :], mean[:, None, :] + np.einsum("tij,pj->tpi", L, dirs)], axis=1).reshape(-1, D)
        wts = np.tile(np.concatenate([[0.2], np.full(2 * D, 0.8 / (2 * D))]), T)
        Y = np.repeat(Yn, 5, axis=0)
        N, vy, n_nodes = len(X), None, T
    Xu = _grid_xu(rng, M, D)
    ell1 = np.array([0.4, 0.45]) if name == "uni" else np.array([0.5, 0.6])     # (M = 70 in the same box: shorter, for the conditioning)
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    Xq = rng.uniform(-1.7, 1.7, (37, D))
    qstart = np.array([0, 5, 6, 20, 37])
    P = dict(name=name, d_out=d_out, D=D, M=M, N=N, T=T, X=X, Y=Y, vy=vy, wts=wts, n_nodes=n_nodes, Xu=Xu, W=W, W2=1.7 * W,
             X2=X + 0.01 * rng.normal(size=X.shape), Y2=Y + 0.3 * rng.normal(size=np.shape(Y)),
             Xu2=_grid_xu(rng, M, D), mean=mean, cov=cov, Yn=Yn,
             Xq=Xq, qstart=qstart, Yq=rng.normal(size=(4, d_out)), wq=rng.uniform(0.2, 1.0, 37),
             S_y=np.diag(rng.uniform(1.0, 3.0, d_out)), theta1=(0.9, ell1, JITTER), theta2=(1.1, 0.9 * ell1, JITTER), family="se", family2="matern32", prior=("iso", 50.0), prior2=("iso", 20.0))
    P["S_y2"] = 0.5 * P["S_y"]
    P["raw1"] = invsoftplus(np.concatenate([[P["theta1"][0]], P["theta1"][1]]))
    P["raw2"] = invsoftplus(np.concatenate([[P["theta2"][0]], P["theta2"][1]]))
    return P


PROBLEMS = ("uni", "multi")


def kuu_cond(P, theta, family, Xu=None):
    """cond(K_uu + jitter I) at a kernel of the tables (Xu: the inducing inputs, P["Xu"] by default)"""
    from tests import multi_theta_ref as R
    s2, ell, jit = theta
    return float(np.linalg.cond(R.kernelmatrix(family, s2, np.asarray(ell), P["Xu"] if Xu is None else Xu) + jit * np.eye(P["M"])))


# ---- the shadow model -------------------------------------------------------------------------------------------------------
SETTERS = ("inducing", "data", "targets", "cov_sum", "kernel", "family", "prior", "noise")    # the order `build` applies them in


class Noise:
    """a noise precision with the E[log w] it was set with (sgp_set_noise's second argument; a bare matrix: its default, log w)"""

    def __init__(self, W, E_logw):
        self.W, self.E_logw = np.atleast_2d(np.asarray(W, dtype=np.float64)), float(E_logw)


def noise_matrix(value):
    return value.W if isinstance(value, Noise) else np.asarray(value)


class Shadow:
    """The handle's normal form.  `cur`: the setter values in force; `at`: those of the last sweep; `kind`: "sweep", "psi"
    (sweep_local_psi + sweep_finish), None (no sweep: nothing on the handle can be compared but a sweep) ; `post`: what has changed
    since, in order -- ("set", name, value) with only the last value of a setter kept, ("posterior", mu, Uv) for a foreign q(v).
    `dev`: the setters whose value in force came back from the device ("device-set"); `stats_stale`: the resident statistics have
    been re-formed since the sweep, at a theta or X_u no setter sequence reaches (the objective at another theta, the descents)."""

    def __init__(self):
        self.cur = {n: None for n in SETTERS}
        self.cur["family"] = "se"
        self.at, self.kind, self.post = None, None, []
        self.dev, self.dev_at, self.stats_stale, self.stats_at = set(), set(), False, None

    def set(self, name, value, device=False):
        self.cur[name] = value
        (self.dev.add if device else self.dev.discard)(name)
        drop = {name}
        if name == "data":                                    # set_data resets the targets and the output-covariance sum
            drop |= {"targets", "cov_sum"}
            self.cur["targets"] = self.cur["cov_sum"] = None
        if name == "targets":                                 # set_targets resets the output-covariance sum
            drop.add("cov_sum")
            self.cur["cov_sum"] = None
        if name == "inducing":                                # set_inducing leaves the handle without a q(v)
            drop.add("posterior")
        self.post = [p for p in self.post if not ((p[0] == "set" and p[1] in drop) or (p[0] == "posterior" and "posterior" in drop))]
        self.post.append(("set", name, value))

    def posterior(self, mu, Uv):
        self.post = [p for p in self.post if p[0] != "posterior"]
        self.post.append(("posterior", mu, Uv))

    def swept(self, kind="sweep", psi=None):
        self.at, self.kind, self.post = dict(self.cur), kind, []
        self.dev_at, self.stats_stale, self.stats_at = set(self.dev), False, None
        if kind == "psi":                                     # the handle holds no data afterwards
            self.at["psi"] = psi
            self.cur["data"] = self.cur["targets"] = None
            self.at["data"] = self.at["targets"] = None

    def restat(self, reachable=True):
        """the resident statistics were re-formed at the values in force; `stats_at`: those values where a setter sequence reaches
        them (a fresh handle swept there hands out the same statistics), None where they are the device's (the descents)"""
        self.stats_stale = True
        self.stats_at = dict(self.cur) if reachable and not self.dev else None

    def forget(self):
        """a device-paced training run: its q(v) and its theta are the run's"""
        self.at, self.kind, self.post = None, None, []

    @property
    def device_set(self):
        return bool(self.dev | self.dev_at)

    def normal_form(self):
        """the calls that bring a fresh handle to this state: [(op, args...)]"""
        ops = []
        first = self.at if self.kind else self.cur
        for n in SETTERS:
            if first.get(n) is not None:
                ops.append(("set", n, first[n]))
        if self.kind == "sweep":
            ops.append(("sweep",))
        elif self.kind == "psi":
            ops.append(("psi_sweep", self.at["psi"], self.at["cov_sum"]))
            ops = [o for o in ops if not (o[0] == "set" and o[1] == "cov_sum")]
        return ops + list(self.post) if self.kind else ops


def apply_set(dev, name, value):
    if name == "inducing":
        dev.set_inducing(value)
    elif name == "data":
        X, Y, vy, wts, n_nodes = value
        if wts is None and n_nodes is None:
            dev.set_data(X, Y, vy)
        else:
            dev.set_data(X, Y, vy, wts, n_nodes=n_nodes)
    elif name == "targets":
        dev.set_targets(*value)
    elif name == "cov_sum":
        dev.set_output_cov_sum(value)
    elif name == "kernel":
        dev.set_kernel(*value)
    elif name == "family":
        dev.set_kernel_family(value)
    elif name == "prior":
        if value[0] == "iso":
            dev.set_prior_isotropic(value[1])
        else:
            dev.set_prior_precision(value[1], value[2])
    elif name == "noise":
        dev.set_noise(value.W, value.E_logw) if isinstance(value, Noise) else dev.set_noise(value)
    else:
        raise KeyError(name)


def build(dev, ops):
    """bring a fresh handle to a normal form"""
    for o in ops:
        if o[0] == "set":
            apply_set(dev, o[1], o[2])
        elif o[0] == "sweep":
            dev.sweep()
        elif o[0] == "psi_sweep":
            dev.sweep_local_psi(*o[1])
            if o[2] is not None:
                dev.set_output_cov_sum(o[2])
            dev.sweep_finish()
        elif o[0] == "posterior":
            dev.set_posterior(o[1], o[2])
    return dev


def first_setters(P):
    """the setter values every sequence starts from"""
    vals = dict(inducing=P["Xu"], data=(P["X"], P["Y"], P["vy"], P["wts"], P["n_nodes"]), kernel=P["theta1"], prior=P["prior"],
                noise=P["W"])
    if P["d_out"] > 1:
        vals["cov_sum"] = P["S_y"]
    return vals


def start(devs, P):
    """the common prefix: setters, one sweep, a few reads.  Returns the model."""
    m = Shadow()
    vals = first_setters(P)
    for n in SETTERS:
        if n in vals:
            m.set(n, vals[n])
            for d in devs:
                apply_set(d, n, vals[n])
    for d in devs:
        d.sweep()
        d.predict(P["Xq"])
        d.posterior()
    m.swept()
    return m


# ---- operations -------------------------------------------------------------------------------------------------------------
def _flat(r):
    return tuple(np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in r if a is not None)


class Op:
    """run(dev, P) -> result; out(result) -> tuple of arrays; model(shadow, P, result, dev): what the call does to the normal form (None: nothing); kind: the next
    sweep on a reuse handle; rows: the entry points of the comment table it stands for; restore(dev, P), model_restore: what a sweep
    needs first where the call leaves the handle without data."""

    def __init__(self, run, model=None, kind=REUSED, rows=(), problems=PROBLEMS, nothing=False, restore=None, model_restore=None,
                 out=None, prepare=None, last=None):
        self.run, self.model, self.kind, self.rows, self.problems = run, model, kind, tuple(rows), tuple(problems)
        self.out = out or _flat                               # (readers) the arrays of a result that are compared
        self.nothing, self.restore, self.model_restore = nothing, restore, model_restore
        # prepare(dev, P): what `run` itself does first where the call refuses the problem's state as it stands (a `nothing` call is
        # then held to the state behind prepare + the call's own part, `run` without it being run(dev, P, prepared=True));
        # last: sgp_sweep_kind's `last` behind the call on EVERY handle where the header documents one (None: a sgp_sweep's)
        self.prepare, self.last = prepare, last


def _setter(name, key):
    return dict(run=lambda d, P: apply_set(d, name, P[key] if isinstance(key, str) else key(P)),
                model=lambda m, P, r, d: m.set(name, P[key] if isinstance(key, str) else key(P)))


def _data(P, X="X"):
    return (P[X], P["Y"], P["vy"], P["wts"], P["n_nodes"])


def _psi(P):
    return (P["mean"], P["cov"], P["Yn"])


def _two_phase(d, P):
    d.sweep_local()
    d.sweep_finish()


def _psi_sweep(d, P):
    d.sweep_local_psi(*_psi(P))
    if P["d_out"] > 1:
        d.set_output_cov_sum(P["S_y"])
    d.sweep_finish()


def _m_psi_sweep(m, P, r, d):
    if P["d_out"] > 1:
        m.cur["cov_sum"] = P["S_y"]
    m.swept("psi", _psi(P))


def _restore_data(d, P):
    apply_set(d, "data", _data(P))
    if P["d_out"] > 1:
        apply_set(d, "cov_sum", P["S_y"])


def _m_restore_data(m, P):
    m.set("data", _data(P))
    if P["d_out"] > 1:
        m.set("cov_sum", P["S_y"])


def _sgp_t_gram():
    from gaussianprocessnode_amd import _lib
    return _lib.SGP_T_GRAM


def _allreduce(d, P):
    d.set_allreduce(lambda buf, count, stream: None)         # one rank: the sum is the identity
    d.set_allreduce(None)                                    # (the descents refuse an installed hook)


def _objective_other(xu):
    def run(d, P):
        d.set_kernel(*P["theta2"])
        r = d.theta_objective_xu(want_grad=True) if xu else d.theta_objective(want_grad=True)
        d.set_kernel(*P["theta1"])                           # back at the sweep's theta: the statistics are still theta2's
        return r
    return run


def _m_objective_other(m, P, r, d):
    m.set("kernel", P["theta2"])
    m.restat()                                               # (the statistics are theta2's: a handle swept there has the same)
    m.set("kernel", P["theta1"])


def _m_objective(m, P, r, d):
    """the objective where it stands: it re-forms the statistics unless kernel, inputs and targets are the sweep's"""
    if m.kind != "sweep" or any(p[0] == "set" and p[1] in ("kernel", "family", "inducing", "data", "targets") for p in m.post):
        m.restat()


def _train(d, P):
    d.train_begin(P["X"], P["Y"], P["raw1"], jitter=JITTER)
    d.train_step(0, 128)
    d.train_step(128, 72)
    return d.train_end()


def _restore_train(d, P):
    for n in ("data", "kernel", "prior", "noise"):
        apply_set(d, n, first_setters(P)[n])


def _m_restore_train(m, P):
    for n in ("data", "kernel", "prior", "noise"):
        m.set(n, first_setters(P)[n])


def _kernel_of(raw):
    p = softplus(raw)
    return (float(p[0]), p[1:].copy(), JITTER)


def _descend(psi, steps):
    def run(d, P):
        if psi:
            return d.theta_descend_psi(*_psi(P), P["raw1"], steps, eta=1e-2)
        return d.theta_descend(P["raw1"], steps, eta=1e-2)
    return run


def _m_descend(psi, steps):
    def model(m, P, r, d):
        if steps:
            m.set("kernel", _kernel_of(r[0]), device=True)
            if not psi:
                m.restat(reachable=False)                     # (the last EVALUATED theta's: no setter sequence reaches them)
    return model


def _inducing(psi, steps, learn):
    def run(d, P):
        if psi:
            return d.inducing_descend_psi(*_psi(P), P["raw1"], P["Xu"], steps, learn_theta=learn, eta=1e-2)
        return d.inducing_descend(P["raw1"], P["Xu"], steps, learn_theta=learn, eta=1e-2)
    return run


def _m_inducing(psi, steps):
    def model(m, P, r, d):
        if not steps:
            return
        mu, _, Uv = d.posterior()                             # q(v) stays installed: the host equivalent installs it again
        m.set("kernel", _kernel_of(r[0]), device=True)
        m.set("inducing", r[1].copy(), device=True)
        m.posterior(mu, Uv)
        if not psi:
            m.restat(reachable=False)
    return model


def _m_carry(m, P, r, d):
    """prior <- posterior in natural form, from the statistics the handle hands out: Lambda0 += W (x) Psi2, xi0 += vec(B W)"""
    Psi2, B, _ = d.stats()
    W, Q = noise_matrix(m.cur["noise"]), P["d_out"] * P["M"]
    prior = m.cur["prior"]
    L0, xi0 = (np.eye(Q) / prior[1], np.zeros(Q)) if prior[0] == "iso" else (prior[2], prior[1])
    m.set("prior", ("precision", xi0 + (B.reshape(P["M"], P["d_out"]) @ W).T.ravel(), L0 + np.kron(W, Psi2)), device=True)


def _m_posterior(m, P, r, d):
    m.posterior(*r)


def _set_posterior(d, P):
    mu, _, Uv = d.posterior()
    mu2, Uv2 = 0.9 * mu, 1.1 * Uv
    d.set_posterior(mu2, Uv2)
    return mu2, Uv2


# ---- sgp_vmp_run (d_out = 1 only: `uni`) ---------------------------------------------------------------------------------------
# The call refuses data with point variances, which `uni` carries: every entry first sets (X, Y) alone, and the model records that.
# Kinds by hand from the header: "on a SGP_FLAG_REUSE_STATS handle the statistics stay reusable" -> REUSED; `last` "is FULL after one
# iteration, else REUSED (Gaussian) or TARGETS (Probit)" on every handle.  The host equivalent of a run is the host-paced sequence the
# header names: the last completed iteration's setters (Probit: its q(f) as targets and variances; the noise that entered it with
# E[log w] = psi(a) - log b), one sweep, then set_noise(mean(q(w)), psi(a) - log b).  The noise that entered the last iteration is
# known because the run is made in two calls through `gamma`, documented to equal the single call bitwise.
VMP_PRIOR_G = (1e-2, 1e-2)


def _vmp_data(P, targets=None, variances=None):
    return (P["X"], P["Y"] if targets is None else targets, variances, None, None)


def _vmp_prepare(d, P):
    apply_set(d, "data", _vmp_data(P))


def _gamma_noise(g):
    from scipy.special import digamma
    a, b = float(g[0]), float(g[1])
    return Noise([[a / b]], digamma(a) - math.log(b))


def _vmp_run_0(d, P, prepared=False):
    if not prepared:
        _vmp_prepare(d, P)
        d.sweep()
    return d.vmp_run(0, gamma_prior=VMP_PRIOR_G)


def _m_vmp_run_0(m, P, r, d):
    m.set("data", _vmp_data(P))
    m.swept()


def _vmp_hold(d, P):
    _vmp_prepare(d, P)
    return d.vmp_run(3, hold_w=True)


def _vmp_gauss(d, P):
    _vmp_prepare(d, P)
    _, _, g2, done, _ = d.vmp_run(2, gamma_prior=VMP_PRIOR_G)
    _, _, g3, done2, _ = d.vmp_run(1, gamma_prior=VMP_PRIOR_G, gamma=g2)
    assert (done, done2) == (2, 1)
    return g2, g3


def _m_vmp(m, P, r, d):
    """r = (q(w) that entered the last completed iteration, the final q(w)[, the targets and variances of that iteration])"""
    m.set("data", _vmp_data(P, *r[2:4]), device=len(r) > 2)
    m.set("noise", _gamma_noise(r[0]), device=True)           # (the device's digamma is not SciPy's to the last bit)
    m.swept()
    m.set("noise", _gamma_noise(r[1]), device=True)


def vmp_labels(P):
    return (P["Y"] > 0).astype(np.float64)


def _vmp_probit(d, P):
    from scipy.special import log_ndtr
    from tests import vmp_ref
    lab = vmp_labels(P)
    apply_set(d, "data", _vmp_data(P, lab))
    _, _, g2, done, _ = d.vmp_run(2, likelihood="probit", gamma_prior=VMP_PRIOR_G)
    mu2 = d.posterior(want_cov=False, want_uv=False)[0]
    apply_set(d, "data", _vmp_data(P, lab))                    # the resident targets are q(f) now: the labels again
    _, _, g3, done2, _ = d.vmp_run(1, likelihood="probit", gamma_prior=VMP_PRIOR_G, gamma=g2, mu_init=mu2)
    assert (done, done2) == (2, 1)
    # the last iteration's q(f) in NumPy, from the reference kernel and the mean that entered it
    s2, ell, _ = P["theta1"]
    mz = vmp_ref.kernel(P["Xu"], P["X"], s2, ell).T @ mu2
    mf, vf, _ = vmp_ref.probit_moments(lab, mz, float(g2[1]) / float(g2[0]), log_ndtr)
    return g2, g3, mf, vf


@functools.lru_cache(maxsize=None)
def vmp_tol_stop(pname="uni"):
    """(tol, k): a tol between the restatement's relative decrements at iterations k - 1 and k, so that the run stops after k + 1"""
    from tests import vmp_ref
    P = problem(pname)
    s2, ell, jit = P["theta1"]
    v = vmp_ref.vmp_run_ref(P["X"], P["Y"], P["Xu"], s2, ell, jit, P["prior"], 7, gamma_prior=VMP_PRIOR_G)["values"]
    dec = np.abs(np.diff(v)) / np.abs(v[1:])
    k = 3
    assert dec[k - 1] < dec[k - 2] / 4, ("the trace does not separate the two decrements", dec)
    return float(np.sqrt(dec[k - 1] * dec[k - 2])), k


def _vmp_tol_stop(d, P):
    tol, k = vmp_tol_stop(P["name"])
    _vmp_prepare(d, P)
    _, _, g_in, _, _ = d.vmp_run(k, gamma_prior=VMP_PRIOR_G)   # q(w) entering iteration k (the run below repeats these bitwise)
    values, _, g, done, conv = d.vmp_run(7, gamma_prior=VMP_PRIOR_G, tol=tol)
    assert (done, conv) == (k + 1, True) and np.isnan(values[k + 1:]).all(), (done, conv, values)
    return g_in, g


MUTATORS = {
    "set_inducing": Op(**_setter("inducing", "Xu2"), kind=FULL, rows=["sgp_set_inducing"]),
    "set_data": Op(**_setter("data", lambda P: _data(P, "X2")), kind=FULL, rows=["sgp_set_data"]),
    "set_targets": Op(**_setter("targets", lambda P: (P["Y2"], P["vy"])), kind=TARGETS, rows=["sgp_set_targets"]),
    "set_output_cov_sum": Op(**_setter("cov_sum", "S_y2"), kind=TARGETS, rows=["sgp_set_output_cov_sum"], problems=["multi"]),
    "set_kernel_same": Op(**_setter("kernel", "theta1"), kind=REUSED, rows=["sgp_set_kernel"], nothing=True),
    "set_kernel_new": Op(**_setter("kernel", "theta2"), kind=FULL, rows=["sgp_set_kernel"]),
    "set_kernel_family_same": Op(**_setter("family", "family"), kind=REUSED, rows=["sgp_set_kernel_family"], nothing=True),
    "set_kernel_family_other": Op(**_setter("family", "family2"), kind=FULL, rows=["sgp_set_kernel_family"]),
    "set_noise": Op(**_setter("noise", "W2"), kind=REUSED),
    "set_prior": Op(**_setter("prior", "prior2"), kind=REUSED),
    "bind_stats": Op(lambda d, P: d.bind_stats(0), kind=FULL, rows=["sgp_bind_stats"]),
    "set_allreduce": Op(_allreduce, kind=FULL, rows=["sgp_set_allreduce"]),
    "sweep_local+finish": Op(_two_phase, lambda m, P, r, d: m.swept(), kind=FULL, rows=["sgp_sweep_local"]),
    "sweep": Op(lambda d, P: d.sweep(), lambda m, P, r, d: m.swept(), kind=REUSED, rows=["sgp_sweep"]),
    "time_kernel": Op(lambda d, P: d.time_kernel(_sgp_t_gram(), 2), kind=FULL, rows=["sgp_time_kernel"]),
    "train_run": Op(_train, lambda m, P, r, d: m.forget(), kind=FULL, rows=["sgp_train_begin", "sgp_train_end"], problems=["uni"],
                    restore=_restore_train, model_restore=_m_restore_train),
    "set_posterior": Op(_set_posterior, _m_posterior, kind=REUSED, rows=["sgp_set_posterior"]),
    "carry_posterior": Op(lambda d, P: d.carry_posterior(), _m_carry, kind=REUSED),
    "theta_objective_same": Op(lambda d, P: d.theta_objective(want_grad=True), kind=REUSED, nothing=True),
    "theta_objective_other": Op(_objective_other(False), _m_objective_other, kind=FULL, rows=["sgp_theta_objective"]),
    "theta_objective_xu_same": Op(lambda d, P: d.theta_objective_xu(want_grad=True), kind=REUSED, nothing=True),
    "theta_objective_xu_other": Op(_objective_other(True), _m_objective_other, kind=FULL, rows=["sgp_theta_objective"]),
    "theta_descend_0": Op(_descend(False, 0), _m_descend(False, 0), kind=REUSED, nothing=True),
    "theta_descend_3": Op(_descend(False, 3), _m_descend(False, 3), kind=FULL, rows=["sgp_theta_descend"]),
    "theta_descend_psi_0": Op(_descend(True, 0), _m_descend(True, 0), kind=REUSED, nothing=True),
    "theta_descend_psi_3": Op(_descend(True, 3), _m_descend(True, 3), kind=FULL, rows=["sgp_theta_descend_psi"]),
    "inducing_descend_0": Op(_inducing(False, 0, True), _m_inducing(False, 0), kind=REUSED, nothing=True),
    "inducing_descend_3": Op(_inducing(False, 3, True), _m_inducing(False, 3), kind=FULL, rows=["sgp_inducing_descend"]),
    "inducing_descend_3_xu_only": Op(_inducing(False, 3, False), _m_inducing(False, 3), kind=FULL, rows=["sgp_inducing_descend"]),
    "inducing_descend_psi_0": Op(_inducing(True, 0, True), _m_inducing(True, 0), kind=REUSED, nothing=True),
    "inducing_descend_psi_3": Op(_inducing(True, 3, True), _m_inducing(True, 3), kind=FULL, rows=["sgp_inducing_descend_psi"]),
    "inducing_descend_psi_3_xu_only": Op(_inducing(True, 3, False), _m_inducing(True, 3), kind=FULL,
                                         rows=["sgp_inducing_descend_psi"]),
    "sweep_local_psi+finish": Op(_psi_sweep, _m_psi_sweep, kind=FULL, rows=["sgp_sweep_local_psi"], restore=_restore_data,
                                 model_restore=_m_restore_data),
    "vmp_run_hold_3": Op(_vmp_hold, _m_vmp_run_0, kind=REUSED, rows=["sgp_vmp_run"], problems=["uni"], last=REUSED),
    "vmp_run_gauss_3": Op(_vmp_gauss, _m_vmp, kind=REUSED, rows=["sgp_vmp_run"], problems=["uni"], last=FULL),
    "vmp_run_probit_3": Op(_vmp_probit, _m_vmp, kind=REUSED, rows=["sgp_vmp_run"], problems=["uni"], last=FULL),
    "vmp_run_tol_stop": Op(_vmp_tol_stop, _m_vmp, kind=REUSED, rows=["sgp_vmp_run"], problems=["uni"], last=REUSED),
    # the calls that claim to change nothing
    "vmp_run_0": Op(_vmp_run_0, _m_vmp_run_0, kind=REUSED, rows=["sgp_vmp_run"], problems=["uni"], nothing=True, prepare=_vmp_prepare),
    "psi_stats": Op(lambda d, P: d.psi_stats(P["mean"], P["cov"], want_out=True), nothing=True),
    "theta_objective_psi": Op(lambda d, P: d.theta_objective_psi(*_psi(P), want_grad=True), nothing=True,
                              rows=["sgp_theta_objective_psi"]),
    "theta_objective_psi_xu": Op(lambda d, P: d.theta_objective_psi_xu(*_psi(P), want_grad=True), nothing=True,
                                 rows=["sgp_theta_objective_psi_xu"]),
    "psi_in_grad": Op(lambda d, P: d.psi_in_grad(*_psi(P)), nothing=True, rows=["sgp_psi_in_grad"]),
    "psi_predict": Op(lambda d, P: d.psi_predict(P["mean"], P["cov"]), nothing=True, rows=["sgp_psi_predict"]),
    "predict": Op(lambda d, P: d.predict(P["Xq"]), nothing=True),
    "predict_var": Op(lambda d, P: d.predict_var(P["Xq"]), nothing=True),
    "w_stats": Op(lambda d, P: d.w_stats(), nothing=True, problems=["uni"]),
    "in_message": Op(lambda d, P: d.in_message(P["Xq"], P["qstart"], P["Yq"], weights=P["wq"]), nothing=True),
    "in_message_grad": Op(lambda d, P: d.in_message_grad(P["Xq"], P["qstart"], P["Yq"]), nothing=True),
    "out_message": Op(lambda d, P: d.out_message(P["Xq"], P["qstart"], weights=P["wq"]), nothing=True),
}


# what a reader's arrays are, for the bounds of a device-set history: "value" (1e-12 relative), "grad" (rtol 1e-9, atol 1e-9
# max|grad|), "snapshot" (the parity suite's cond-scaled bounds)
READERS = {
    "stats": Op(lambda d, P: d.stats()),
    "w_stats": Op(lambda d, P: d.w_stats(), problems=["uni"]),
    "predict": Op(lambda d, P: [d.predict(P["Xq"])]),
    "predict_var": Op(lambda d, P: d.predict_var(P["Xq"])),
    "in_message": Op(lambda d, P: d.in_message(P["Xq"], P["qstart"], P["Yq"], weights=P["wq"])),
    "in_message_grad": Op(lambda d, P: d.in_message_grad(P["Xq"], P["qstart"], P["Yq"])),
    "out_message": Op(lambda d, P: [d.out_message(P["Xq"], P["qstart"], weights=P["wq"])]),
    "theta_objective": Op(lambda d, P: d.theta_objective(want_grad=True), _m_objective),
    "theta_objective_xu": Op(lambda d, P: d.theta_objective_xu(want_grad=True), _m_objective),
    "theta_descend_1": Op(lambda d, P: d.theta_descend(P["raw2"], 1, eta=1e-2), _m_descend(False, 1),
                          out=lambda r: _flat([r[1][:1]])),   # first value only
    "inducing_descend_1": Op(lambda d, P: d.inducing_descend(P["raw2"], P["Xu2"], 1, learn_theta=False, eta=1e-2),
                             _m_inducing(False, 1), out=lambda r: _flat([r[2][:1]])),
    "sweep": Op(None, lambda m, P, r, d: m.swept()),           # sweep + snapshot: the GPU test supplies the snapshot
}
# the readers sgp_set_posterior is documented to refuse (it carries no Sigma_v), with an explicit q(v) instead
EXPLICIT_QV = {
    "predict_var": lambda d, P, mu, Sig: d.predict_var(P["Xq"], mu_v=mu, Sigma_v=Sig),
    "in_message": lambda d, P, mu, Sig: d.in_message(P["Xq"], P["qstart"], P["Yq"], weights=P["wq"], mu_v=mu, Sigma_v=Sig),
    "in_message_grad": lambda d, P, mu, Sig: d.in_message_grad(P["Xq"], P["qstart"], P["Yq"], mu_v=mu, Sigma_v=Sig),
}
GRADIENTS = {"theta_objective": (1,), "theta_objective_xu": (1, 2), "in_message_grad": (1, 2)}   # which arrays are gradients
# A-C pairs of a history that is not device-set and still not bitwise, each with the code that orders the sums differently: these
# pairs alone are held to the parity suite's bound (post_tol at cond(K_uu)) instead
ORDER_PAIRS = {
    # A evaluates on sgp_theta_objective's re-evaluation path (theta_objective_eval: R_v = Uv' Uv from theta_Rv, the traces and
    # k_scalars again), C on its fresh path (the sums sgp_sweep's own k_scalars left in dOut, traced against the sweep's R): d_out = 1
    ("theta_objective_other", "theta_objective", "uni"), ("theta_objective_other", "theta_objective_xu", "uni"),
    ("theta_objective_xu_other", "theta_objective", "uni"), ("theta_objective_xu_other", "theta_objective_xu", "uni"),
}
STATS_READERS = ("stats", "w_stats")                          # they hand out the resident statistics / K_uf as they are


# ---- the ledger: every exported entry point has a class -------------------------------------------------------------------------
MUTATOR, READER, NO_STATE = "mutator", "reader", "no handle state"
ENTRY_POINTS = {
    **{n: MUTATOR for n in (
        "sgp_set_inducing", "sgp_set_data", "sgp_set_targets", "sgp_set_output_cov_sum", "sgp_set_kernel", "sgp_set_kernel_family",
        "sgp_set_prior", "sgp_set_noise", "sgp_sweep_local", "sgp_sweep_finish", "sgp_sweep", "sgp_bind_stats", "sgp_set_allreduce",
        "sgp_use_rccl",                # (the set_allreduce row: it installs the hook; driving it needs a communicator)
        "sgp_time_kernel", "sgp_train_begin", "sgp_train_step", "sgp_train_end", "sgp_train_likelihood", "sgp_set_posterior",
        "sgp_carry_posterior", "sgp_theta_descend", "sgp_theta_descend_psi", "sgp_inducing_descend", "sgp_inducing_descend_psi",
        "sgp_sweep_local_psi", "sgp_vmp_run")},
    **{n: READER for n in (
        "sgp_get_posterior", "sgp_get_scalars", "sgp_get_stats", "sgp_get_kuu_chol", "sgp_get_wishart_invscale", "sgp_sweep_kind",
        "sgp_w_stats", "sgp_predict", "sgp_predict_var", "sgp_in_message", "sgp_in_message_grad", "sgp_out_message",
        "sgp_theta_objective", "sgp_theta_objective_xu",      # (mutators too, at another theta: MUTATORS has both variants)
        "sgp_psi_stats", "sgp_theta_objective_psi", "sgp_theta_objective_psi_xu", "sgp_psi_in_grad", "sgp_psi_predict",
        "sgp_train_get_gamma")},
    **{n: NO_STATE for n in (
        "sgp_abi_version", "sgp_create", "sgp_destroy", "sgp_last_error", "sgp_wait", "sgp_stats_layout", "sgp_overlap_plan",
        "sgp_sweep_plan",              # (reads the bits the last sweep recorded: tests/test_gpu_sweep_plans.py)
        "sgp_kernelmatrix", "sgp_kernelmatrix_family", "sgp_potrf", "sgp_potri", "sgp_measure_sclk_mhz", "sgp_measure_clocks",
        "sgp_get_timestamps", "sgp_get_phase_totals", "sgp_get_chain_trace", "sgp_get_step_trace", "sgp_get_sweep_trace")},
}
# rows of the comment table that no call sequence can reach without making a sweep fail on purpose
UNREACHABLE_ROWS = ("next_kind",)


def exported_names(header_text):
    """the sgp_* functions include/sgp_hip.h declares"""
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(sgp_\w+)\s*\(", header_text, flags=re.M)))


def table_rows(api_text):
    """the rows of the "Entry point -> effect" comment: [(names in the row's left column, the row's text)]"""
    body = api_text.split("Entry point -> effect:", 1)[1].split("struct StatsRecord", 1)[0]
    rows = []
    for line in body.splitlines():
        m = re.match(r"//   (\S.{0,44}?)\s{2,}\S", line)
        if m and not line.startswith("//    "):
            rows.append((re.findall(r"sgp_\w+|next_kind|use_rccl", m.group(1)), line))
    return rows
