"""sgp_vmp_run_w on the GPU against tests/vmp_w_ref.py, at the branch points of its kernels, and what the call leaves behind.

The tolerance rule is that of tests/test_gpu_vmp_run.py, restated: per quantity, 10 x the larger of |extended-precision restatement -
float64 restatement| and |float64 restatement - the restatement with Psi2, B and W_bar displaced relatively by 50 eps at every
iteration|; none is taken from the code under test.  Every error / tolerance ratio is printed.  The largest one seen is recorded in
profiles/vmp_wishart.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import vmp_ref as R
from tests import vmp_w_ref as W

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SGP_ERR_ARG = -1                                             # include/sgp_hip.h
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vmp_run_neighbour.npz")

# name: (T nodes, S points per node, M, D, d, family, prior form, covariance sum)
CASES = {
    "q40_iso": (50, 1, 20, 1, 2, "se", "iso", False),               # Q = 40 < 256: one workgroup of k_vmp_kl
    "q280_dense": (60, 1, 70, 2, 4, "matern32", "precision", False),  # Q = 280 > 256, M no multiple of 64, dense prior (form 1)
    "one_node": (1, 1, 8, 1, 3, "se", "meancov", False),            # one node, prior form 0
    "pendulum": (30, 5, 48, 2, 2, "se", "iso", True),               # 30 nodes x 5 weighted points, a covariance sum, N = 30
}


@functools.lru_cache(maxsize=None)
def problem(name):
    T, S, M, D, d, family, form, cov = CASES[name]
    pts, wts, Y, Xu = W.make_problem(T, S, M, D, d, seed=sum(map(ord, name)))
    Q = d * M
    if form == "iso":
        prior = ("iso", 50.0)
    else:
        rng = np.random.default_rng(7)
        A = rng.normal(size=(Q, Q)) / np.sqrt(Q)
        S0 = 2.0 * np.eye(Q) + A @ A.T
        m0 = 0.3 * rng.normal(size=Q)
        prior = ("meancov", m0, S0) if form == "meancov" else ("precision", np.linalg.solve(S0, m0), np.linalg.inv(S0))
    R0 = 0.5 * np.eye(d) + 0.1
    return dict(pts=pts, wts=wts, Y=Y, Xu=Xu, s2=0.8, ell=np.full(D, 0.5 * np.sqrt(D)), jitter=1e-6, prior=prior, family=family,
                w_prior=(d + 2.0, R0), cov=T * 0.01 * (np.eye(d) + 0.3) if cov else None, T=T, S=S, M=M, D=D, d=d)


def ref_run(P, K, **kw):
    return W.vmp_run_w_ref(P["pts"], P["wts"], P["Y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], K, cov_sum=P["cov"],
                           family=P["family"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name, K, hold=False):
    """(float64 run, per-quantity tolerance) -- computed once per case and shared"""
    P = problem(name)
    kw = dict(hold_w=HOLD(P["d"])) if hold else dict(w_prior=P["w_prior"])
    ref, ext, dis = ref_run(P, K, **kw), ref_run(P, K, dtype=np.longdouble, **kw), ref_run(P, K, displace=50 * EPS, **kw)
    tol = {}
    for q in ("values", "terms", "mu", "Sigma") + (() if hold else ("R",)):
        worst = np.maximum(np.abs(np.asarray(ext[q], dtype=np.float64) - ref[q]), np.abs(dis[q] - ref[q]))
        tol[q] = 10 * (worst.max(axis=0) if q == "terms" else worst.max())
    return ref, tol


def HOLD(d):
    Wb = 3.0 * np.eye(d) + 0.5
    return Wb, float(np.linalg.slogdet(Wb)[1]) - 0.1


def device(name, reuse=True, Xu=None, jitter=None):
    from gaussianprocessnode_amd import SGPDevice
    from gaussianprocessnode_amd.meta import set_engine_kernel
    P = problem(name)
    X, y, w, n_nodes = W.flat(P["pts"], P["wts"], P["Y"])
    dev = SGPDevice(len(X), P["M"], P["D"], P["d"], reuse_stats=reuse)
    dev.set_inducing(P["Xu"] if Xu is None else Xu)
    set_engine_kernel(dev, P["s2"], P["ell"], P["jitter"] if jitter is None else jitter, P["family"])
    if P["prior"][0] == "iso":
        dev.set_prior_isotropic(P["prior"][1])
    elif P["prior"][0] == "meancov":
        dev.set_prior_meancov(P["prior"][1], P["prior"][2])
    else:
        dev.set_prior_precision(P["prior"][1], P["prior"][2])
    dev.set_data(X, y, weights=w, n_nodes=n_nodes)
    if P["cov"] is not None:
        dev.set_output_cov_sum(P["cov"])
    return dev, P


def ratios_of(values, terms, mu, Sigma, q_w, rk, tol):
    ratios = dict(values=np.abs(values - rk["values"]).max() / tol["values"], mu=np.abs(mu - rk["mu"]).max() / tol["mu"],
                  Sigma=np.abs(Sigma - rk["Sigma"]).max() / tol["Sigma"])
    for j in range(4):                                        # (a term that is exactly 0 in the restatement is 0)
        err, t = np.abs(terms[:, j] - rk["terms"][:, j]).max(), tol["terms"][j]
        ratios[f"terms{j}"] = err / t if t > 0 else (np.inf if err > 0 else 0.0)
    if q_w is not None:
        ratios["R"] = np.abs(q_w.invS - rk["R"]).max() / tol["R"]
    return ratios


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(name):
    for K in (1, 7):
        rk, tol = reference(name, K)
        dev, P = device(name)
        with dev:
            values, terms, q_w, done, conv = dev.vmp_run_w(K, wishart_prior=P["w_prior"])
            mu, Sigma, _ = dev.posterior(want_uv=False)
            sc = dev.stats()[2]
        assert done == K and not conv
        assert q_w.nu == rk["nu"] == P["w_prior"][0] + P["T"] and sc[2] == P["T"]       # N is the number of nodes, not of points
        assert np.all(terms[:, 1] == 0.0)
        ratios = ratios_of(values, terms, mu, Sigma, q_w, rk, tol)
        print(f"vmp_run_w {name} K={K} error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios


def test_identical_calls_and_split_runs_agree_bitwise():
    out = []
    for split in ((7,), (7,), (3, 4)):
        dev, P = device("pendulum")
        with dev:
            q_w, vals, trms = None, [], []
            for K in split:
                v, t, q_w, done, _ = dev.vmp_run_w(K, wishart_prior=P["w_prior"], wishart=q_w)
                assert done == K
                vals.append(v)
                trms.append(t)
            mu, Sigma, _ = dev.posterior(want_uv=False)
        out.append((np.concatenate(vals), np.concatenate(trms), mu, Sigma, np.array([q_w.nu]), q_w.invS))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


def host_sequence(dev, P, K, displace_w=0.0):
    """the host-paced sequence of existing calls on a prepared handle: set_noise, sweep, wishart_invscale per iteration, then the
    noise of the final q(W); W_bar optionally displaced relatively at every iteration.  Returns the final (nu, R)."""
    from scipy.special import digamma
    nu0, R0 = P["w_prior"]
    nu, Rm = nu0, R0
    for _ in range(K):
        Wb, el = W.wishart_mean_logdet(nu, Rm, digamma)
        dev.set_noise(Wb * (1.0 + displace_w), float(el))
        dev.sweep()
        nu, Rm = nu0 + P["T"], R0 + dev.wishart_invscale()
    Wb, el = W.wishart_mean_logdet(nu, Rm, digamma)
    dev.set_noise(Wb, float(el))
    return nu, Rm


def state_of(dev):
    sc = dev.scalars()
    mu, Sigma, _ = dev.posterior(want_uv=False)
    return dict(mu=mu, Sigma=Sigma, S=dev.wishart_invscale(),
                sums=np.array([sc.sum_I1, sc.energy, sc.logdet_kuu, sc.logdet_lambda])), dev.sweep_kind()


@pytest.mark.parametrize("name", ["pendulum", "q40_iso"])
def test_state_equals_the_host_paced_sequence(name):
    K, seq = 4, []
    for dw in (0.0, 4 * EPS):
        dev, P = device(name)
        with dev:
            nu, Rm = host_sequence(dev, P, K, dw)
            seq.append((state_of(dev), Rm))
    dev, P = device(name)
    with dev:
        _, _, q_w, done, _ = dev.vmp_run_w(K, wishart_prior=P["w_prior"])
        got, kinds = state_of(dev)
        assert done == K and kinds == seq[0][0][1] and kinds[1] == 2          # SGP_SWEEP_REUSED
        assert q_w.nu == nu
        for q in got:
            tol = 10 * np.abs(seq[1][0][0][q] - seq[0][0][0][q]).max()
            err = np.abs(got[q] - seq[0][0][0][q]).max()
            print(f"vmp_run_w {name} state {q}: error/tolerance {err / tol if tol > 0 else float(err > 0):.3g}")
            assert err <= tol, q
        assert np.abs(q_w.invS - seq[0][1]).max() <= 10 * np.abs(seq[1][1] - seq[0][1]).max()
        dev.sweep()                                           # the statistics stayed reusable
        assert dev.sweep_kind()[1] == 2
    dev, P = device(name, reuse=False)                        # without SGP_FLAG_REUSE_STATS the run is the same
    with dev:
        _, _, q2, _, _ = dev.vmp_run_w(K, wishart_prior=P["w_prior"])
        assert np.array_equal(q2.invS, q_w.invS) and dev.sweep_kind()[1] == 2
    dev, P = device(name)
    with dev:
        assert dev.vmp_run_w(1, wishart_prior=P["w_prior"])[3] == 1 and dev.sweep_kind()[1] == 0     # FULL after one iteration


def test_hold_w():
    """q(W) held: terms[3] = 0, the noise is unchanged, the values are the restatement's; and -- the noise being the one the last
    sweep ran at -- a following sgp_sweep is a REUSED sweep that reproduces the last q(v) bitwise.  (Without HOLD_W the call leaves the
    NEW noise in force, as the host-paced sequence does: the following sweep is REUSED -- test_state_equals_the_host_paced_sequence --
    and is the next iteration's q(v), not the last one's.)"""
    K = 7
    rk, tol = reference("pendulum", K, hold=True)
    dev, P = device("pendulum")
    Wb, el = HOLD(P["d"])
    with dev:
        dev.set_noise(Wb, el)
        values, terms, q_w, done, conv = dev.vmp_run_w(K, hold_w=True)
        mu, Sigma, _ = dev.posterior(want_uv=False)
        assert q_w is None and done == K and np.all(terms[:, 3] == 0.0)
        ratios = ratios_of(values, terms, mu, Sigma, None, rk, tol)
        print("vmp_run_w hold_w error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios
        dev.sweep()
        mu2, Sigma2, _ = dev.posterior(want_uv=False)
        assert dev.sweep_kind()[1] == 2 and np.array_equal(mu2, mu) and np.array_equal(Sigma2, Sigma)
        # unchanged noise: the host-paced sweep at (Wb, el) gives the same energy as the run's first term
        assert abs(dev.scalars().energy - terms[-1, 0]) <= 1e-12 * abs(terms[-1, 0])


def test_the_tol_stop():
    name, K = "q40_iso", 7
    v = reference(name, K)[0]["values"]
    dec = np.abs(np.diff(v)) / np.abs(v[1:])                  # dec[k - 1]: the relative decrement at iteration k
    k = next(i for i in range(1, K - 1) if dec[i] < 0.5 * dec[:i].min() and dec[i] > 1e-12)   # the stop: iteration k + 1
    tol = float(np.sqrt(dec[:k].min() * dec[k]))
    dev, P = device(name)
    with dev:
        values, terms, q_w, done, conv = dev.vmp_run_w(K, wishart_prior=P["w_prior"], tol=tol)
        assert conv and done == k + 2
        assert np.isfinite(values[:done]).all() and np.isnan(values[done:]).all() and np.isnan(terms[done:]).all()
        mu, _, _ = dev.posterior(want_cov=False, want_uv=False)
    dev, P = device(name)
    with dev:
        v2, _, q2, _, _ = dev.vmp_run_w(done, wishart_prior=P["w_prior"])
        assert np.array_equal(v2, values[:done]) and np.array_equal(q2.invS, q_w.invS)
        assert np.array_equal(dev.posterior(want_cov=False, want_uv=False)[0], mu)


def test_the_failure_stop():
    """K_uu not positive definite (two equal inducing inputs, no jitter): an ordinary status return at iteration 0"""
    P = problem("q40_iso")
    Xu = P["Xu"].copy()
    Xu[3] = Xu[2]
    dev, _ = device("q40_iso", Xu=Xu, jitter=0.0)
    with dev:
        with pytest.raises(np.linalg.LinAlgError, match="iteration 0: K_uu is not positive definite") as e:
            dev.vmp_run_w(3, wishart_prior=P["w_prior"])
        assert e.value.iterations_done == 0 and e.value.counts[1] == -e.value.minor < 0 and np.isnan(e.value.values).all()
        assert e.value.wishart.nu == P["w_prior"][0] and np.array_equal(e.value.wishart.invS, P["w_prior"][1])
        dev.set_inducing(P["Xu"])                             # the handle stays usable
        assert dev.vmp_run_w(2, wishart_prior=P["w_prior"])[3] == 2


def test_refusals():
    from gaussianprocessnode_amd import SGPDevice, SGPError
    dev, P = device("q40_iso")
    d, prior = P["d"], P["w_prior"]
    X, y, _, _ = W.flat(P["pts"], P["wts"], P["Y"])

    def raw(flags, K, p0, q, tol=0.0):
        pk = lambda v: None if v is None else np.ascontiguousarray(np.concatenate([[v[0]], np.asarray(v[1], dtype=np.float64).T.ravel()]))
        a, b = pk(p0), pk(q)
        ptr = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
        rc = dev._lib.sgp_vmp_run_w(dev._h, flags, K, ptr(a), ptr(b), tol, None, None, None)
        return rc, (dev._lib.sgp_last_error(dev._h) or b"").decode()

    bad_sym, bad_pd, bad_nan = prior[1].copy(), prior[1].copy(), prior[1].copy()
    bad_sym[0, 1] += 1e-3
    bad_pd[0, 1] = bad_pd[1, 0] = 5.0
    bad_nan[1, 1] = np.nan
    with dev:
        for args, msg in (((0, -1, prior, prior), "iterations must be >= 0"), ((2, 1, prior, prior), "unknown flags"),
                          ((0, 1, prior, prior, -1.0), "tol must be >= 0"), ((0, 1, prior, prior, float("nan")), "tol must be >= 0"),
                          ((0, 1, None, prior), "wishart_prior and wishart are required"), ((0, 1, prior, None), "wishart_prior and wishart are required"),
                          ((0, 1, (d - 1.0, prior[1]), prior), "wishart_prior: the degrees of freedom"),
                          ((0, 1, prior, (d - 1.0, prior[1])), "wishart: the degrees of freedom"),
                          ((0, 1, (float("inf"), prior[1]), prior), "wishart_prior: the degrees of freedom"),
                          ((0, 1, (prior[0], bad_nan), prior), "wishart_prior: the inverse scale has a non-finite entry"),
                          ((0, 1, prior, (prior[0], bad_sym)), "wishart: the inverse scale is not symmetric"),
                          ((0, 1, (prior[0], bad_pd), prior), "wishart_prior: the inverse scale is not positive definite")):
            rc, err = raw(*args)
            assert rc == SGP_ERR_ARG and msg in err and err.startswith("sgp_vmp_run_w: "), (args[:2], err)
        dev.set_allreduce(lambda buf, count, stream: None)
        with pytest.raises(SGPError, match="data-sharded runs are not supported"):
            dev.vmp_run_w(1, wishart_prior=prior)
        dev.set_allreduce(None)
        with pytest.raises(SGPError, match="y_var is only defined for d_out = 1"):
            dev.set_data(X, y, y_var=np.full(len(X), 0.1))   # data with y_var cannot become resident on a MultiSGP handle at all:
        dev.set_data(X, y)                                    # the run's own y_var rule is a guard no call sequence reaches
        assert dev.vmp_run_w(0, wishart_prior=prior)[3] == 0  # iterations = 0: nothing happens, behind every refusal
        assert dev.vmp_run_w(2, wishart_prior=prior)[3] == 2  # the handle is usable after every refusal
        # exact Psi-statistics resident
        dev.sweep_local_psi(X, np.tile(0.01 * np.eye(P["D"]), (len(X), 1, 1)), y)
        dev.sweep_finish()
        with pytest.raises(SGPError, match="exact Psi-statistics"):
            dev.vmp_run_w(1, wishart_prior=prior)
    with SGPDevice(8, 4, 1) as uni:                            # d_out = 1
        with pytest.raises(SGPError, match="MultiSGP handles only"):
            uni.vmp_run_w(1, wishart_prior=(3.0, np.eye(1)))
    with SGPDevice(8, 4, 1, 2) as empty:                       # nothing set
        with pytest.raises(SGPError, match="set_inducing, set_kernel and set_data"):
            empty.vmp_run_w(1, wishart_prior=(4.0, np.eye(2)))
    # (an open sgp_train_* run cannot be reached on a MultiSGP handle: sgp_train_begin refuses d_out > 1, and on a UniSGP handle
    # the d_out refusal comes first; the rule itself is vmp_check_handle's, which tests/test_gpu_vmp_run.py drives)


def neighbour_case():
    """one fixed sgp_vmp_run case of the neighbouring entry point: Gaussian and Probit, five and three iterations"""
    from gaussianprocessnode_amd import SGPDevice
    out = {}
    for lik, K in (("gaussian", 5), ("probit", 3)):
        X, y, Xu = R.make_toy(200, 30, 2, seed=3, probit=lik == "probit")
        with SGPDevice(200, 30, 2) as dev:
            dev.set_inducing(Xu)
            dev.set_kernel(0.8, [1.2, 0.9], 1e-6)
            dev.set_prior_isotropic(50.0)
            dev.set_data(X, y)
            values, terms, gamma, _, _ = dev.vmp_run(K, likelihood=lik, gamma_prior=(1e-2, 1e-2))
            out[lik + "_values"], out[lik + "_terms"], out[lik + "_gamma"] = values, terms, np.asarray(gamma)
            out[lik + "_mu"] = dev.posterior(want_cov=False, want_uv=False)[0]
    return out


def test_the_neighbour_is_unchanged():
    """sgp_vmp_run returns bitwise what the library of the parent commit returned (tests/golden/vmp_run_neighbour.npz, written by
    neighbour_case() run against that library)"""
    want, got = np.load(GOLDEN), neighbour_case()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert np.array_equal(want[k], got[k]), k


def test_train_vmp_regression_multi_both_ways():
    """train.vmp_regression_multi, device-paced and host-paced, gives the restatement's free energies and q(W): PointMass inputs, the
    prior N(0, 50 I) given as a dense precision (as vmp_gpssm gives it)"""
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.meta import MultiSGPMeta
    T, M, D, d, K = 50, 20, 1, 2, 5
    pts, wts, Y, Xu = W.make_problem(T, 1, M, D, d, seed=21)
    s2, ell, R0 = 0.8, np.full(D, 0.5), 0.5 * np.eye(d) + 0.1
    args = (pts, wts, Y, Xu, s2, ell, 1e-6, ("precision", np.zeros(d * M), np.eye(d * M) / 50.0), K)
    ref = W.vmp_run_w_ref(*args, w_prior=(d + 2.0, R0))
    ext = W.vmp_run_w_ref(*args, w_prior=(d + 2.0, R0), dtype=np.longdouble)
    dis = W.vmp_run_w_ref(*args, w_prior=(d + 2.0, R0), displace=50 * EPS)
    tol = {q: 10 * max(np.abs(np.asarray(ext[q], dtype=np.float64) - ref[q]).max(), np.abs(dis[q] - ref[q]).max()) for q in ("values", "R", "mu")}
    for paced in (True, False):
        meta = MultiSGPMeta(None, Xu, None, None, None, None, lambda th: (s2, ell), jitter=1e-6)
        try:
            q_v, q_w, fe = train.vmp_regression_multi(np.zeros(2), pts[:, 0, :], Y, meta, iterations=K, w_prior=(d + 2.0, R0),
                                                      device_paced=paced)
        finally:
            if meta.engine is not None:
                meta.engine.close()
        ratios = dict(values=np.abs(fe - ref["values"]).max() / tol["values"], R=np.abs(q_w.invS - ref["R"]).max() / tol["R"],
                      mu=np.abs(q_v.m - ref["mu"]).max() / tol["mu"])
        print(f"vmp_regression_multi device_paced={paced} error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert q_w.nu == ref["nu"] and all(v <= 1.0 for v in ratios.values()), ratios


def test_the_wishart_failure_stop():
    """R0 + S not positive definite -- an output covariance sum of -1e3 I makes S negative definite --: the run stops at iteration 0
    like a failed factorisation, q(W) comes back unchanged, and the handle stays usable"""
    dev, P = device("pendulum")
    with dev:
        dev.set_output_cov_sum(-1e3 * np.eye(P["d"]))
        with pytest.raises(np.linalg.LinAlgError, match=r"iteration 0: the Wishart inverse scale R0 \+ S is not positive definite") as e:
            dev.vmp_run_w(3, wishart_prior=P["w_prior"])
        assert e.value.minor == 1 and e.value.counts == (0, -1) and np.isnan(e.value.values).all() and np.isnan(e.value.terms).all()
        assert e.value.wishart.nu == P["w_prior"][0] and np.array_equal(e.value.wishart.invS, P["w_prior"][1])
        dev.set_output_cov_sum(P["cov"])
        values, _, q_w, done, _ = dev.vmp_run_w(7, wishart_prior=P["w_prior"])
        rk, tol = reference("pendulum", 7)
        assert done == 7 and np.abs(values - rk["values"]).max() <= tol["values"] and np.abs(q_w.invS - rk["R"]).max() <= tol["R"]


def test_train_vmp_regression_multi_gaussian_inputs():
    """q_ins: Gaussian inputs held fixed enter as the weighted points of meta.method's cubature rule (restated here: 2 D + 1 points
    m +- sqrt(D + 1) L e_i with weights 1 / (2 (D + 1)), and m with 1 / (D + 1)), N = the number of nodes; device- and host-paced.
    iterations = 0 returns the priors and an empty trace either way."""
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.cubature import SphericalRadialCubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance
    from gaussianprocessnode_amd.meta import MultiSGPMeta
    T, M, D, d, K = 30, 20, 2, 2, 5
    centres, _, Y, Xu = W.make_problem(T, 1, M, D, d, seed=33)
    rng = np.random.default_rng(34)
    covs = [0.02 * np.eye(D) + 0.01 * np.outer(v, v) for v in rng.normal(size=(T, D))]
    r = np.sqrt(D + 1.0)
    pts = np.stack([np.stack([m + r * L[:, i] for i in range(D)] + [m - r * L[:, i] for i in range(D)] + [m])
                    for m, L in ((centres[t, 0], np.linalg.cholesky(covs[t])) for t in range(T))])
    wts = np.tile(np.concatenate([np.full(2 * D, 0.5 / (D + 1.0)), [1.0 / (D + 1.0)]]), (T, 1))
    s2, ell, w_prior = 0.8, np.full(D, 0.5 * np.sqrt(D)), (d + 2.0, 0.5 * np.eye(d) + 0.1)
    args = (pts, wts, Y, Xu, s2, ell, 1e-6, ("precision", np.zeros(d * M), np.eye(d * M) / 50.0), K)
    ref = W.vmp_run_w_ref(*args, w_prior=w_prior)
    ext = W.vmp_run_w_ref(*args, w_prior=w_prior, dtype=np.longdouble)
    dis = W.vmp_run_w_ref(*args, w_prior=w_prior, displace=50 * EPS)
    tol = {q: 10 * max(np.abs(np.asarray(ext[q], dtype=np.float64) - ref[q]).max(), np.abs(dis[q] - ref[q]).max()) for q in ("values", "R", "mu")}
    q_ins = [MvNormalMeanCovariance(centres[t, 0], covs[t]) for t in range(T)]
    for paced in (True, False):
        meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, lambda th: (s2, ell), jitter=1e-6)
        try:
            q_v0, q_w0, fe0 = train.vmp_regression_multi(np.zeros(2), None, Y, meta, iterations=0, w_prior=w_prior, device_paced=paced,
                                                         q_ins=q_ins)
            assert len(fe0) == 0 and q_w0.nu == w_prior[0] and np.array_equal(q_v0.S, 50.0 * np.eye(d * M))
            q_v, q_w = train.vmp_regression_multi(np.zeros(2), None, Y, meta, iterations=K, w_prior=w_prior, device_paced=paced,
                                                  q_ins=q_ins, free_energy=False)
            q_v2, q_w2, fe = train.vmp_regression_multi(np.zeros(2), None, Y, meta, iterations=K, w_prior=w_prior, device_paced=paced,
                                                        q_ins=q_ins)
        finally:
            if meta.engine is not None:
                meta.engine.close()
        assert np.array_equal(q_w.invS, q_w2.invS) and np.array_equal(q_v.m, q_v2.m)
        ratios = dict(values=np.abs(fe - ref["values"]).max() / tol["values"], R=np.abs(q_w.invS - ref["R"]).max() / tol["R"],
                      mu=np.abs(q_v.m - ref["mu"]).max() / tol["mu"])
        print(f"vmp_regression_multi q_ins device_paced={paced} error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert q_w.nu == ref["nu"] == w_prior[0] + T and all(v <= 1.0 for v in ratios.values()), ratios
