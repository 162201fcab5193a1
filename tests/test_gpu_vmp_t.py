"""sgp_vmp_run_t on the GPU against tests/vmp_t_ref.py, against the host-paced loop of existing calls, its properties (monotone
values, the Gaussian limit, bitwise repeatability and continuation, the two stops, the state it leaves, robustness) and every refusal.

Tolerances: the rule of tests/test_gpu_vmp_run.py (vmp_t_ref.tolerances): per quantity 10 x the larger of the restatement's
float64-vs-extended difference and its change under a relative displacement of Psi2, B and w by 50 eps per iteration, from a
K-iteration reference.  None is taken from the code under test."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import vmp_ref as R
from tests import vmp_t_ref as T

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PRIOR_G = (1e-2, 1e-2)
HOLD = (3.0, float(np.log(3.0)))

# name -> (N, M, D, K, nu, family, prior form, hold_w); each chosen for a branch
CASES = {
    "tiny": (3, 2, 1, 3, 4.0, "se", "iso", False),
    "wg257": (257, 8, 1, 3, 4.0, "se", "iso", False),            # the second workgroup of k_t_points holds one point
    "tiles": (300, 65, 2, 4, 4.0, "se", "iso", False),           # two tile columns
    "reduce_65537": (65537, 8, 1, 2, 4.0, "se", "iso", False),   # 257 triples: the reduce stages' second pass, with one triple
    "meancov": (300, 20, 2, 3, 4.0, "se", "meancov", False),
    "precision": (300, 20, 2, 3, 4.0, "se", "precision", False),
    "matern12": (257, 20, 2, 3, 4.0, "matern12", "iso", False),
    "matern32": (257, 20, 2, 3, 4.0, "matern32", "iso", False),
    "matern52": (257, 20, 2, 3, 4.0, "matern52", "iso", False),
    "hold_w": (300, 20, 2, 3, 4.0, "se", "iso", True),
    "nu0.5": (257, 8, 1, 3, 0.5, "se", "iso", False),            # alpha = 0.75: twenty steps of the digamma recurrence
    "nu25": (257, 8, 1, 3, 25.0, "se", "iso", False),            # alpha = 13: seven
    "nu1e8": (257, 8, 1, 3, 1e8, "se", "iso", False),            # none; the Gamma KL's halves cancel to O(1 / nu)
    "outliers": (200, 12, 1, 6, 4.0, "se", "iso", False),        # 5 % of the targets displaced by 20 sigma
}
SEED = 11


@functools.lru_cache(maxsize=None)
def problem(name):
    N, M, D, K, nu, family, form, hold = CASES[name]
    if name == "outliers":
        X, y, Xu, clean, f = T.make_outlier_toy(N, M, seed=2)
        ell, s2 = np.array([0.7]), 1.0
    else:
        X, y, Xu = R.make_toy(N, min(M, N), D, seed=SEED)
        ell, s2, clean, f = np.full(D, 0.5 * np.sqrt(D)), 0.8, None, None
    rng = np.random.default_rng(7)
    if form == "iso":
        prior = ("iso", 50.0)
    else:
        A = rng.normal(size=(M, M)) / np.sqrt(M)
        S0 = 2.0 * np.eye(M) + A @ A.T
        m0 = 0.3 * rng.normal(size=M)
        prior = ("meancov", m0, S0) if form == "meancov" else ("precision", np.linalg.solve(S0, m0), np.linalg.inv(S0))
    return dict(X=X, y=y, Xu=Xu, s2=s2, ell=ell, jitter=1e-6, prior=prior, family=family, hold=HOLD if hold else None, M=M, N=N, D=D,
                K=K, nu=nu, g0=PRIOR_G, clean=clean, f=f)


@functools.lru_cache(maxsize=None)
def reference(name, K=None):
    P = problem(name)
    return T.tolerances(P, P["K"] if K is None else K, P["nu"])


def device(name, reuse=True, keep_kuf=True):
    from gaussianprocessnode_amd import SGPDevice
    from gaussianprocessnode_amd.meta import set_engine_kernel
    P = problem(name)
    d = SGPDevice(P["N"], P["M"], P["D"], reuse_stats=reuse, keep_kuf=keep_kuf)
    d.set_inducing(P["Xu"])
    set_engine_kernel(d, P["s2"], P["ell"], P["jitter"], P["family"])
    if P["prior"][0] == "iso":
        d.set_prior_isotropic(P["prior"][1])
    elif P["prior"][0] == "meancov":
        d.set_prior_meancov(P["prior"][1], P["prior"][2])
    else:
        d.set_prior_precision(P["prior"][1], P["prior"][2])
    d.set_data(P["X"], P["y"])
    if P["hold"]:
        d.set_noise([[P["hold"][0]]], P["hold"][1])
    return d, P


def run(d, P, K, **kw):
    return d.vmp_run_t(K, P["nu"], gamma_prior=None if P["hold"] else P["g0"], hold_w=P["hold"] is not None, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(name):
    rk, tol = reference(name)
    d, P = device(name)
    with d:
        values, terms, gamma, beta, done, conv = run(d, P, P["K"])
        mu, Sigma, _ = d.posterior(want_uv=False)
    assert done == P["K"] and not conv
    ratios = dict(values=np.abs(values - rk["values"]).max() / tol["values"], mu=np.abs(mu - rk["mu"]).max() / tol["mu"],
                  Sigma=np.abs(Sigma - rk["Sigma"]).max() / tol["Sigma"],
                  tau_rate=np.abs(beta - rk["tau_rate"]).max() / tol["tau_rate"])
    for j in range(4):                                        # (a term that is exactly 0 in the restatement -- q(w) held -- is 0)
        err, t = np.abs(terms[:, j] - rk["terms"][:, j]).max(), tol["terms"][j]
        ratios[f"terms{j}"] = err / t if t > 0 else (np.inf if err > 0 else 0.0)
    if gamma is not None:
        assert gamma[0] == rk["gamma"][0]
        ratios["rate"] = abs(gamma[1] - rk["gamma"][1]) / tol["gamma"]
    print(f"vmp_run_t {name} K={P['K']} error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the values do not increase, within the restatement's own rounding floor
    assert np.all(np.diff(values) <= tol["values"]), np.diff(values)


def host_loop(d, P, K, displace_w=0.0):
    """train.vmp_regression's host-paced Student-t loop on a prepared handle, with E[log w] passed on and, optionally, mean(q_w)
    displaced relatively at every iteration; leaves the handle behind the last sweep with the noise set to the new mean(q_w)"""
    from scipy.special import digamma
    alpha, hn = 0.5 * (P["nu"] + 1.0), 0.5 * P["nu"]
    a, b = PRIOR_G
    beta = np.full(P["N"], alpha)
    for _ in range(K):
        d.set_data(P["X"], P["y"], weights=alpha / beta)
        d.set_noise([[a / b * (1.0 + displace_w)]], float(digamma(a) - np.log(b)))
        d.sweep()
        sc = d.scalars()
        a, b = PRIOR_G[0] + 0.5 * P["N"], PRIOR_G[1] + 0.5 * (sc.sum_I1 + sc.sum_I2)
        I1, I2 = d.w_stats()
        beta = hn + 0.5 * (a / b) * (I1 + I2)
    d.set_noise([[a / b]], float(digamma(a) - np.log(b)))
    return (a, b), beta


def state_of(d, P):
    sc = d.scalars()
    mu, Sigma, Uv = d.posterior()
    I1, I2 = d.w_stats()
    pm, pv = d.predict_var(P["X"][:5], noise=True)
    Psi2, B, scal = d.stats()
    return dict(sums=np.array([sc.sum_I1, sc.sum_I2, sc.logdet_kuu, sc.logdet_lambda]), mu=mu, Sigma=Sigma, Uv=Uv, I1=I1, I2=I2,
                pred_mean=pm, pred_var=pv, Psi2=Psi2, B=B, scal=scal)


def test_against_the_host_paced_loop():
    """(300, 65, 2, 4): the device-paced run against train.vmp_regression(student_t=nu, device_paced=False) -- set_data(weights=),
    sweep, w_stats, get_scalars -- whose full sweeps may sum in another order: by the rule of the existing host-paced comparison, 10 x
    the change of that loop's results when mean(q_w) is displaced by 4 ulp at every iteration.  The free-energy traces of both paths
    are held to the restatement."""
    from gaussianprocessnode_amd import train
    name = "tiles"
    P = problem(name)
    ref, tol = reference(name)
    theta = np.concatenate([[P["s2"]], P["ell"]])
    kw = dict(iterations=P["K"], prior_var=50.0, shape=PRIOR_G[0], rate=PRIOR_G[1], jitter=P["jitter"], student_t=P["nu"], free_energy=True)
    outs = []
    for paced in (False, True):
        d, _ = device(name)
        with d:
            q, g, beta, trace = train.vmp_regression(theta, P["X"], P["y"], P["Xu"], d, device_paced=paced, **kw)
            outs.append((q.m, q.S, g, beta, state_of(d, P), d.sweep_kind()))
        ratio = np.abs(trace - ref["values"]).max() / tol["values"]
        print(f"vmp_run_t {name} free-energy trace, device_paced={paced}: error/tolerance {ratio:.3g}")
        assert ratio <= 1.0
    seq = []
    for disp in (0.0, 4 * EPS):
        h, _ = device(name)
        with h:
            g, beta = host_loop(h, P, P["K"], disp)
            seq.append((g, beta, state_of(h, P)))
    (mh, Sh, gh, bh, sth, _), (md, Sd, gd, bd, std, kinds) = outs
    assert kinds[1] == 3                                      # SGP_SWEEP_REWEIGHTED
    assert gd[0] == gh[0] and abs(gd[1] - gh[1]) <= 10 * abs(seq[1][0][1] - seq[0][0][1])
    assert np.abs(bd - bh).max() <= 10 * np.abs(seq[1][1] - seq[0][1]).max()
    for q in std:
        t = 10 * np.abs(seq[1][2][q] - seq[0][2][q]).max()
        err = np.abs(std[q] - seq[0][2][q]).max()
        print(f"vmp_run_t {name} state {q}: error/tolerance {err / t if t > 0 else float(err > 0):.3g}")
        # asserted: what the existing comparison holds, q(v)'s mean and covariance.  The other figures are printed only: the host
        # loop's full sweeps sum Psi2 in another order, which a displaced w does not probe (sums and Uv come out at 1 - 2).
        if q in ("mu", "Sigma"):
            assert err <= t, (q, err, t)


def test_large_nu_is_the_gaussian_run():
    """nu = 1e8 against sgp_vmp_run Gaussian on the same data, within the difference the float64 restatements of the two models show
    (plus both runs' own tolerances)"""
    from tests.test_gpu_vmp_run import tolerances as gaussian_tolerances
    name = "nu1e8"
    P = problem(name)
    rt, tol_t = reference(name)
    rg, tol_g = gaussian_tolerances(P, P["K"], dict(gamma_prior=PRIOR_G))
    d, _ = device(name)
    with d:
        _, _, gt, _, _, _ = run(d, P, P["K"])
        mt = d.posterior(want_cov=False, want_uv=False)[0]
    d, _ = device(name)
    with d:
        _, _, gg, _, _ = d.vmp_run(P["K"], gamma_prior=PRIOR_G)
        mg = d.posterior(want_cov=False, want_uv=False)[0]
    model_mu, model_rate = np.abs(rt["mu"] - rg["mu"]).max(), abs(rt["gamma"][1] - rg["gamma"][1])
    print(f"vmp_run_t nu=1e8 vs Gaussian: mu {np.abs(mt - mg).max():.3g} (models differ by {model_mu:.3g}), "
          f"rate {abs(gt[1] - gg[1]):.3g} (models {model_rate:.3g})")
    assert np.abs(mt - mg).max() <= model_mu + tol_t["mu"] + tol_g["mu"]
    assert abs(gt[1] - gg[1]) <= model_rate + tol_t["gamma"] + tol_g["gamma"]


@pytest.mark.parametrize("name", ["tiles", "precision", "hold_w"])
def test_bitwise_repeat_and_continuation(name):
    outs = []
    for _ in range(2):
        d, P = device(name)
        with d:
            v, t, g, beta, _, _ = run(d, P, 5)
            outs.append((v, t, g if g is not None else np.zeros(2), beta, *d.posterior(want_uv=False)[:2], *d.stats()))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    d, P = device(name)
    with d:
        v1, t1, g1, b1, _, _ = run(d, P, 2)
        v2, t2, g2, b2, _, _ = run(d, P, 3, gamma=g1, tau_rate=b1)
        mu, Sigma = d.posterior(want_uv=False)[:2]
        st = d.stats()
    assert np.array_equal(np.concatenate([v1, v2]), outs[0][0]) and np.array_equal(np.vstack([t1, t2]), outs[0][1])
    assert np.array_equal(g2 if g2 is not None else np.zeros(2), outs[0][2]) and np.array_equal(b2, outs[0][3])
    assert np.array_equal(mu, outs[0][4]) and np.array_equal(Sigma, outs[0][5])
    assert all(np.array_equal(x, y) for x, y in zip(st, outs[0][6:]))


def test_null_tau_rate_starts_from_unit_weights():
    d, P = device("wg257")
    with d:
        v, _, g, beta, _, _ = run(d, P, 2)
    d, P = device("wg257")
    with d:
        g0, g1 = (C.c_double * 2)(*PRIOR_G), (C.c_double * 2)(*PRIOR_G)
        vals = np.full(2, np.nan)
        rc = d._lib.sgp_vmp_run_t(d._h, P["nu"], None, 0, 2, g0, g1, 0.0, vals.ctypes.data_as(C.POINTER(C.c_double)), None, None)
        assert rc == 0 and np.array_equal(vals, v) and (g1[0], g1[1]) == (g[0], g[1])


def test_tol_stops_the_run():
    name = "tiles"
    ref, _ = reference(name, 7)
    v = ref["values"]
    dec = np.abs(np.diff(v)) / np.abs(v[1:])
    k = 3
    assert dec[k - 1] < dec[k - 2], "the trace does not separate the two decrements"
    tol = float(np.sqrt(dec[k - 1] * dec[k - 2]))
    d, P = device(name)
    with d:
        values, terms, gamma, beta, done, conv = run(d, P, 7, tol=tol)
        st, kinds = state_of(d, P), d.sweep_kind()
    assert (done, conv) == (k + 1, True) and np.isnan(values[k + 1:]).all() and np.isfinite(values[:k + 1]).all()
    d, P = device(name)
    with d:
        v2, _, g2, b2, _, _ = run(d, P, k + 1)
        st2 = state_of(d, P)
    # the rates and q(w) are those iteration k formed; the weights, the statistics and q(v) those of sweep k
    assert np.array_equal(values[:k + 1], v2) and np.array_equal(gamma, g2) and np.array_equal(beta, b2)
    assert all(np.array_equal(st[q], st2[q]) for q in st) and kinds[1] == 3


def test_failure_stop_and_recovery():
    """the `toy` problem of tests/test_gpu_vmp_run.py: two coincident inducing inputs and no jitter, K_uu fails at minor 6"""
    from gaussianprocessnode_amd import SGPDevice
    from tests.test_gpu_vmp_run import problem as gaussian_problem
    P = gaussian_problem("toy")
    Xu = P["Xu"].copy()
    Xu[5] = Xu[2]
    beta0 = np.linspace(1.0, 3.0, P["N"])
    with SGPDevice(P["N"], P["M"], P["D"], reuse_stats=True, keep_kuf=True) as d:
        d.set_inducing(Xu)
        d.set_kernel(P["s2"], P["ell"], 0.0)
        d.set_prior_isotropic(50.0)
        d.set_data(P["X"], P["y"])
        with pytest.raises(np.linalg.LinAlgError) as e:
            d.vmp_run_t(4, 4.0, gamma_prior=PRIOR_G, tau_rate=beta0)
        assert e.value.minor == 6 and e.value.iterations_done == 0 and np.isnan(e.value.values).all()
        assert np.array_equal(e.value.gamma, PRIOR_G) and np.array_equal(e.value.tau_rate, beta0)
        assert e.value.counts == (0, -6)
        d.set_inducing(P["Xu"])
        d.set_kernel(P["s2"], P["ell"], P["jitter"])
        values, _, _, _, done, _ = d.vmp_run_t(2, 4.0, gamma_prior=PRIOR_G)          # (the weights the failed run left are its own)
        assert done == 2 and np.isfinite(values).all()


@pytest.mark.parametrize("reuse", [True, False])
def test_state_afterwards(reuse):
    """sgp_sweep_kind, the getters, the resident weights, and a following sgp_sweep (over the resident statistics on a REUSE_STATS
    handle, a full one otherwise: both must reproduce the last iteration's q(v) from the weights the run left)"""
    from scipy.special import digamma
    from gaussianprocessnode_amd import _lib
    name = "tiles"
    rk, tol = reference(name)
    d, P = device(name, reuse=reuse)
    with d:
        assert run(d, P, 1)[4] == 1 and d.sweep_kind()[1] == _lib.SGP_SWEEP_FULL
    d, P = device(name, reuse=reuse)
    with d:
        _, _, gamma, beta, done, _ = run(d, P, P["K"])
        nxt, last = d.sweep_kind()
        assert last == _lib.SGP_SWEEP_REWEIGHTED == 3 and nxt == (_lib.SGP_SWEEP_REUSED if reuse else _lib.SGP_SWEEP_FULL)
        before = state_of(d, P)
        sc = d.scalars()
        assert np.array_equal(gamma, [PRIOR_G[0] + P["N"] / 2, PRIOR_G[1] + 0.5 * (sc.sum_I1 + sc.sum_I2)])
        # the data scalars are the last sweep's weights': S_YY = sum omega y^2, S_W = sum omega, S_N = N
        assert abs(before["scal"][1] - rk["omega"].sum()) <= 10 * P["N"] * np.abs(rk["omega"]).max() * (tol["tau_rate"] / rk["tau_rate"].min() + EPS)
        assert before["scal"][2] == P["N"]
        # the noise in force is mean(q(w))
        noise = d.predict_var(P["X"][:3], noise=True)[1] - d.predict_var(P["X"][:3])[1]
        assert np.allclose(noise, gamma[1] / gamma[0], rtol=1e-9, atol=0)
        # the last sweep again, at the noise that entered it: q(v) comes back
        g_in = run_prefix_gamma(name, reuse, P["K"] - 1)
        d.set_noise([[g_in[0] / g_in[1]]], float(digamma(g_in[0]) - np.log(g_in[1])))
        d.sweep()
        assert d.sweep_kind()[1] == (_lib.SGP_SWEEP_REUSED if reuse else _lib.SGP_SWEEP_FULL)
        again = state_of(d, P)
    for q in ("mu", "Sigma", "Psi2", "B", "scal"):
        t = tol[q] if q in tol else 0.0
        err = np.abs(again[q] - before[q]).max()
        # REUSED: phase 2 over the statistics the run left, in another column layout at most; FULL: Psi2 and B again from the weights
        bound = 10 * t if t else 1e3 * EPS * np.abs(before[q]).max()
        assert err <= bound, (q, err, bound)


@functools.lru_cache(maxsize=None)
def run_prefix_gamma(name, reuse, k):
    d, P = device(name, reuse=reuse)
    with d:
        return tuple(run(d, P, k)[2])


def test_the_robust_mean_is_closer_at_the_clean_points():
    name = "outliers"
    P = problem(name)
    d, _ = device(name)
    with d:
        _, _, _, beta, _, _ = run(d, P, 10)
        mt = d.predict(P["X"])
        omega = d_weights(P, beta)
    d, _ = device(name)
    with d:
        d.vmp_run(10, gamma_prior=PRIOR_G)
        mg = d.predict(P["X"])
    clean, f = P["clean"], P["f"]
    err_t, err_g = np.sqrt(np.mean((mt - f)[clean] ** 2)), np.sqrt(np.mean((mg - f)[clean] ** 2))
    print(f"vmp_run_t outliers: rms error at the clean points {err_t:.4g} (Student-t) vs {err_g:.4g} (Gaussian); "
          f"weights of the displaced targets <= {omega[~clean].max():.3g}, of the clean >= {omega[clean].min():.3g}")
    assert err_t < 0.5 * err_g
    assert omega[~clean].max() < 0.1 * omega[clean].min()


def d_weights(P, beta):
    return 0.5 * (P["nu"] + 1.0) / beta


def test_refusals():
    from gaussianprocessnode_amd import SGPDevice, SGPError
    P = problem("tiny")
    d, _ = device("tiny")
    with d:
        d.sweep()
        before = (d.scalars(), d.posterior(), d.sweep_kind(), d.stats())

        def unchanged():
            after = (d.scalars(), d.posterior(), d.sweep_kind(), d.stats())
            assert before[0] == after[0] and before[2] == after[2]
            assert all(np.array_equal(x, y) for x, y in zip(before[1] + before[3], after[1] + after[3]))

        n = P["N"]
        bad = [(dict(nu=0.0, gamma_prior=PRIOR_G), "nu must be positive"),
               (dict(nu=-1.0, gamma_prior=PRIOR_G), "nu must be positive"),
               (dict(nu=np.inf, gamma_prior=PRIOR_G), "nu must be positive"),
               (dict(nu=np.nan, gamma_prior=PRIOR_G), "nu must be positive"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, tau_rate=np.array([1.0, 0.0, 1.0])), "tau_rate must be positive"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, tau_rate=np.array([1.0, 1.0, np.nan])), "tau_rate must be positive"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, tau_rate=np.array([np.inf, 1.0, 1.0])), "tau_rate must be positive"),
               (dict(nu=4.0, gamma_prior=(0.0, 1.0)), "gamma_prior must be positive"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, gamma=(1.0, np.inf)), "gamma must be positive"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, tol=-1.0), "tol must be >= 0"),
               (dict(nu=4.0, gamma_prior=PRIOR_G, tol=np.nan), "tol must be >= 0")]
        for K in (0, 3):
            for kw, text in bad:
                kw = dict(kw)
                with pytest.raises(SGPError, match=text):
                    d.vmp_run_t(K, kw.pop("nu"), **kw)
        with pytest.raises(SGPError, match="iterations must be >= 0"):
            d.vmp_run_t(-1, 4.0, gamma_prior=PRIOR_G)
        rc = d._lib.sgp_vmp_run_t(d._h, 4.0, None, 2, 1, None, None, 0.0, None, None, None)
        assert rc == -1 and b"unknown flags" in d._lib.sgp_last_error(d._h)
        two = (C.c_double * 2)(1.0, 1.0)
        for g0, g in ((None, two), (two, None), (None, None)):
            rc = d._lib.sgp_vmp_run_t(d._h, 4.0, None, 0, 1, g0, g, 0.0, None, None, None)
            assert rc == -1 and b"gamma_prior and gamma are required" in d._lib.sgp_last_error(d._h)
        unchanged()
        d.set_allreduce(lambda buf, count, stream: None)
        for K in (0, 1):
            with pytest.raises(SGPError, match="data-sharded"):
                d.vmp_run_t(K, 4.0, gamma_prior=PRIOR_G)
        d.set_allreduce(None)
        for data, text in (((P["X"], P["y"], np.ones(n)), "without y_var"), ((P["X"], P["y"], None, np.full(n, 0.5)), "caller's pt_weight")):
            d.set_data(*data)
            d.sweep()
            st = d.stats()
            for K in (0, 1):
                with pytest.raises(SGPError, match=text):
                    d.vmp_run_t(K, 4.0, gamma_prior=PRIOR_G)
            assert all(np.array_equal(x, y) for x, y in zip(st, d.stats()))           # (a caller's cubature weights are not overwritten)
            d.sweep()
            assert all(np.array_equal(x, y) for x, y in zip(st, d.stats()))
        d.sweep_local_psi(P["X"][:2], None, P["y"][:2])
        for K in (0, 1):
            with pytest.raises(SGPError, match="exact Psi-statistics"):
                d.vmp_run_t(K, 4.0, gamma_prior=PRIOR_G)
        d.set_data(P["X"], P["y"])
        out = d.vmp_run_t(0, 4.0, gamma_prior=PRIOR_G)
        assert out[4] == 0 and out[0].size == 0
        d.train_begin(P["X"], P["y"], np.zeros(2))
        for K in (0, 1):
            with pytest.raises(SGPError, match="training run is open"):
                d.vmp_run_t(K, 4.0, gamma_prior=PRIOR_G)
        d.train_end()
        # weights an earlier run left are continued, and sgp_vmp_run still refuses them
        d.set_data(P["X"], P["y"])
        d.vmp_run_t(1, 4.0, gamma_prior=PRIOR_G)
        assert d.vmp_run_t(1, 4.0, gamma_prior=PRIOR_G)[4] == 1
        with pytest.raises(SGPError, match="without pt_weight"):
            d.vmp_run(1, gamma_prior=PRIOR_G)
    d, _ = device("tiny", keep_kuf=False)
    with d:
        for K in (0, 1):
            with pytest.raises(SGPError, match="SGP_FLAG_KEEP_KUF"):
                d.vmp_run_t(K, 4.0, gamma_prior=PRIOR_G)
    with SGPDevice(10, 4, 1, keep_kuf=True) as e:
        with pytest.raises(SGPError, match="set_inducing, set_kernel and set_data"):
            e.vmp_run_t(1, 4.0, gamma_prior=PRIOR_G)
    with SGPDevice(10, 4, 1, d_out=2, keep_kuf=True) as e:
        with pytest.raises(SGPError, match="UniSGP handles only"):
            e.vmp_run_t(1, 4.0, gamma_prior=PRIOR_G)
