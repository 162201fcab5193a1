"""sgp_vmp_run on the GPU against tests/vmp_ref.py, against the host-paced loop on the same library, bitwise repeatability and
splitting, the tol stop, the failure stop, the state it leaves and every refusal.

Tolerances: per quantity 10 x the larger of the restatement's float64-vs-extended difference and its change when Psi2, B and w are
displaced relatively by 50 eps at every iteration (the rule of tests/test_gpu_gpssm.py); none is taken from the code under test."""
import functools

import numpy as np
import pytest

from tests import vmp_ref as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PRIOR_G = (1e-2, 1e-2)

# name -> (N, M, D, likelihood, family, prior form, hold_w)
CASES = {
    "toy": (50, 20, 1, "gaussian", "se", "iso", False),
    "ard": (300, 70, 3, "gaussian", "se", "iso", False),
    "tiles": (1025, 130, 2, "gaussian", "se", "iso", False),
    "probit255": (255, 20, 1, "probit", "se", "iso", False),
    "probit256": (256, 20, 2, "probit", "se", "iso", False),
    "probit257": (257, 70, 3, "probit", "se", "iso", False),
    "probit1025": (1025, 130, 2, "probit", "se", "iso", False),
    "matern52": (300, 70, 3, "gaussian", "matern52", "iso", False),
    "meancov": (300, 70, 3, "gaussian", "se", "meancov", False),
    "precision": (300, 70, 3, "probit", "se", "precision", False),
    "hold_w": (300, 70, 3, "gaussian", "se", "iso", True),
    "hold_w_probit": (257, 20, 1, "probit", "se", "iso", True),
}
DMAX = 32                                                    # the largest input dimension a handle accepts (include/sgp_hip.h)
# The branch points of k_vmp_kl, k_vmp_close, digamma_dev and the family / dimension dispatch inside the call.  These cases share
# one toy seed and the lengthscale 0.5 sqrt(D) in every dimension: cond(K_uu + jitter I) < 1e8 (tests/test_vmp_host.py asserts it).
BRANCH_CASES = {
    "kl_iso_257": (320, 257, 2, "gaussian", "se", "iso", False),        # isotropic prior: two workgroups, the second with one entry
    "kl_dense_300": (320, 300, 2, "probit", "se", "precision", False),  # dense: second row pass, column wrap, ld != Q, > 4 tile steps
    "kl_meancov_257": (300, 257, 2, "gaussian", "se", "meancov", False),    # the same through form 0, stored as a precision
    "reduce_65537": (65537, 20, 1, "probit", "se", "iso", False),       # 257 pairs: the reduce stage's second pass, with one pair
    "n1": (1, 4, 1, "gaussian", "se", "iso", False),                    # one factor node: a = a0 + 1/2
    "n3_tiny_shape": (3, 2, 1, "gaussian", "se", "iso", False),         # shape0 = 1e-6: lgamma(a0) at its pole, nine recurrence steps
    "n19": (19, 8, 1, "probit", "se", "iso", False),                    # closing stage: one recurrence step of digamma (a = 9.51)
    "n20": (20, 8, 1, "probit", "se", "iso", False),                    # closing stage: none (a = 10.01)
    "matern12_probit": (257, 70, 3, "probit", "matern12", "iso", False),
    "matern32_probit": (257, 70, 3, "probit", "matern32", "iso", False),
    "d5": (300, 70, 5, "gaussian", "se", "iso", False),
    "dmax": (300, 70, DMAX, "probit", "se", "iso", False),
}
CASES.update(BRANCH_CASES)
BRANCH_SEED = 11
ITERATIONS = {"reduce_65537": (1, 2)}                        # (its extended-precision restatement is the longest host-side reference)
PRIOR_G_OF = {"n3_tiny_shape": (1e-6, 1e-6)}
HOLD = (3.0, float(np.log(3.0)))


@functools.lru_cache(maxsize=None)
def problem(name):
    N, M, D, lik, family, form, hold = CASES[name]
    branch = name in BRANCH_CASES
    X, y, Xu = R.make_toy(N, min(M, N), D, seed=BRANCH_SEED if branch else sum(map(ord, name)), probit=lik == "probit")
    if M > N:                                                # fewer points than inducing inputs: the rest drawn from the same box
        Xu = np.concatenate([Xu, np.random.default_rng(BRANCH_SEED + 1).uniform(-1.7, 1.7, (M - N, D))])
    rng = np.random.default_rng(7)
    ell = np.array([1.2, 0.9, 1.5])[:D] if D > 1 else np.array([0.8])
    if branch:
        ell = np.full(D, 0.5 * np.sqrt(D))
    if form == "iso":
        prior = ("iso", 50.0)
    else:
        A = rng.normal(size=(M, M)) / np.sqrt(M)
        S0 = 2.0 * np.eye(M) + A @ A.T                       # non-diagonal
        m0 = 0.3 * rng.normal(size=M)
        prior = ("meancov", m0, S0) if form == "meancov" else ("precision", np.linalg.solve(S0, m0), np.linalg.inv(S0))
    return dict(X=X, y=y, Xu=Xu, s2=0.8, ell=ell, jitter=1e-6, prior=prior, lik=lik, family=family, hold=HOLD if hold else None, M=M,
                N=N, D=D, g0=PRIOR_G_OF.get(name, PRIOR_G))


@functools.lru_cache(maxsize=None)
def reference(name, K=7):
    """(float64 run, per-quantity tolerance) -- computed once per case and shared"""
    P = problem(name)
    return tolerances(P, K, dict(likelihood=P["lik"], gamma_prior=P["g0"], hold_w=P["hold"], family=P["family"]))


def tolerances(P, K, kw):
    """the float64 restatement of a K-iteration run and the tolerance rule of this file"""
    args = (P["X"], P["y"], P["Xu"], P["s2"], P["ell"], P["jitter"], P["prior"], K)
    ref = R.vmp_run_ref(*args, **kw)
    if R.mpmath is None:
        print("vmp_ref: mpmath is missing -- psi, lgamma and log Phi of the extended run are SciPy's float64 ones")
    ext = R.vmp_run_ref(*args, dtype=np.longdouble, **kw)
    dis = R.vmp_run_ref(*args, displace=50 * EPS, **kw)
    tol = {}
    for q in ("values", "terms", "mu", "Sigma"):
        worst = np.maximum(np.abs(np.asarray(ext[q], dtype=np.float64) - ref[q]), np.abs(dis[q] - ref[q]))
        tol[q] = 10 * (worst.max(axis=0) if q == "terms" else worst.max())
    tol["gamma"] = 10 * max(abs(float(ext["gamma"][1]) - ref["gamma"][1]), abs(dis["gamma"][1] - ref["gamma"][1]))
    return ref, tol


def device(name, reuse=True):
    from gaussianprocessnode_amd import SGPDevice
    from gaussianprocessnode_amd.meta import set_engine_kernel
    P = problem(name)
    d = SGPDevice(P["N"], P["M"], P["D"], reuse_stats=reuse)
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
    return d.vmp_run(K, likelihood=P["lik"], gamma_prior=None if P["hold"] else P["g0"], hold_w=P["hold"] is not None, **kw)


def host_loop(d, P, K, displace_w=0.0):
    """The host-paced loop of train.vmp_regression / vmp_classification on a prepared handle (isotropic prior cases), with E[log w] of
    the Gamma q(w) passed on and, optionally, mean(q_w) displaced relatively at every iteration.  Leaves the handle behind the last
    sweep with the noise set to the new mean(q_w) -- the sequence sgp_vmp_run is documented to equal.  Returns the final (a, b)."""
    from scipy.special import digamma
    from gaussianprocessnode_amd import train
    a, b = PRIOR_G
    mu = np.zeros(P["M"])
    for k in range(K):
        w = a / b * (1.0 + displace_w)
        if P["lik"] == "probit":
            mf, vf = train.probit_marginal(P["y"], d.predict(P["X"], mu), 1.0 / w)
            d.set_targets(mf, vf) if k else d.set_data(P["X"], mf, vf)
        d.set_noise([[w]], float(digamma(a) - np.log(b)))
        d.sweep()
        sc = d.scalars()
        a, b = PRIOR_G[0] + 0.5 * P["N"], PRIOR_G[1] + 0.5 * (sc.sum_I1 + sc.sum_I2)
        mu = d.posterior(want_cov=False, want_uv=False)[0]
    d.set_noise([[a / b]], float(digamma(a) - np.log(b)))
    return a, b


def state_of(d, P):
    """what check 6 compares: the scalars the sweep left, q(v), the theta objective with its gradient, the predictive variance"""
    sc = d.scalars()
    mu, Sigma, Uv = d.posterior()
    val, grad = d.theta_objective(want_grad=True, n_ell=len(P["ell"]))
    pm, pv = d.predict_var(P["X"][:5], noise=True)
    return dict(sums=np.array([sc.sum_I1, sc.sum_I2, sc.logdet_kuu, sc.logdet_lambda]), mu=mu, Sigma=Sigma, Uv=Uv,
                objective=np.concatenate([[val], grad]), pred_mean=pm, pred_var=pv)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(name):
    for K in ITERATIONS.get(name, (1, 2, 7)):
        rk, tol = reference(name, K)                          # the tolerance of a K-iteration run comes from a K-iteration reference
        d, P = device(name)
        with d:
            values, terms, gamma, done, conv = run(d, P, K)
            mu, Sigma, _ = d.posterior(want_uv=False)
        assert done == K and not conv
        ratios = dict(values=np.abs(values - rk["values"]).max() / tol["values"],
                      mu=np.abs(mu - rk["mu"]).max() / tol["mu"], Sigma=np.abs(Sigma - rk["Sigma"]).max() / tol["Sigma"])
        for j in range(4):                                    # (a term that is exactly 0 in the restatement -- no Probit factors, q(w) held -- is 0)
            err, t = np.abs(terms[:, j] - rk["terms"][:, j]).max(), tol["terms"][j]
            if t == 0 and np.any(rk["terms"][:, j] != 0):
                # both measures of the rule round to 0 (n1, K = 1: KL(q(w)) of one factor node): the float64 restatement is itself
                # defined to half an ulp only, and that is the smallest difference from the extended run the rule can read
                t = 10 * 0.5 * np.spacing(np.abs(rk["terms"][:, j]).max())
            ratios[f"terms{j}"] = err / t if t > 0 else (np.inf if err > 0 else 0.0)
        if gamma is not None:
            assert gamma[0] == rk["gamma"][0]
            ratios["rate"] = abs(gamma[1] - rk["gamma"][1]) / tol["gamma"]
        print(f"vmp_run {name} K={K} error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios


TAILS = (300, 20, 1)                                         # N, M, D of the tails problem
TAILS_GAMMA = (30.0, 10.0)                                   # q(w) on entry: vz = 1 / 3


@functools.lru_cache(maxsize=None)
def tails_problem(c):
    """Probit at mu_init = c sign(K_uf (1 - 2 y)): the first forward means point away from the labels, g down to -46 (c = 10) and
    -460 (c = 100) and up to +25 and +250 -- the erfcx branch of log Phi and of phi / Phi, and the cancellation in vf"""
    N, M, D = TAILS
    X, y, Xu = R.make_toy(N, M, D, seed=3, probit=True)
    ell = np.array([0.8])
    mu_init = c * np.sign(R.kernel(Xu, X, 0.8, ell) @ (1.0 - 2.0 * y))
    P = dict(X=X, y=y, Xu=Xu, s2=0.8, ell=ell, jitter=1e-6, prior=("iso", 50.0), lik="probit", family="se", hold=None, M=M, N=N, D=D,
             g0=PRIOR_G, mu_init=mu_init)
    g = (2.0 * y - 1.0) * (R.kernel(Xu, X, 0.8, ell).T @ mu_init) / np.sqrt(1.0 + TAILS_GAMMA[1] / TAILS_GAMMA[0])
    return P, g


@functools.lru_cache(maxsize=None)
def tails_reference(c, K=2):
    P, _ = tails_problem(c)
    return tolerances(P, K, dict(likelihood="probit", gamma_prior=PRIOR_G, gamma=TAILS_GAMMA, mu_init=P["mu_init"]))


@pytest.mark.parametrize("c", [10, 100])
def test_probit_tails_through_mu_init(c):
    from gaussianprocessnode_amd import SGPDevice
    P, g = tails_problem(c)
    assert g.min() < -4.5 * c and g.max() > 2.4 * c            # both tails are reached
    rk, tol = tails_reference(c)
    with SGPDevice(P["N"], P["M"], P["D"], reuse_stats=True) as d:
        d.set_inducing(P["Xu"])
        d.set_kernel(P["s2"], P["ell"], P["jitter"])
        d.set_prior_isotropic(P["prior"][1])
        d.set_data(P["X"], P["y"])
        values, terms, gamma, done, conv = d.vmp_run(2, likelihood="probit", gamma_prior=PRIOR_G, gamma=TAILS_GAMMA, mu_init=P["mu_init"])
        mu, Sigma, _ = d.posterior(want_uv=False)
    assert done == 2 and not conv
    assert all(np.isfinite(x).all() for x in (values, terms, gamma, mu, Sigma))
    assert 0.5 < terms[0, 1] / (1.4e5 * (c / 10) ** 2) < 2.0    # the Probit term grows with g^2 / 2
    ratios = dict(values=np.abs(values - rk["values"]).max() / tol["values"],
                  mu=np.abs(mu - rk["mu"]).max() / tol["mu"], Sigma=np.abs(Sigma - rk["Sigma"]).max() / tol["Sigma"])
    for j in range(4):
        ratios[f"terms{j}"] = np.abs(terms[:, j] - rk["terms"][:, j]).max() / tol["terms"][j]
    assert gamma[0] == rk["gamma"][0]
    ratios["rate"] = abs(gamma[1] - rk["gamma"][1]) / tol["gamma"]
    print(f"vmp_run tails c={c} g in [{g.min():.4g}, {g.max():.4g}] relative tolerance of the values {tol['values'] / np.abs(rk['values']).max():.3g}"
          " error/tolerance: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("name", ["ard", "probit257"])
def test_against_the_host_paced_loop(name):
    from gaussianprocessnode_amd import train
    P = problem(name)
    d, _ = device(name)
    with d:
        fn = train.vmp_classification if P["lik"] == "probit" else train.vmp_regression
        kw = dict(iterations=7, prior_var=50.0, shape=PRIOR_G[0], rate=PRIOR_G[1], jitter=P["jitter"], family=P["family"])
        theta = np.concatenate([[P["s2"]], P["ell"]])
        qh, gh = fn(theta, P["X"], P["y"], P["Xu"], d, **kw)
        qd, gd = fn(theta, P["X"], P["y"], P["Xu"], d, device_paced=True, **kw)
    # the tolerance: the change of that loop's results when mean(q_w) is displaced by 4 ulp at every one of its iterations
    runs = []
    for disp in (0.0, 4 * EPS):
        h, _ = device(name)
        with h:
            g = host_loop(h, P, 7, disp)
            m, S = h.posterior(want_uv=False)[:2]
        runs.append((m, S, g))
    assert np.abs(qd.m - qh.m).max() <= 10 * np.abs(runs[1][0] - runs[0][0]).max()
    assert np.abs(qd.S - qh.S).max() <= 10 * np.abs(runs[1][1] - runs[0][1]).max()
    assert gd[0] == gh[0] and abs(gd[1] - gh[1]) <= 10 * abs(runs[1][2][1] - runs[0][2][1])


@pytest.mark.parametrize("name", ["ard", "probit257"])
def test_free_energy_traces_of_the_two_paths(name):
    """train.vmp_*(free_energy=True): the host-paced trace (the same formulas in NumPy) and the device-paced one are each within the
    restatement's tolerance of the restatement's values"""
    from gaussianprocessnode_amd import train
    P = problem(name)
    ref, tol = reference(name, 7)
    fn = train.vmp_classification if P["lik"] == "probit" else train.vmp_regression
    kw = dict(iterations=7, prior_var=50.0, shape=PRIOR_G[0], rate=PRIOR_G[1], jitter=P["jitter"], family=P["family"], free_energy=True)
    theta = np.concatenate([[P["s2"]], P["ell"]])
    for paced in (False, True):
        d, _ = device(name)
        with d:
            out = fn(theta, P["X"], P["y"], P["Xu"], d, device_paced=paced, **kw)
        assert len(out) == 3 and out[2].shape == (7,)
        ratio = np.abs(out[2] - ref["values"]).max() / tol["values"]
        print(f"vmp_run {name} free-energy trace, device_paced={paced}: error/tolerance {ratio:.3g}")
        assert ratio <= 1.0


@pytest.mark.parametrize("name", ["toy", "probit257", "precision"])
def test_bitwise_repeat_and_split(name):
    outs = []
    for _ in range(2):
        d, P = device(name)
        with d:
            v, t, g, _, _ = run(d, P, 7)
            outs.append((v, t, g, *d.posterior(want_uv=False)[:2]))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    d, P = device(name)
    with d:
        v1, t1, g1, _, _ = run(d, P, 3)
        mu1 = d.posterior(want_cov=False, want_uv=False)[0]
        if P["lik"] == "probit":
            d.set_data(P["X"], P["y"])                        # the resident targets are q(f) now: the labels again
        v2, t2, g2, _, _ = run(d, P, 4, gamma=g1, mu_init=mu1)
        mu, Sigma = d.posterior(want_uv=False)[:2]
    assert np.array_equal(np.concatenate([v1, v2]), outs[0][0]) and np.array_equal(np.vstack([t1, t2]), outs[0][1])
    assert np.array_equal(g2, outs[0][2]) and np.array_equal(mu, outs[0][3]) and np.array_equal(Sigma, outs[0][4])


@pytest.mark.parametrize("name", ["ard", "probit257"])
def test_tol_stops_the_run(name):
    ref, _ = reference(name)
    v = ref["values"]
    dec = np.abs(np.diff(v)) / np.abs(v[1:])                  # dec[k - 1]: the relative decrement at iteration k
    k = 3
    assert dec[k - 1] < dec[k - 2], "the trace does not separate the two decrements"
    tol = float(np.sqrt(dec[k - 1] * dec[k - 2]))
    d, P = device(name)
    with d:
        values, terms, gamma, done, conv = run(d, P, 7, tol=tol)
        mu, Sigma = d.posterior(want_uv=False)[:2]
        noise = d.predict_var(P["X"][:3], noise=True)[1] - d.predict_var(P["X"][:3])[1]
    assert (done, conv) == (k + 1, True) and np.isnan(values[k + 1:]).all() and np.isfinite(values[:k + 1]).all()
    d, P = device(name)
    with d:
        v2, _, g2, _, _ = run(d, P, k + 1)
        mu2, Sigma2 = d.posterior(want_uv=False)[:2]
        noise2 = d.predict_var(P["X"][:3], noise=True)[1] - d.predict_var(P["X"][:3])[1]
    assert np.array_equal(values[:k + 1], v2) and np.array_equal(gamma, g2)
    assert np.array_equal(mu, mu2) and np.array_equal(Sigma, Sigma2) and np.array_equal(noise, noise2)


def test_failure_stop_and_recovery():
    from gaussianprocessnode_amd import SGPDevice
    P = problem("toy")
    Xu = P["Xu"].copy()
    Xu[5] = Xu[2]                                            # coincident inducing inputs, no jitter: K_uu fails at minor 6
    with SGPDevice(P["N"], P["M"], P["D"], reuse_stats=True) as d:
        d.set_inducing(Xu)
        d.set_kernel(P["s2"], P["ell"], 0.0)
        d.set_prior_isotropic(50.0)
        d.set_data(P["X"], P["y"])
        with pytest.raises(np.linalg.LinAlgError) as e:
            d.vmp_run(4, gamma_prior=PRIOR_G)
        assert e.value.minor == 6 and e.value.iterations_done == 0 and np.isnan(e.value.values).all()
        assert np.array_equal(e.value.gamma, PRIOR_G) and e.value.counts == (0, -6)
        d.set_inducing(P["Xu"])
        d.set_kernel(P["s2"], P["ell"], P["jitter"])         # (these twenty inducing inputs need the case's jitter)
        values, _, _, done, _ = d.vmp_run(2, gamma_prior=PRIOR_G)
        assert done == 2 and np.isfinite(values).all()


@pytest.mark.parametrize("name", ["ard", "probit257"])
def test_state_afterwards(name):
    from gaussianprocessnode_amd import _lib
    d, P = device(name)
    with d:
        _, _, gamma, _, _ = run(d, P, 3)
        kind_last = d.sweep_kind()[1]
        sc, post = d.scalars(), d.posterior()
        obj = d.theta_objective(want_grad=True, n_ell=len(P["ell"]))
        pv = d.predict_var(P["X"][:5], noise=True)
        assert kind_last == (_lib.SGP_SWEEP_TARGETS if P["lik"] == "probit" else _lib.SGP_SWEEP_REUSED)
        # the host-paced sequence on the same handle state: the last iteration's sweep again at the noise that entered it
        a, b = PRIOR_G[0] + P["N"] / 2, PRIOR_G[1] + 0.5 * (sc.sum_I1 + sc.sum_I2)
        assert np.array_equal(gamma, [a, b])
        d.set_data(P["X"], P["y"])
        d.set_noise([[1.0]])
        d.sweep()
        fresh = d.scalars()
    d2, _ = device(name)
    with d2:
        d2.set_noise([[1.0]])
        d2.sweep()
        assert d2.scalars() == fresh
    assert np.isfinite(obj[0]) and np.isfinite(pv[1]).all() and all(np.isfinite(x).all() for x in post)


def test_state_equals_the_host_paced_sequence():
    """Gaussian: the host-paced loop does the same sweeps at the same noise -- a / b is one IEEE division of the same (a, b), and
    b = rate0 + (sum I1 + sum I2) / 2 rounds once on either side (the halving is exact) -- so everything but E[log w] (another
    digamma) is the same arithmetic on the same kernels: q(v), q(w), the sums, the objective and the predictive variance agree
    bitwise with that loop followed by set_noise(mean(q_w)); the energy scalar, which carries E[log w] of the q(w) that entered the
    last iteration, within N / 2 times 4-ulp errors of psi(a) and log b."""
    from scipy.special import digamma
    name = "ard"
    d, P = device(name)
    with d:
        _, _, gamma, _, _ = run(d, P, 3)
        dev = (d.scalars(), d.posterior(), d.theta_objective(want_grad=True, n_ell=len(P["ell"])),
               d.predict_var(P["X"][:5], noise=True), d.sweep_kind())
    h, _ = device(name)
    with h:
        a, b = PRIOR_G                                         # train.vmp_regression's loop, with E[log w] of the Gamma q(w) passed on
        for _ in range(3):                                     # (that loop leaves it at set_noise's default, log mean(q_w))
            h.set_noise([[a / b]], float(digamma(a) - np.log(b)))
            h.sweep()
            sc = h.scalars()
            a_old, b_old = a, b
            a, b = PRIOR_G[0] + 0.5 * P["N"], PRIOR_G[1] + 0.5 * (sc.sum_I1 + sc.sum_I2)
        h.set_noise([[a / b]], float(digamma(a) - np.log(b)))
        host = (h.scalars(), h.posterior(), h.theta_objective(want_grad=True, n_ell=len(P["ell"])),
                h.predict_var(P["X"][:5], noise=True), h.sweep_kind())
    assert np.array_equal(gamma, [a, b])
    assert dev[0].sum_I1 == host[0].sum_I1 and dev[0].sum_I2 == host[0].sum_I2 and dev[0].logdet_lambda == host[0].logdet_lambda
    assert abs(dev[0].energy - host[0].energy) <= 0.5 * P["N"] * 8 * EPS * (abs(digamma(a_old)) + abs(np.log(b_old)))
    for x, y in zip(dev[1], host[1]):
        assert np.array_equal(x, y)
    assert dev[2][0] == host[2][0] and np.array_equal(dev[2][1], host[2][1])
    assert np.array_equal(dev[3][0], host[3][0]) and np.array_equal(dev[3][1], host[3][1])
    assert dev[4] == host[4]


@pytest.mark.parametrize("name", ["ard", "probit257", "kl_dense_300", "n19"])
def test_state_against_the_host_paced_sequence(name):
    """After the run the getters, the theta objective and the predictive variance are those of the host-paced sequence (set_data /
    set_targets(q(f)), set_noise, sweep per iteration, then set_noise(mean(q_w))) within 10 x their change when mean(q_w) is
    displaced by 4 ulp at every iteration of that sequence; sweep_kind agrees exactly.  Probit: the host forms q(f) in NumPy, so
    this also holds the targets, variances and data scalars the device wrote to those set_targets uploads."""
    P = problem(name)
    d, _ = device(name)
    with d:
        _, _, gamma, _, _ = run(d, P, 3)
        dev, kinds = state_of(d, P), d.sweep_kind()
    seq = []
    for disp in (0.0, 4 * EPS):
        h, _ = device(name)
        with h:
            g = host_loop(h, P, 3, disp)
            seq.append((state_of(h, P), h.sweep_kind(), g))
    assert kinds == seq[0][1]
    assert gamma[0] == seq[0][2][0] and abs(gamma[1] - seq[0][2][1]) <= 10 * abs(seq[1][2][1] - seq[0][2][1])
    for q in dev:
        tol = 10 * np.abs(seq[1][0][q] - seq[0][0][q]).max()
        err = np.abs(dev[q] - seq[0][0][q]).max()
        print(f"vmp_run {name} state {q}: error/tolerance {err / tol if tol > 0 else float(err > 0):.3g}")
        assert err <= tol, (q, err, tol)


@pytest.mark.parametrize("name", ["ard", "probit257"])
def test_handle_without_reuse_stats(name):
    """the same launches on a handle created without SGP_FLAG_REUSE_STATS: bitwise the flagged handle's results"""
    outs = []
    for reuse in (True, False):
        d, P = device(name, reuse=reuse)
        with d:
            v, t, g, done, _ = run(d, P, 4)
            outs.append((v, t, g, *d.posterior(want_uv=False)[:2]))
            assert done == 4
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_refusals():
    from gaussianprocessnode_amd import SGPDevice, SGPError
    P = problem("toy")
    d, _ = device("toy")
    with d:
        bad = [(dict(likelihood="gaussian", gamma_prior=(0.0, 1.0)), "gamma_prior must be positive"),
               (dict(gamma_prior=(1.0, np.nan)), "gamma_prior must be positive"),
               (dict(gamma_prior=PRIOR_G, gamma=(1.0, np.inf)), "gamma must be positive"),
               (dict(gamma_prior=PRIOR_G, gamma=(-1.0, 1.0)), "gamma must be positive"),
               (dict(gamma_prior=PRIOR_G, tol=-1.0), "tol must be >= 0"),
               (dict(gamma_prior=PRIOR_G, tol=np.nan), "tol must be >= 0"),
               (dict(gamma_prior=PRIOR_G, mu_init=np.full(P["M"], np.nan)), "mu_init must be finite"),
               (dict(gamma_prior=PRIOR_G, likelihood="probit"), "labels must be 0 or 1")]
        for K in (0, 3):
            for kw, text in bad:
                with pytest.raises(SGPError, match=text):
                    d.vmp_run(K, **kw)
        with pytest.raises(SGPError, match="iterations must be >= 0"):
            d.vmp_run(-1, gamma_prior=PRIOR_G)
        rc = d._lib.sgp_vmp_run(d._h, 2, 0, 1, None, None, None, 0.0, None, None, None)
        assert rc == -1 and b"unknown likelihood" in d._lib.sgp_last_error(d._h)
        rc = d._lib.sgp_vmp_run(d._h, 0, 2, 1, None, None, None, 0.0, None, None, None)
        assert rc == -1 and b"unknown flags" in d._lib.sgp_last_error(d._h)
        import ctypes as C
        two = (C.c_double * 2)(1.0, 1.0)
        for g0, g in ((None, two), (two, None), (None, None)):
            rc = d._lib.sgp_vmp_run(d._h, 0, 0, 1, g0, g, None, 0.0, None, None, None)
            assert rc == -1 and b"gamma_prior and gamma are required" in d._lib.sgp_last_error(d._h)
        d.set_allreduce(lambda buf, count, stream: None)
        with pytest.raises(SGPError, match="data-sharded"):
            d.vmp_run(1, gamma_prior=PRIOR_G)
        d.set_allreduce(None)
        d.set_data(P["X"], P["y"], np.ones(P["N"]))
        with pytest.raises(SGPError, match="without y_var"):
            d.vmp_run(1, gamma_prior=PRIOR_G)
        d.set_data(P["X"], P["y"], None, np.ones(P["N"]))
        with pytest.raises(SGPError, match="without pt_weight"):
            d.vmp_run(1, gamma_prior=PRIOR_G)
        d.sweep_local_psi(P["X"][:8], None, P["y"][:8])
        for K in (0, 1):
            with pytest.raises(SGPError, match="exact Psi-statistics"):
                d.vmp_run(K, gamma_prior=PRIOR_G)
        d.set_data(P["X"], P["y"])
        before = d.vmp_run(0, gamma_prior=PRIOR_G)
        assert before[3] == 0 and before[0].size == 0
        d.train_begin(P["X"], P["y"], np.zeros(2))
        with pytest.raises(SGPError, match="training run is open"):
            d.vmp_run(1, gamma_prior=PRIOR_G)
        d.train_end()
    with SGPDevice(10, 4, 1) as e:
        with pytest.raises(SGPError, match="set_inducing, set_kernel and set_data"):
            e.vmp_run(1, gamma_prior=PRIOR_G)
    with SGPDevice(10, 4, 1, d_out=2) as e:
        with pytest.raises(SGPError, match="UniSGP handles only"):
            e.vmp_run(1, gamma_prior=PRIOR_G)
