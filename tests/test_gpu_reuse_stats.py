"""Sweeps over resident statistics (SGP_FLAG_REUSE_STATS, sgp_set_targets, sgp_sweep_kind) on the device: a handle with the flag
must compute bitwise what a handle without it computes after the same setters, skip the work it says it skips, drop the
reuse wherever the statistics stop being valid, and call an all-reduce hook only for the tail of new targets."""
import ctypes as C

import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu

FULL, TARGETS, REUSED = 0, 1, 2


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def synth(N, M, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    return X, Xu, (y - y.mean()) / y.std()


def snapshot(dev):
    """Everything a sweep leaves behind, as raw arrays (compared bitwise)."""
    mu, Sig, Uv = dev.posterior()
    out = np.empty(8)
    assert dev._lib.sgp_get_scalars(dev._h, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    Psi2, B, sc = dev.stats()
    snap = dict(mu=mu, Sigma=Sig, Uv=Uv, scalars=out, Psi2=Psi2, B=B, stats_scalars=sc, KuuL=dev.kuu_chol())
    if dev.d_out > 1:
        snap["wishart"] = dev.wishart_invscale()
    return snap


def assert_bitwise(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} differs (max |diff| {np.max(np.abs(a[k] - b[k])):.3e})"


# T: the overlapped order at BASELINE's shape; C4; a ragged point count; MultiSGP with weighted points and Gaussian outputs
CASES = {
    "T": dict(N=10000, M=512, D=8, d_out=1, overlap="1"),
    "C4": dict(N=4000, M=128, D=2, d_out=1, overlap=None),
    "ragged": dict(N=6007, M=192, D=3, d_out=1, overlap=None),
    "multi": dict(N=3005, M=96, D=2, d_out=2, overlap=None),
}


def _setters(case, seed):
    """The setter sequence of the equivalence test: list of (name, callable(dev)) applied between the sweeps."""
    c = CASES[case]
    N, M, D, Do = c["N"], c["M"], c["D"], c["d_out"]
    X, Xu, y = synth(N, M, D, seed)
    rng = np.random.default_rng(seed + 1)
    ell, ell2 = rng.uniform(0.8, 1.6, D), rng.uniform(0.8, 1.6, D)
    wts = rng.uniform(0.2, 1.0, N) if Do > 1 else None
    Y = np.stack([y, np.cos(X[:, 0])], axis=1)[:, :Do] if Do > 1 else y
    Y2 = Y + 0.3 * rng.normal(size=np.shape(Y))
    X3 = X + 0.01 * rng.normal(size=X.shape)
    vy = rng.uniform(0.05, 0.3, N) if Do == 1 else None
    W = np.eye(Do) * 30.0 + (np.full((Do, Do), 2.0) if Do > 1 else 0.0)
    S_y = np.diag(rng.uniform(1.0, 3.0, Do))

    def first(dev):
        dev.set_inducing(Xu)
        dev.set_data(X, Y, None, wts, n_nodes=N // 5 if Do > 1 else None)
        if Do > 1:
            dev.set_output_cov_sum(S_y)
        dev.set_kernel(0.9, ell, 1e-8)
        dev.set_prior_isotropic(50.0)
        dev.set_noise(W)

    def targets(dev):
        if Do > 1:
            dev.set_targets(Y2)
            dev.set_output_cov_sum(0.5 * S_y)
        else:
            dev.set_targets(Y2, vy)

    steps = [("set_noise", lambda d: d.set_noise(W * 1.7), REUSED),
             ("set_prior", lambda d: d.set_prior_isotropic(20.0), REUSED),
             ("set_targets", targets, TARGETS),
             ("set_kernel same", lambda d: d.set_kernel(0.9, ell, 1e-8), REUSED),
             ("set_kernel new", lambda d: d.set_kernel(1.1, ell2, 1e-8), FULL),
             ("set_data new X", lambda d: d.set_data(X3, Y, None, wts, n_nodes=N // 5 if Do > 1 else None), FULL)]
    return first, steps, dict(X3=X3, Xu=Xu, Y=Y, wts=wts, ell2=ell2, W=W * 1.7, D=D)


@pytest.mark.parametrize("case", list(CASES))
def test_reused_sweeps_are_bitwise_full_sweeps(G, case, monkeypatch):
    c = CASES[case]
    if c["overlap"] is not None:
        monkeypatch.setenv("SGP_OVERLAP", c["overlap"])
    first, steps, ref = _setters(case, 11)
    with G.SGPDevice(c["N"], c["M"], c["D"], c["d_out"], keep_kuf=True, reuse_stats=True) as a, \
            G.SGPDevice(c["N"], c["M"], c["D"], c["d_out"], keep_kuf=True) as b:
        assert a.reuse_stats and not b.reuse_stats
        for dev in (a, b):
            first(dev)
            dev.sweep()
        assert a.sweep_kind() == (REUSED, FULL)
        assert_bitwise(snapshot(a), snapshot(b), "first sweep")
        kinds = []
        for name, step, want in steps:
            for dev in (a, b):
                step(dev)
            assert a.sweep_kind()[0] == want, name
            assert b.sweep_kind() == (FULL, FULL), name
            for dev in (a, b):
                dev.sweep()
            kinds.append(a.sweep_kind()[1])
            assert_bitwise(snapshot(a), snapshot(b), f"after {name}")
        assert kinds == [REUSED, REUSED, TARGETS, REUSED, FULL, FULL]
        mu, Sig, _ = a.posterior()
    if c["d_out"] == 1:
        # and the last state against the oracle, at the parity tests' bound
        r = O.vmp_sweep(ref["Xu"], ref["X3"], ref["Y"], None, 1.1, ref["ell2"], float(ref["W"][0, 0]), jitter=1e-8,
                        Lambda0=np.eye(c["M"]) / 20.0, xi0=np.zeros(c["M"]))
        assert np.linalg.norm(mu - r.mu_v) / np.linalg.norm(r.mu_v) < 1e-5
        assert np.linalg.norm(Sig - r.Sigma_v) / np.linalg.norm(r.Sigma_v) < 1e-5


def test_skipped_phases_accrue_no_time(G):
    c = CASES["T"]
    X, Xu, y = synth(c["N"], c["M"], c["D"], 5)
    with G.SGPDevice(c["N"], c["M"], c["D"], reuse_stats=True) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(0.9, np.ones(c["D"]), 1e-8)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[30.0]])
        dev.sweep()
        dev.scalars()
        assert dev.sweep_kind()[0] == REUSED
        dev.phase_totals(reset=True)
        for i in range(20):
            dev.set_noise([[30.0 + i]])
            dev.sweep()
        tot, n = dev.phase_totals(reset=True)
        assert n == 20 and dev.sweep_kind()[1] == REUSED
        assert tot[G._lib.SGP_T_GRAM] == 0 and tot[G._lib.SGP_T_SYRK] == 0 and tot[G._lib.SGP_T_KUU] == 0
        assert tot[G._lib.SGP_T_LOCAL] == 0 and tot[G._lib.SGP_T_GAP_LOCAL_FINISH] == 0
        assert tot[G._lib.SGP_T_SWEEP] > 0 and tot[G._lib.SGP_T_FINISH1] > 0
        dev.set_targets(-y)
        dev.sweep()
        tot, n = dev.phase_totals(reset=True)
        assert n == 1 and dev.sweep_kind()[1] == TARGETS
        assert tot[G._lib.SGP_T_SYRK] == 0 and tot[G._lib.SGP_T_KUU] == 0 and tot[G._lib.SGP_T_LOCAL] > 0


def test_reuse_is_dropped_where_the_statistics_stop_being_valid(G):
    N, M, D = 3000, 128, 3
    X, Xu, y = synth(N, M, D, 7)
    ell, ell2 = np.array([1.1, 0.9, 1.3]), np.array([0.7, 1.2, 1.0])
    with G.SGPDevice(N, M, D, keep_kuf=True, reuse_stats=True) as a, G.SGPDevice(N, M, D, keep_kuf=True) as b:
        with pytest.raises(G.SGPError):
            a.set_targets(y)                                  # before any set_data
        for dev in (a, b):
            dev.set_inducing(Xu)
            dev.set_data(X, y)
            dev.set_kernel(0.8, ell, 1e-8)
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[25.0]])
            dev.sweep()
        # the per-point outputs and predictions read the statistics, they do not change them
        a.w_stats()
        a.predict(X[:50])
        assert a.sweep_kind()[0] == REUSED
        # the objective at another theta re-forms the statistics there: back at the old theta the next sweep is a full one
        for dev in (a, b):
            dev.set_kernel(0.8, ell2, 1e-8)
            dev.theta_objective(want_grad=True)
            dev.set_kernel(0.8, ell, 1e-8)
        assert a.sweep_kind()[0] == FULL
        for dev in (a, b):
            dev.sweep()
        assert a.sweep_kind() == (REUSED, FULL)
        assert_bitwise(snapshot(a), snapshot(b), "after theta_objective")
        # the objective at the sweep's own theta reuses what is resident
        a.theta_objective(want_grad=True)
        assert a.sweep_kind()[0] == REUSED
        a.bind_stats(0)                                       # (re)binding the statistics buffer
        assert a.sweep_kind()[0] == FULL
        a.sweep()
        assert_bitwise(snapshot(a), snapshot(b), "after bind_stats")
        # predictive variances read the K_uu chain's outputs and q(v), they do not change them
        a.predict_var(X[:50])
        assert a.sweep_kind()[0] == REUSED

        # every other path that overwrites the statistics or changes what they depend on: the next sweep is a full one
        def two_phase(dev):
            dev.sweep_local()
            dev.sweep_finish()

        def passthrough(buf, count, stream):                  # one rank: the sum is the identity
            pass

        steps = [("set_inducing", lambda d: d.set_inducing(Xu)),
                 ("sweep_local + sweep_finish", two_phase),
                 ("time_kernel", lambda d: d.time_kernel(G._lib.SGP_T_GRAM, 2)),
                 ("set_allreduce", lambda d: d.set_allreduce(passthrough)),
                 ("set_allreduce(None)", lambda d: d.set_allreduce(None))]
        for name, step in steps:
            for dev in (a, b):
                step(dev)
            assert a.sweep_kind()[0] == FULL, name
            assert b.sweep_kind() == (FULL, FULL), name
            for dev in (a, b):
                dev.sweep()
            assert a.sweep_kind() == (REUSED, FULL), name
            assert_bitwise(snapshot(a), snapshot(b), f"after {name}")
        # a device-paced training run rewrites the statistics of its windows and moves theta
        for dev in (a, b):
            dev.train_begin(X, y, np.zeros(1 + D), jitter=1e-6)
            assert dev.sweep_kind()[0] == FULL
            dev.train_step(0, 1000)
            assert dev.sweep_kind()[0] == FULL
            dev.train_end()
        assert a.sweep_kind()[0] == FULL
        assert b.sweep_kind()[0] == FULL
        for dev in (a, b):
            dev.set_data(X, y)                                # (the run leaves the handle without data)
            dev.set_kernel(0.8, ell, 1e-8)
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[25.0]])
            dev.sweep()
        assert a.sweep_kind() == (REUSED, FULL)
        assert_bitwise(snapshot(a), snapshot(b), "after a training run")


def test_hook_is_called_once_for_new_targets_and_never_for_reused_statistics(G):
    N, M, D = 4000, 128, 2
    X, Xu, y = synth(N, M, D, 9)
    counts = {"a": [], "b": []}

    def hook_for(key):
        return lambda buf, count, stream: counts[key].append(count)      # one rank: the sum is the identity

    with G.SGPDevice(N, M, D, reuse_stats=True) as a, G.SGPDevice(N, M, D) as b:
        for key, dev in (("a", a), ("b", b)):
            dev.set_allreduce(hook_for(key))
            dev.set_inducing(Xu)
            dev.set_data(X, y)
            dev.set_kernel(0.8, np.array([1.0, 1.2]), 1e-8)
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[25.0]])
            dev.sweep()
        assert_bitwise(snapshot(a), snapshot(b), "hooked full sweep")
        _, _, mp = a.stats_layout()
        del counts["a"][:]
        for dev in (a, b):
            dev.set_noise([[40.0]])
            dev.sweep()
        assert a.sweep_kind()[1] == REUSED and counts["a"] == []
        assert_bitwise(snapshot(a), snapshot(b), "hooked reused sweep")
        for dev in (a, b):
            dev.set_targets(0.5 * y)
            dev.sweep()
        assert a.sweep_kind()[1] == TARGETS
        assert counts["a"] == [mp * 1 + 8 + 1]
        assert_bitwise(snapshot(a), snapshot(b), "hooked targets sweep")
        for dev in (a, b):
            dev.set_allreduce(None)


def test_vmp_loops_are_bitwise_equal_with_and_without_reuse(G):
    from gaussianprocessnode_amd import train as TR
    N, M, D = 2000, 64, 2
    X, Xu, y = synth(N, M, D, 13)
    labels = (y > 0).astype(float)
    res = {}
    for reuse in (False, True):
        with G.SGPDevice(N, M, D, reuse_stats=reuse) as dev:
            qv, ab = TR.vmp_regression([0.9, 1.1, 0.8], X, y, Xu, dev, iterations=7)
            res[("reg", reuse)] = (qv.mean(), qv.cov(), ab)
        with G.SGPDevice(N, M, D, reuse_stats=reuse) as dev:
            qv, ab = TR.vmp_classification([0.9, 1.1, 0.8], X, labels, Xu, dev, iterations=6, jitter=1e-6)
            assert dev.sweep_kind()[1] == (TARGETS if reuse else FULL)
            res[("cls", reuse)] = (qv.mean(), qv.cov(), ab)
    for kind in ("reg", "cls"):
        m0, S0, ab0 = res[(kind, False)]
        m1, S1, ab1 = res[(kind, True)]
        assert np.array_equal(m0, m1) and np.array_equal(S0, S1) and ab0 == ab1, kind


def test_unisgp_node_mirror_loop_is_bitwise_equal_with_and_without_reuse(G):
    from gaussianprocessnode_amd import meta as Mt
    from gaussianprocessnode_amd import unisgp as U
    from gaussianprocessnode_amd.distributions import GammaShapeRate, MvNormalMeanCovariance, NormalMeanVariance, PointMass
    N, M = 400, 24
    rng = np.random.default_rng(17)
    X = rng.uniform(-2, 2, N)
    y = np.sin(2 * X) + 0.1 * rng.normal(size=N)
    Xu = np.linspace(-2, 2, M)
    theta = PointMass(np.array([1.0, 0.8]))
    prior = MvNormalMeanCovariance(np.zeros(M), 50.0 * np.eye(M))
    results = {}
    for reuse in (False, True):
        eng = G.SGPDevice(N, M, 1, keep_kuf=True, reuse_stats=reuse)
        meta = Mt.make_uni_meta(None, Xu, Mt.SEARDKernel(), N, engine=eng, jitter=1e-8)
        q_w, out = GammaShapeRate(1.0, 0.1), []
        for it in range(7):
            q_out = [NormalMeanVariance(y[i] + 0.05 * it, 0.1) for i in range(N)]
            msgs = [U.rule_v(q_out[i], PointMass(X[i]), q_w, theta, meta) for i in range(N)]
            q = prior
            for m in msgs:
                q = U.prod(q, m)
            q_w = U.rule_w_summed(meta, GammaShapeRate(1.0, 0.1))
            out.append((q.mean(), q.cov(), q_w.shape(), q_w.rate()))
        kinds = eng.sweep_kind()
        eng.close()
        results[reuse] = (out, kinds)
    assert results[True][1][1] == TARGETS
    for (m0, S0, a0, b0), (m1, S1, a1, b1) in zip(results[False][0], results[True][0]):
        assert np.array_equal(m0, m1) and np.array_equal(S0, S1) and a0 == a1 and b0 == b1
