"""sgp_predict_grad on the device against the float64 restatement of tests/predict_grad_ref.py at its bounds
(tests/test_predict_grad_host.py holds the bounds' constant to the spread of the restatement's own routes).

    grid + corners     every family x {ARD, isotropic} x d_out {1, 2, 4}; D in {1, 3, 8, 9, 32}; M in {5, 64, 65, 130} (below a tile,
                       a full tile, one and two tiles with padding); ns in {1, 4, 17, 65} (a partial wave, a partial 16-point
                       panel workgroup, a partial 64-column GEMM block)
    dense              a random dense SPD Sigma_v at d_out = 2: cross blocks far from symmetric (a transposed GEMM cannot pass)
    coincident_*       a point exactly on an inducing input and another 1e-9 away
    chunk              150 points under SGP_PREDICT_CHUNK = 64 against the default, bitwise
    rollout_*          forecast_gpssm(method="linearize") against the NumPy loop over the restatement

Every comparison prints its worst error / bound ratio before it asserts that it is at most 1."""
import ctypes as C

import numpy as np
import pytest

from tests import predict_grad_ref as PG

pytestmark = pytest.mark.gpu
ERR_ARG = -1


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_for(G, c, **kw):
    dev = G.SGPDevice(64, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    return dev


def call(dev, c, X=None, **kw):
    kw.setdefault("jac_cov", True)
    out = dev.predict_grad(c["X"] if X is None else X, c["mu_v"], c["Sigma_v"], **kw)
    return dict(zip(PG.OUTPUTS, (out[0], out[1], out[2], out[3], out[4])))


def check(name, c, out):
    for k, v in out.items():
        assert v is None or np.isfinite(v).all(), (name, k)
    r = PG.ratios(c["ref"], c["tol"], out)
    print(f"case {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, (name, k, v)
    if out.get("var_grad") is not None:
        assert np.array_equal(out["var_grad"], out["var_grad"].transpose(0, 2, 1, 3)), name
    if out.get("jac_cov") is not None:
        assert np.array_equal(out["jac_cov"], out["jac_cov"].transpose(0, 2, 1)), name


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in PG.OUTPUTS)


@pytest.mark.parametrize("name", PG.GRID + PG.CORNERS)
def test_against_the_restatement_and_the_existing_calls(G, name):
    c = PG.reference(name)
    ns, o = len(c["X"]), c["d_out"]
    with device_for(G, c) as dev:
        out = call(dev, c)
        check(name, c, out)
        # bitwise the existing calls
        pm = np.asarray(dev.predict(c["X"], c["mu_v"])).reshape(ns, o)
        assert np.array_equal(out["mean"], pm), name
        for noise in (False, True):
            m, v = dev.predict_var(c["X"], c["mu_v"], c["Sigma_v"], noise=noise)
            got = out if not noise else call(dev, c, noise=True)
            assert np.array_equal(got["var"], np.asarray(v).reshape(ns, o, o)) and np.array_equal(got["mean"], np.asarray(m).reshape(ns, o))
            if noise:                                                # the noise does not depend on x: var alone moves
                assert all(got[k].tobytes() == out[k].tobytes() for k in ("mean", "jac", "var_grad", "jac_cov"))


def test_a_dense_sigma_with_unsymmetric_cross_blocks(G):
    c = PG.reference("dense")
    with device_for(G, c) as dev:
        out = call(dev, c)
    check("dense", c, out)
    D = c["D"]
    off = (slice(None), slice(0, D), slice(D, 2 * D))
    ratio = PG.worst(np.abs(out["jac_cov"][off] - c["ref"]["jac_cov"][off]), c["tol"]["jac_cov"][off])
    print(f"case dense: off-diagonal jac_cov blocks, error / bound {ratio:.3g}")
    assert ratio <= 1.0
    bad = PG.evaluate(c, transpose_cross=True)
    assert PG.worst(np.abs(bad["jac_cov"][off] - c["ref"]["jac_cov"][off]), c["tol"]["jac_cov"][off]) > 1e3


@pytest.mark.parametrize("name", PG.COINCIDENT)
def test_points_on_and_beside_an_inducing_input(G, name):
    c = PG.reference(name)
    assert np.array_equal(c["X"][0], c["Xu"][0]) and 0 < np.max(np.abs(c["X"][1] - c["Xu"][1])) < 1e-8
    with device_for(G, c) as dev:
        check(name, c, call(dev, c))


def test_chunks_single_points_and_repeats_agree_bitwise(G, monkeypatch):
    c = PG.reference("chunk")
    assert len(c["X"]) == 150
    with device_for(G, c) as dev:
        whole = call(dev, c)
        check("chunk", c, whole)
        assert same_bits(whole, call(dev, c))
        for s in (0, 63, 64, 149):                                   # a point alone: the same bits as in the batch
            one = call(dev, c, X=c["X"][s:s + 1])
            assert all(one[k][0].tobytes() == whole[k][s].tobytes() for k in PG.OUTPUTS), s
        tail = call(dev, c, X=c["X"][100:])                          # ... and at another position among other points
        assert all(tail[k].tobytes() == whole[k][100:].tobytes() for k in PG.OUTPUTS)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")
    with device_for(G, c) as dev:
        assert same_bits(whole, call(dev, c))
        assert same_bits(whole, call(dev, c))


def test_optional_outputs_leave_the_others_unchanged(G):
    c = PG.reference("se_ard_o4_D8_M65_n17")
    with device_for(G, c) as dev:
        full = call(dev, c)
        for off in (("var",), ("var_grad",), ("jac_cov",), ("var", "var_grad"), ("var", "var_grad", "jac_cov")):
            got = call(dev, c, **{k: False for k in off})
            for k in PG.OUTPUTS:
                if k in off:
                    assert got[k] is None
                else:
                    assert got[k].tobytes() == full[k].tobytes(), (off, k)
        # mean = NULL through the ABI
        X, mu, Sig = G._lib.as_f64(c["X"]), G._lib.as_f64(c["mu_v"]), G._lib.as_f64(np.asarray(c["Sigma_v"]).T)
        jac = np.empty_like(full["jac"])
        p = G._lib.ptr
        rc = dev._lib.sgp_predict_grad(dev._h, p(X), len(X), p(mu), p(Sig), 0, None, p(jac), None, None, None)
        assert rc == 0 and jac.tobytes() == full["jac"].tobytes()


def _swept_device(G, c, **kw):
    """a handle with data and one finished sweep at the case's kernel"""
    rng = np.random.default_rng(5)
    N = 200
    X = rng.uniform(-1.7, 1.7, (N, c["D"]))
    Y = rng.normal(size=(N, c["d_out"]))
    dev = G.SGPDevice(N, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_data(X, Y if c["d_out"] > 1 else Y[:, 0])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_prior_isotropic(1.0)
    dev.set_noise(c["W"])
    dev.sweep()
    return dev


def test_the_posterior_rules(G):
    c = PG.reference("coincident_matern52")
    with _swept_device(G, c) as dev:
        mu, Sig, Uv = dev.posterior()
        own = dev.predict_grad(c["X"], jac_cov=True)                  # NULL posterior: the last sweep's
        given = dev.predict_grad(c["X"], mu, Sig, jac_cov=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(own, given))
        dev.set_posterior(mu, Uv)
        with pytest.raises(G._lib.SGPError, match="sgp_set_posterior gave no Sigma_v"):
            dev.predict_grad(c["X"])
        again = dev.predict_grad(c["X"], mu, Sig, jac_cov=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, given))
        dev.sweep()
        dev.predict_grad(c["X"])


def test_nothing_the_sweep_keeps_is_written(G):
    """On a SGP_FLAG_REUSE_STATS handle, the call between a set_noise and a sweep leaves sweep_kind, the REUSED sweep's results and
    the theta objective bitwise unchanged."""
    REUSED = G._lib.SGP_SWEEP_REUSED
    c = PG.reference("matern32_iso_o1_D9_M5_n65")
    W2 = 1.7 * np.asarray(c["W"])

    def run(between):
        with _swept_device(G, c, reuse_stats=True) as dev:
            dev.set_noise(W2)
            assert dev.sweep_kind()[0] == REUSED
            if between:
                dev.predict_grad(c["X"], jac_cov=True)
                dev.predict_grad(c["X"], c["mu_v"], c["Sigma_v"], noise=True)
                assert dev.sweep_kind()[0] == REUSED
            val, grad = dev.theta_objective(want_grad=True)
            dev.sweep()
            assert dev.sweep_kind()[1] == REUSED
            mu, Sig, Uv = dev.posterior()
            Psi2, B, sc = dev.stats()
            scal = np.array([getattr(dev.scalars(), f) for f in ("sum_I1", "sum_I2", "energy", "logdet_kuu", "logdet_lambda")])
            return [np.asarray(x) for x in (val, grad, mu, Sig, Uv, Psi2, B, sc, dev.kuu_chol(), scal)]
    for x, y in zip(run(False), run(True)):
        assert x.tobytes() == y.tobytes()


class Refusals:
    def __init__(self, G, c, dev):
        self.G, self.c, self.dev, self.lib = G, c, dev, dev._lib
        f = G._lib.as_f64
        ns, o, D = len(c["X"]), c["d_out"], c["D"]
        self.args = dict(X=f(c["X"]), ns=ns, mu=f(c["mu_v"]), Sig=f(np.asarray(c["Sigma_v"]).T), flags=0)
        self.out = dict(mean=np.full((o, ns), 7.0), jac=np.full((ns, o, D), 7.0), var=np.full((ns, o, o), 7.0),
                        vg=np.full((ns, o, o, D), 7.0), jc=np.full((ns, o * D, o * D), 7.0))

    def call(self, **over):
        a = dict(self.args, **self.out)
        a.update(over)
        p = self.G._lib.ptr
        h = over.get("h", self.dev._h)
        return self.lib.sgp_predict_grad(h, p(a["X"]), a["ns"], p(a["mu"]), p(a["Sig"]), a["flags"], p(a["mean"]), p(a["jac"]),
                                         p(a["var"]), p(a["vg"]), p(a["jc"]))

    def untouched(self):
        return all((v == 7.0).all() for v in self.out.values())


def test_every_refusal_leaves_the_outputs_untouched(G):
    c = PG.reference("coincident_se")
    with device_for(G, c) as dev:
        k = Refusals(G, c, dev)
        assert k.call(h=None) == ERR_ARG
        for over in (dict(X=None), dict(jac=None), dict(flags=2), dict(flags=-1), dict(mu=None), dict(Sig=None),
                     dict(mu=None, Sig=None)):                       # (no sweep yet: a NULL posterior is refused)
            assert k.call(**over) == ERR_ARG and k.untouched(), over
        for bad in (np.nan, np.inf):
            X = k.args["X"].copy()
            X[-1, -1] = bad
            assert k.call(X=X) == ERR_ARG and k.untouched()
        dev.set_kernel_family("matern12")
        assert k.call() == ERR_ARG and k.untouched()
        assert b"Matern-1/2" in dev._lib.sgp_last_error(dev._h)
        dev.set_kernel_family("se")
        assert k.call(ns=0) == 0 and k.untouched()
        # a K_uu that is not positive definite returns its failing minor: two identical inducing inputs and no jitter
        Xu = np.array(c["Xu"])
        Xu[3] = Xu[1]
        dev.set_inducing(Xu)
        dev.set_kernel(c["sigma2"], c["ell_dev"], 0.0, family="se")
        rc = k.call()
        assert 0 < rc <= c["M"] and k.untouched()
        assert dev._lib.sgp_last_error(dev._h).decode() == "K_uu (current kernel) is not positive definite"
        assert k.call(var=None) == rc and k.untouched()
        # ... and Sigma_v's, only when var is wanted
        dev.set_inducing(c["Xu"])
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family="se")
        Sig = k.args["Sig"].copy()
        Sig[2, 2] = -1.0
        assert k.call(Sig=Sig) == 3 and k.untouched()
        assert dev._lib.sgp_last_error(dev._h).decode() == "Sigma_v is not positive definite"
        assert k.call(Sig=Sig, var=None) == 0 and not k.untouched()


def test_an_open_training_run_is_refused(G):
    c = PG.reference("rollout_se")
    rng = np.random.default_rng(9)
    N = 128
    X, y = rng.uniform(-1.5, 1.5, (N, c["D"])), rng.normal(size=N)
    with G.SGPDevice(N, c["M"], c["D"], 1) as dev:
        dev.set_inducing(c["Xu"])
        dev.set_prior_isotropic(1.0)
        dev.set_noise([[10.0]])
        dev.train_begin(X, y, np.zeros(c["D"] + 1), jitter=1e-6)
        try:
            with pytest.raises(G._lib.SGPError, match="training run is open"):
                dev.predict_grad(c["X"], np.zeros(c["M"]), np.eye(c["M"]))
        finally:
            dev.train_end()


# ---- forecast_gpssm(method="linearize") ------------------------------------------------------------------------------------------------
class _QV:
    def __init__(self, mu, Sig):
        self.mu, self.Sig = mu, Sig

    def mean_cov(self):
        return self.mu, self.Sig


def _gpssm(G, c):
    from gaussianprocessnode_amd.distributions import PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta
    from gaussianprocessnode_amd.cubature import srcubature

    class Kernel:                                                    # theta is ignored: the case's kernel as it is
        family = c["family"]

        def __call__(self, theta):
            return c["sigma2"], np.asarray(c["ell"])
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, Kernel(), jitter=c["jitter"])
    return meta, _QV(c["mu_v"], c["Sigma_v"]), PointMass(np.asarray(c["W"])), PointMass(np.zeros(1))


def _close(meta):
    for eng in (getattr(meta, "engine", None), getattr(meta, "_aux_engine_out", None)):
        if eng is not None:
            eng.close()


@pytest.mark.parametrize("name", ["rollout_se", "rollout_matern52"])
def test_the_linearised_forecast(G, name):
    from gaussianprocessnode_amd.distributions import PointMass
    from gaussianprocessnode_amd.train import forecast_gpssm
    from tests.test_predict_grad_host import rollout_start
    c = PG.reference(name)
    m0, S0 = rollout_start(c)
    meta, q_v, q_w, q_theta = _gpssm(G, c)

    class Gauss:
        def __init__(self, m, S):
            self.m, self.S = m, S

        def mean(self):
            return self.m

        def mean_cov(self):
            return self.m, self.S
    try:
        means, covs = forecast_gpssm([Gauss(m0[b], S0[b]) for b in range(2)], 3, q_v, q_w, q_theta, meta, method="linearize")
        want_m, want_S = PG.linearize_rollout(c, m0, S0, 3, noise=True)
        # per step the outputs hold to the restatement's bounds (below 1e-9 of their scale at cond(K_uu) <= 1e5) and W^-1 to a few
        # roundings; three steps through Jacobians of norm below 10 amplify that by less than 1e3
        tol_m, tol_S = 1e-6 * max(1.0, np.max(np.abs(want_m))), 1e-6 * max(1.0, np.max(np.abs(want_S)))
        print(f"case {name}: linearised forecast, max error mean {np.max(np.abs(means - want_m)):.3g} cov {np.max(np.abs(covs - want_S)):.3g}")
        assert np.max(np.abs(means - want_m)) <= tol_m and np.max(np.abs(covs - want_S)) <= tol_S
        assert np.array_equal(covs, covs.transpose(0, 1, 3, 2))
        # S = 0 and one step: predict_var's mean and covariance
        m1, S1 = forecast_gpssm([PointMass(m0[b]) for b in range(2)], 1, q_v, q_w, q_theta, meta, noise=False, method="linearize")
        eng = meta._aux_engine_out
        pm, pv = eng.predict_var(m0, c["mu_v"], c["Sigma_v"])
        assert np.array_equal(m1[0], pm) and np.array_equal(S1[0], pv)
        if name == "rollout_se":                                     # the default method is what it was
            a = forecast_gpssm([Gauss(m0[b], S0[b]) for b in range(2)], 2, q_v, q_w, q_theta, meta)
            b = forecast_gpssm([Gauss(m0[b], S0[b]) for b in range(2)], 2, q_v, q_w, q_theta, meta, method="exact")
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            mm, SS = eng.psi_predict(m0, S0, noise=True)[:2]
            assert np.array_equal(a[0][0], mm) and np.array_equal(a[1][0], np.asarray(SS).reshape(2, 2, 2))
        else:
            with pytest.raises(ValueError):
                forecast_gpssm([Gauss(m0[0], S0[0])], 1, q_v, q_w, q_theta, meta)
    finally:
        _close(meta)


def test_predictive_grad(G):
    from gaussianprocessnode_amd import multisgp
    c = PG.reference("rollout_matern52")
    meta, q_v, q_w, q_theta = _gpssm(G, c)
    try:
        m, var, jac, vg = multisgp.predictive(c["X"], q_v, q_w, q_theta, meta, noise=False, grad=True)
        r = PG.ratios(c["ref"], c["tol"], dict(mean=m, jac=jac, var=var, var_grad=vg))
        print("case rollout_matern52: multisgp.predictive(grad=True), error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert max(r.values()) <= 1.0
    finally:
        _close(meta)
