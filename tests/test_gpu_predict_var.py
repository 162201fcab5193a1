"""sgp_predict_var on the device: predictive means and (co)variances against NumPy references built from the oracle's kernel
matrix, the last sweep's q(v) and an explicit one, chunking, refusals, and the guarantee that the call leaves the sweep's state
alone (theta gradient, reuse of the resident statistics).

Error model (as in test_gpu_parity.py): the Q_ff term sigma2 - |L_K^-1 k*|^2 cancels, so its error is bounded by
50 eps cond(K_uu) sigma2; the Sigma term k*' Sigma_v k* = |L_S' k*|^2 by 50 eps cond(Sigma_v) k*' Sigma_v k* (a Cholesky
factor's backward error, eps |Sigma_v| |k*|^2, is at most cond(Sigma_v) eps times the form).  MultiSGP cross terms use
|k*' Sigma_v^(ij) k*| <= sqrt(form_ii form_jj) in place of the form."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FULL, TARGETS, REUSED = 0, 1, 2


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def synth(N, M, D, seed, d_out=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.stack([np.sin(X.sum(axis=1) + o) for o in range(d_out)], axis=1) + 0.1 * rng.normal(size=(N, d_out))
    y = (y - y.mean(axis=0)) / y.std(axis=0)
    return X, Xu, (y[:, 0] if d_out == 1 else y)


def reference(Xu, Xs, s2, ell, jitter, mu_v, Sigma_v, d_out=1):
    """NumPy: mean, latent (co)variance and the per-point error bound of the model above."""
    M = Xu.shape[0]
    Ks = O.kernelmatrix(s2, ell, Xu, Xs)                                    # M x ns
    Kuu = O.kernelmatrix(s2, ell, Xu) + jitter * np.eye(M)
    A = solve_triangular(np.linalg.cholesky(Kuu), Ks, lower=True)
    qff = s2 - np.sum(A * A, axis=0)
    mean = np.stack([Ks.T @ mu_v[o * M:(o + 1) * M] for o in range(d_out)], axis=1)
    forms = np.empty((Xs.shape[0], d_out, d_out))
    for i in range(d_out):
        for j in range(d_out):
            S_ij = Sigma_v[i * M:(i + 1) * M, j * M:(j + 1) * M]
            forms[:, i, j] = np.sum(Ks * (S_ij @ Ks), axis=0)
    C = forms + qff[:, None, None] * np.eye(d_out)[None]
    diag = np.sqrt(np.abs(np.einsum("sii->si", forms)))
    tol = 50 * EPS * (np.linalg.cond(Kuu) * s2 * np.eye(d_out)[None] + np.linalg.cond(Sigma_v) * diag[:, :, None] * diag[:, None, :])
    if d_out == 1:
        return mean[:, 0], C[:, 0, 0], tol[:, 0, 0]
    return mean, C, tol


def swept(G, N, M, D, seed, d_out=1, s2=0.8, jitter=1e-8, **kw):
    X, Xu, y = synth(N, M, D, seed, d_out)
    ell = np.linspace(1.1, 2.0, D)
    dev = G.SGPDevice(N, M, D, d_out, **kw)
    dev.set_inducing(Xu)
    dev.set_data(X, y)
    dev.set_kernel(s2, ell, jitter)
    dev.set_prior_isotropic(50.0)
    dev.set_noise([[10.0]] if d_out == 1 else 10.0 * np.eye(d_out))
    dev.sweep()
    return dev, X, Xu, y, ell


def test_kin40k_test_set_at_theta_opt(G, golden):
    """The posterior at theta_opt on the real training set, predictions at all 30 000 test points."""
    fx, data = golden("kin40k_fixture"), golden("kin40k_data")
    s2, ell = O.kernel_from_theta(fx["theta_opt"], softplus_params=True)
    M, D = fx["Xu"].shape
    with G.SGPDevice(10000, M, D) as dev:
        dev.set_inducing(fx["Xu"])
        dev.set_data(data["xtrain"], data["ytrain"])
        dev.set_kernel(s2, ell, 0.0)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[1e4]])
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        m, v = dev.predict_var(data["xtest"])
        assert np.array_equal(m, dev.predict(data["xtest"]))
    assert m.shape == v.shape == (30000,)
    _, v_ref, tol = reference(fx["Xu"], data["xtest"], s2, ell, 0.0, mu, Sig)
    err = np.abs(v - v_ref)
    assert np.all(err <= tol), (err / tol).max()
    assert np.all(v >= -tol)


@pytest.mark.parametrize("N,M,D", [(2000, 256, 8), (10000, 512, 8)])
def test_unisgp_after_a_sweep(G, N, M, D):
    dev, X, Xu, y, ell = swept(G, N, M, D, seed=N)
    with dev:
        Xs = np.random.default_rng(1).uniform(-2.0, 2.0, (777, D))
        mu, Sig, _ = dev.posterior(want_uv=False)
        m, v = dev.predict_var(Xs)
        m_n, v_n = dev.predict_var(Xs, noise=True)
        assert np.array_equal(m, dev.predict(Xs)) and np.array_equal(m_n, m)
    m_ref, v_ref, tol = reference(Xu, Xs, 0.8, ell, 1e-8, mu, Sig)
    assert np.all(np.abs(v - v_ref) <= tol), (np.abs(v - v_ref) / tol).max()
    np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())
    # with the noise flag: + 1 / w_bar, one rounding
    d = np.abs(v_n - (v + 0.1))
    assert np.all(d <= np.spacing(np.abs(v_n))), d.max()


def test_null_posterior_is_the_explicit_posterior_of_the_handle(G):
    N, M, D = 1500, 96, 3
    dev, X, Xu, y, ell = swept(G, N, M, D, seed=3)
    Xs = np.random.default_rng(2).uniform(-2.0, 2.0, (300, D))

    def same(where):
        mu, Sig, _ = dev.posterior(want_uv=False)
        a = dev.predict_var(Xs, noise=True)
        b = dev.predict_var(Xs, mu, Sig, noise=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), where
        return a
    with dev:
        r0 = same("after the sweep")
        dev.carry_posterior()
        r1 = same("after carry_posterior")
        assert np.array_equal(r0[1], r1[1])
        dev.theta_objective(want_grad=True)
        same("after theta_objective")
        dev.set_prior_meancov(np.zeros(M), 2.0 * np.eye(M))              # (reuses the Lambda factor's buffer)
        r3 = same("after set_prior(form 0)")
        assert np.array_equal(r0[1], r3[1])
        # a short device-paced run, then its last minibatch's q(v)
        dev.set_prior_isotropic(50.0)
        dev.train_begin(X, y, np.array([0.5] + [1.0] * D), jitter=1e-8)
        for k in range(3):
            dev.train_step(500 * k, 500, learn=True, reset_prior=(k == 0))
        dev.train_end()
        same("after train_end")


def test_changed_kernel_is_used(G):
    N, M, D = 1500, 128, 3
    dev, X, Xu, y, ell = swept(G, N, M, D, seed=4)
    Xs = np.random.default_rng(3).uniform(-2.0, 2.0, (200, D))
    with dev:
        mu, Sig, _ = dev.posterior(want_uv=False)
        ell2 = ell * 1.3
        dev.set_kernel(1.1, ell2, 1e-8)
        m, v = dev.predict_var(Xs)
        assert np.array_equal(m, dev.predict(Xs))
    m_ref, v_ref, tol = reference(Xu, Xs, 1.1, ell2, 1e-8, mu, Sig)
    np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())
    assert np.all(np.abs(v - v_ref) <= tol)
    _, v_old, _ = reference(Xu, Xs, 0.8, ell, 1e-8, mu, Sig)
    assert np.max(np.abs(v - v_old)) > 1e-3                              # (it is not the old kernel's)


def test_gradient_unchanged_by_predict_var(G):
    N, M, D = 600, 96, 3
    X, Xu, y = synth(N, M, D, seed=8)
    ell = np.array([1.2, 1.7, 2.2])
    res = []
    for with_call in (False, True):
        with G.SGPDevice(N, M, D) as dev:
            dev.set_inducing(Xu); dev.set_data(X, y); dev.set_kernel(0.8, ell, 1e-8)
            dev.set_prior_isotropic(50.0); dev.set_noise([[10.0]])
            dev.sweep()
            dev.set_noise([[35.0]])
            if with_call:
                dev.predict_var(X[:50], noise=True)
            res.append(dev.theta_objective(want_grad=True))
    (v0, g0), (v1, g1) = res
    assert v0 == v1 and np.array_equal(g0, g1)


def _snapshot(dev):
    mu, Sig, Uv = dev.posterior()
    Psi2, B, sc = dev.stats()
    return dict(mu=mu, Sigma=Sig, Uv=Uv, Psi2=Psi2, B=B, sc=sc, KuuL=dev.kuu_chol(),
                scalars=np.array([getattr(dev.scalars(), f) for f in ("sum_I1", "sum_I2", "energy", "logdet_kuu", "logdet_lambda")]))


def test_reused_sweep_after_predict_var(G):
    N, M, D = 3000, 192, 4
    snaps = []
    for with_call in (False, True):
        dev, X, Xu, y, ell = swept(G, N, M, D, seed=5, reuse_stats=True)
        with dev:
            dev.set_noise([[20.0]])
            if with_call:
                dev.predict_var(X[:100])
                dev.predict_var(X[:100], *dev.posterior(want_uv=False)[:2], noise=True)
                assert dev.sweep_kind()[0] == REUSED
            dev.sweep()
            assert dev.sweep_kind()[1] == REUSED
            snaps.append(_snapshot(dev))
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k


def test_chunks_and_edges(G, monkeypatch):
    N, M, D = 800, 40, 3
    X, Xu, y = synth(N, M, D, seed=6)
    ell = np.array([1.0, 1.4, 1.8])
    Xs = np.random.default_rng(4).uniform(-2.0, 2.0, (1000, D))
    out = {}
    for chunk in (None, "256"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)                # 1 000 points = 3 full chunks and 232
        with G.SGPDevice(N, M, D) as dev:
            dev.set_inducing(Xu); dev.set_data(X, y); dev.set_kernel(0.8, ell, 1e-8)
            dev.set_prior_isotropic(50.0); dev.set_noise([[10.0]])
            dev.sweep()
            mu, Sig, _ = dev.posterior(want_uv=False)
            out[chunk] = dev.predict_var(Xs)
            m0, v0 = dev.predict_var(Xs[:0])
            assert m0.shape == v0.shape == (0,)
            m1, v1 = dev.predict_var(Xs[:1])
            assert m1.shape == v1.shape == (1,)
            assert m1[0] == out[chunk][0][0] and v1[0] == out[chunk][1][0]
    assert np.array_equal(out[None][0], out["256"][0]) and np.array_equal(out[None][1], out["256"][1])
    _, v_ref, tol = reference(Xu, Xs, 0.8, ell, 1e-8, mu, Sig)
    assert np.all(np.abs(out["256"][1] - v_ref) <= tol)


def test_refusals(G):
    N, M, D = 400, 32, 2
    X, Xu, y = synth(N, M, D, seed=7)
    Xs = X[:10]
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu); dev.set_data(X, y); dev.set_kernel(0.8, [1.2, 1.5], 1e-8)
        dev.set_prior_isotropic(50.0); dev.set_noise([[10.0]])
        with pytest.raises(G.SGPError):                                   # no sweep yet
            dev.predict_var(Xs)
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
        from gaussianprocessnode_amd._lib import ptr
        Xc = np.ascontiguousarray(Xs)
        mean, var = np.empty(10), np.empty(10)
        for a, b in ((mu, None), (None, np.asfortranarray(Sig))):           # only one of the two
            rc = dev._lib.sgp_predict_var(dev._h, ptr(Xc), 10, ptr(a), ptr(b), 0, ptr(mean), ptr(var))
            assert rc == -1                                               # SGP_ERR_ARG
        bad = Sig.copy()
        bad[5, :] = bad[:, 5] = 0.0
        bad[5, 5] = -1.0
        with pytest.raises(G.PosDefException) as e:                       # non-PD explicit Sigma_v: its leading minor
            dev.predict_var(Xs, mu, bad)
        assert e.value.info == 6
        dev.set_posterior(mu, Uv)
        with pytest.raises(G.SGPError):                                   # set_posterior gives no Sigma_v
            dev.predict_var(Xs)
        dev.predict_var(Xs, mu, Sig)                                      # (the explicit one is fine)
        dev.sweep()
        dev.predict_var(Xs)
        dev.train_begin(X, y, np.array([0.5, 1.0, 1.0]), jitter=1e-8)
        with pytest.raises(G.SGPError):                                   # an open training run
            dev.predict_var(Xs, mu, Sig)
        dev.train_end()


def multi_reference_check(m, C, m_ref, C_ref, tol):
    assert np.all(np.abs(C - C_ref) <= tol), (np.abs(C - C_ref) / tol).max()
    assert np.array_equal(C, C.transpose(0, 2, 1))
    np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())


def test_multisgp_after_a_sweep_d_out_2(G):
    N, M, D, Do = 1500, 48, 2, 2
    dev, X, Xu, y, ell = swept(G, N, M, D, seed=9, d_out=Do)
    Xs = np.random.default_rng(5).uniform(-2.0, 2.0, (333, D))
    with dev:
        mu, Sig, _ = dev.posterior(want_uv=False)
        m, C = dev.predict_var(Xs)
        m_n, C_n = dev.predict_var(Xs, noise=True)
        assert np.array_equal(m, dev.predict(Xs)) and m.shape == (333, Do) and C.shape == (333, Do, Do)
    m_ref, C_ref, tol = reference(Xu, Xs, 0.8, ell, 1e-8, mu, Sig, Do)
    multi_reference_check(m, C, m_ref, C_ref, tol)
    d = np.abs(C_n - (C + 0.1 * np.eye(Do)[None]))
    assert np.all(d <= 2 * np.spacing(np.abs(C_n) + 0.1)), d.max()
    assert np.array_equal(C_n, C_n.transpose(0, 2, 1))


def test_multisgp_explicit_posterior_d_out_4(G):
    M, D, Do = 512, 3, 4
    Q = M * Do
    rng = np.random.default_rng(10)
    Xu = rng.uniform(-1.7, 1.7, (M, D))
    ell = np.array([1.3, 1.6, 2.0])
    mu = rng.normal(size=Q)
    A = rng.normal(size=(Q, Q)) / np.sqrt(Q)
    Sig = 0.05 * (A @ A.T) + 1e-3 * np.eye(Q)
    Xs = rng.uniform(-2.0, 2.0, (300, D))
    with G.SGPDevice(64, M, D, Do) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(0.9, ell, 1e-6)
        m, C = dev.predict_var(Xs, mu, Sig)
        assert np.array_equal(m, dev.predict(Xs, mu))
    m_ref, C_ref, tol = reference(Xu, Xs, 0.9, ell, 1e-6, mu, Sig, Do)
    multi_reference_check(m, C, m_ref, C_ref, tol)


def test_unisgp_predictive_uncertain_input(G):
    from gaussianprocessnode_amd import unisgp as U
    from gaussianprocessnode_amd.cubature import ghcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, NormalMeanVariance, PointMass
    from gaussianprocessnode_amd.meta import SEARDKernel, UniSGPMeta
    rng = np.random.default_rng(11)
    M = 30
    Xu = np.linspace(-3, 3, M)[:, None]
    A = rng.normal(size=(M, M)) / np.sqrt(M)
    Sig = 0.02 * A @ A.T + 1e-4 * np.eye(M)
    mu = rng.normal(size=M)
    meta = UniSGPMeta(ghcubature(15), Xu, None, None, None, None, SEARDKernel(), None, 0, 10, jitter=1e-8)
    theta = PointMass(np.array([0.9, 0.7]))
    q_v, q_w = MvNormalMeanCovariance(mu, Sig), PointMass(25.0)
    q_in = NormalMeanVariance(0.4, 0.3)
    m, v = U.predictive(q_in, q_v, q_w, theta, meta, noise=True)
    pts, wts = ghcubature(15).points_weights(0.4, 0.3)
    ms, vs, tol = reference(Xu, np.asarray(pts).reshape(-1, 1), 0.9, np.array([0.7]), 1e-8, mu, Sig)
    vs = vs + 1.0 / 25.0
    mean = wts @ ms
    var = wts @ (vs + ms * ms) - mean * mean
    assert abs(m - mean) <= 1e-12 * (1 + abs(mean))
    assert abs(v - var) <= 10 * (wts @ tol) + 1e-12 * (1 + abs(var))
    # the point-input path is the same engine call
    Xs = np.array([[0.1], [1.2]])
    m2, v2 = U.predictive(Xs, q_v, q_w, theta, meta, noise=False)
    _, v2_ref, tol2 = reference(Xu, Xs, 0.9, np.array([0.7]), 1e-8, mu, Sig)
    assert np.all(np.abs(v2 - v2_ref) <= tol2)
    p = U.probit_predictive(Xs, q_v, q_w, theta, meta)
    from scipy.special import ndtr
    np.testing.assert_allclose(p, ndtr(m2 / np.sqrt(1.0 + v2 + 1.0 / 25.0)), rtol=1e-14)
    meta.engine.close()
