"""Matern-1/2, 3/2 and 5/2 kernels (sgp_set_kernel_family, sgp_kernelmatrix_family) on the device against the oracle with its
kernel replaced by the Matern restatement of tests/test_kernel_family_host.py (which pins that restatement to sklearn): the Gram
kernels, the sweep, prediction, the theta objective and its gradient, the training drivers, the statistics reuse and a sharded
sweep.  The bounds are those the SE tests apply to the same entry points (test_gpu_parity, test_gpu_dims, test_gpu_shards);
test_kernel_family_host.test_fixtures_discriminate_between_families shows that they tell the families apart."""
import math
import zlib

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests.test_gpu_parity import kuu_tol, post_tol, relF
from tests.test_gpu_parity import synth as parity_synth
from tests.test_kernel_family_host import MATERN, matern

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def case_inputs(name, N, M, D, cls):
    """The inputs of test_gpu_parity.test_sweep_matches_oracle's case `name` (s2 = 0.9, ell = 1.5 .. 3.0)."""
    X, Xu, y, vy = parity_synth(N, M, D, seed=zlib.crc32(name.encode()) % 1000, classification=cls)
    return X, Xu, y, vy, 0.9, np.linspace(1.5, 3.0, D)


# ------------------------------------------------------------------------------------------------
# 1. kernelmatrix

@gpu
@pytest.mark.parametrize("family", MATERN)
def test_kernelmatrix_matches_the_restatement(G, family):
    rng = np.random.default_rng(len(family))
    K_ref = matern(family)
    for D in [1, 3, 8, 16]:
        A, B = rng.normal(size=(70, D)), rng.normal(size=(45, D))
        B[:5] = A[:5]                                               # coincident points: r = 0
        B[5:10] = A[5:10] + 1e-9 * rng.normal(size=(5, D))          # near-coincident: r ~ 1e-9
        for ell in (rng.uniform(0.5, 3.0, D), np.array([1.7])):
            K = G.kernelmatrix(A, B, 0.37, ell, family=family)
            assert np.isfinite(K).all()
            np.testing.assert_allclose(K, K_ref(0.37, ell, A, B), rtol=1e-13, atol=1e-300)
            assert np.all(K[np.arange(5), np.arange(5)] == 0.37)
    # the SE name is the SE entry point
    np.testing.assert_allclose(G.kernelmatrix(A, B, 0.37, ell, family="se"), O.kernelmatrix(0.37, ell, A, B), rtol=1e-13)


# ------------------------------------------------------------------------------------------------
# 2. the sweep (bounds of test_gpu_parity.test_sweep_matches_oracle)

def check_sweep(G, family, X, Xu, y, vy, s2, ell_dev, w, jit, omega=None):
    N, M = len(X), len(Xu)
    D = X.shape[1]
    ell = np.broadcast_to(ell_dev, (D,)).copy()
    E_logw = math.log(w) - 0.01
    with G.SGPDevice(N, M, D, keep_kuf=True) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y, vy, weights=omega)
        dev.set_kernel(s2, ell_dev, jit, family=family)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[w]], E_logw)
        dev.sweep()
        Psi2, B, sc_data = dev.stats()
        KuuL = dev.kuu_chol()
        mu, Sig, Uv = dev.posterior()
        sc = dev.scalars()
        I1, I2 = dev.w_stats()
        obj = dev.theta_objective()
    stats = O.suff_stats(Xu, X, y, vy, s2, ell, omega=omega)
    ref = O.vmp_sweep(Xu, X, y, vy, s2, ell, w, E_logw=E_logw, jitter=jit, Lambda0=np.eye(M) / 50.0, xi0=np.zeros(M), stats=stats)
    assert relF(Psi2, ref.stats.Psi2) < 1e-13, relF(Psi2, ref.stats.Psi2)
    assert relF(B, np.reshape(ref.stats.b, B.shape)) < 1e-13
    assert math.isclose(sc_data[0], ref.stats.s_yy[0, 0], rel_tol=1e-13)
    Kuu = O.kernelmatrix(s2, ell, Xu) + jit * np.eye(M)
    cond_K = np.linalg.cond(Kuu)
    assert relF(KuuL, ref.KuuL) < kuu_tol(cond_K), (relF(KuuL, ref.KuuL), cond_K)
    cond_L = np.linalg.cond(np.eye(M) / 50.0 + w * ref.stats.Psi2)
    tol_post = post_tol(cond_L)
    assert relF(mu, ref.mu_v) < tol_post, (relF(mu, ref.mu_v), cond_L)
    assert relF(Sig, ref.Sigma_v) < tol_post
    assert relF(Uv, ref.Uv) < tol_post
    tol_I1 = 50 * np.finfo(float).eps * cond_K * ref.stats.s_kk + 1e-12
    assert abs(sc.sum_I1 - ref.sum_I1) <= tol_I1
    assert math.isclose(sc.sum_I2, ref.sum_I2, rel_tol=max(1e-7, tol_post))
    assert abs(sc.energy - ref.energy) <= max(1e-7, tol_post) * abs(ref.energy) + 0.5 * w * tol_I1
    assert sc.info_kuu == 0 and sc.info_lambda == 0
    if omega is None:
        rI1, rI2 = O.w_stats_perpoint(Xu, X, y, vy, s2, ell, ref.KuuL, ref.mu_v, ref.Uv)
        np.testing.assert_allclose(I1, rI1, rtol=0, atol=tol_I1 / N + 1e-12)
        scale_I2 = float(np.max(y * y + np.sum((ref.Uv @ O.kernelmatrix(s2, ell, Xu, X)) ** 2, axis=0)))
        np.testing.assert_allclose(I2, rI2, rtol=1e-6, atol=max(1e-9, tol_post * scale_I2))
        ref_obj = O.theta_objective(Xu, X, y, s2, ell, ref.mu_v, ref.Uv, w, jitter=jit)
        assert abs(obj - ref_obj) <= 1e-7 * abs(ref_obj) + 0.5 * w * tol_I1


SHAPES = [("toy-C1", 50, 20, 1, 100.0, 1e-8, False), ("banana-C4", 1000, 128, 2, 3.0, 1e-8, True),
          ("kin40k-T", 1500, 512, 8, 1e4, 0.0, False), ("gated", 4000, 128, 2, 30.0, 1e-8, False)]


@gpu
@pytest.mark.parametrize("family", MATERN)
@pytest.mark.parametrize("name,N,M,D,w,jit,cls", SHAPES, ids=[s[0] for s in SHAPES])
def test_sweep_matches_the_oracle(G, family, name, N, M, D, w, jit, cls, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    X, Xu, y, vy, s2, ell = case_inputs(name, N, M, D, cls)
    check_sweep(G, family, X, Xu, y, vy, s2, ell, w, jit)


@gpu
@pytest.mark.parametrize("family", MATERN)
@pytest.mark.parametrize("iso", [False, True], ids=["ard", "iso"])
def test_sweep_at_d16_matches_the_oracle(G, family, iso, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    D = 16
    X, Xu, y, _, _, _ = case_inputs("d16", 700, 100, D, False)
    ell = np.array([2.0 * math.sqrt(2.0)]) if iso else math.sqrt(2.0) * np.linspace(3.0, 1.5, D)
    check_sweep(G, family, X, Xu, y, None, 0.9, ell, 100.0, 1e-8)


@gpu
@pytest.mark.parametrize("family", MATERN)
def test_weighted_cubature_points_match_the_oracle(G, family, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    X, Xu, y, _, s2, ell = case_inputs("weighted", 900, 64, 3, False)
    omega = np.random.default_rng(3).uniform(0.05, 1.0, len(X))
    check_sweep(G, family, X, Xu, y, None, s2, ell, 30.0, 1e-8, omega=omega)


@gpu
@pytest.mark.parametrize("family", MATERN)
def test_multisgp_sweep_matches_the_oracle(G, family, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    T, M, Do, Din = 60, 40, 2, 2
    rng = np.random.default_rng(T + M)
    Xu = rng.uniform(-2, 2, (M, Din))
    s2, ell = 0.8, np.array([1.3, 0.9])
    means = rng.normal(size=(T, Din))
    cub = [O.srcubature(means[t], np.diag(rng.uniform(0.02, 0.2, Din))) for t in range(T)]
    pts, wts = np.stack([c[0] for c in cub]), np.stack([c[1] for c in cub])
    S = pts.shape[1]
    Y = rng.normal(size=(T, Do))
    A = rng.normal(size=(Do, Do))
    W = A @ A.T + Do * np.eye(Do)
    E_logdetW = float(np.linalg.slogdet(W)[1]) - 0.1
    Q = Do * M
    Lam0, xi0 = np.eye(Q) / 10.0, 0.01 * rng.normal(size=Q)
    ms = O.multi_suff_stats(Xu, pts, wts, Y, None, s2, ell)
    mu_ref, Sig_ref = O.multi_v_update(ms, W, Lam0, xi0)
    with G.SGPDevice(T * S, M, Din, d_out=Do) as dev:
        dev.set_inducing(Xu)
        dev.set_data(pts.reshape(T * S, Din), np.repeat(Y, S, axis=0), None, wts.reshape(-1), n_nodes=T)
        dev.set_kernel(s2, ell, 1e-10, family=family)
        dev.set_prior_precision(xi0, Lam0)
        dev.set_noise(W, E_logdetW)
        dev.sweep()
        Psi2, B, _ = dev.stats()
        mu, Sig, _ = dev.posterior()
    assert relF(Psi2, ms.Psi2) < 1e-12 and relF(B, ms.B) < 1e-12
    assert relF(mu, mu_ref) < 1e-8 and relF(Sig, Sig_ref) < 1e-8


# ------------------------------------------------------------------------------------------------
# 3. prediction (the reference of test_gpu_predict_var with the kernel replaced)

@gpu
@pytest.mark.parametrize("family", MATERN)
@pytest.mark.parametrize("D", [2, 8, 9])
def test_predict_and_predict_var_match_the_restatement(G, family, D, monkeypatch):
    from tests.test_gpu_predict_var import reference
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    X, Xu, y, _, s2, ell = case_inputs("predict", 700, 100, D, False)
    rng = np.random.default_rng(D)
    with G.SGPDevice(len(X), len(Xu), D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(s2, ell, 1e-8, family=family)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[100.0]])
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        for ns in [1, 257, 1000]:
            Xs = rng.uniform(-2.0, 2.0, (ns, D))
            m = dev.predict(Xs)
            mv, v = dev.predict_var(Xs)
            _, vn = dev.predict_var(Xs, noise=True)
            m_ref, v_ref, tol = reference(Xu, Xs, s2, ell, 1e-8, mu, Sig)
            np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())
            np.testing.assert_allclose(mv, m, rtol=0, atol=1e-12 * np.abs(m_ref).max())
            assert np.all(np.abs(v - v_ref) <= tol + 1e-12 * np.abs(v_ref))
            np.testing.assert_allclose(vn, v + 1.0 / 100.0, rtol=1e-12)


# ------------------------------------------------------------------------------------------------
# 4. theta objective and gradient (test_gpu_parity.test_theta_objective_and_gradient_at_fixed_posterior)

@gpu
@pytest.mark.parametrize("family", MATERN)
@pytest.mark.parametrize("iso", [False, True], ids=["ard", "iso"])
def test_theta_objective_and_gradient_match_the_oracle(G, family, iso, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    N, M, D, w, jit = 600, 48, 3, 200.0, 1e-8
    X, Xu, y, _, _, _ = case_inputs("grad", N, M, D, False)
    rng = np.random.default_rng(5)
    ell = np.full(D, 1.9) if iso else np.array([1.4, 2.2, 2.9])
    s2n = 1.05
    elln = np.full(D, 1.8) if iso else ell * rng.uniform(0.9, 1.1, D)
    n_ell = 1 if iso else D
    p0 = np.concatenate([[s2n], elln[:n_ell]])
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(0.9, ell[:n_ell], jit, family=family)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[w]])
        dev.sweep()
        mu0, _, Uv0 = dev.posterior()
        dev.set_kernel(s2n, elln[:n_ell], jit)
        val, grad = dev.theta_objective(want_grad=True, n_ell=n_ell)
    full = lambda p: p[1:] if not iso else np.full(D, p[1])
    f = lambda p: O.theta_objective(Xu, X, y, p[0], full(p), mu0, Uv0, w, jitter=jit)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + n_ell)])
    assert math.isclose(val, f(p0), rel_tol=1e-8), (val, f(p0))
    np.testing.assert_allclose(grad, g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())


# ------------------------------------------------------------------------------------------------
# 5. training (test_gpu_dims.test_streaming_driver_matches_oracle_loop_at_d16 with Matern-5/2)

@gpu
@pytest.mark.parametrize("device_paced", [True, False], ids=["device-paced", "host-paced"])
def test_streaming_driver_with_matern52_matches_the_oracle_loop(G, device_paced, monkeypatch):
    from gaussianprocessnode_amd.train import AdaMax, perform_inference, sigmoid
    monkeypatch.setattr(O, "kernelmatrix", matern("matern52"))
    rng = np.random.default_rng(52)
    N, M, D, bs = 230, 16, 4, 100
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[:M].copy()
    y = np.sin(X.sum(axis=1) / 2.0) + 0.1 * rng.normal(size=N)
    theta0 = O.invsoftplus(np.concatenate([[1.0], np.linspace(2.5, 1.5, D)]))
    w = 50.0
    with G.SGPDevice(bs, M, D) as eng:
        qv, theta = perform_inference(theta0, X, y, Xu, eng, batch_size=bs, epochs=2, w_val=w, optimizer=AdaMax(eta=0.01),
                                      device_paced=device_paced, family="matern52")
    th, opt = theta0.copy(), AdaMax(eta=0.01)
    for _ in range(2):
        mu, Sig = np.zeros(M), 50.0 * np.eye(M)
        for lo in range(0, N, bs):
            xi, yi = X[lo:lo + bs], y[lo:lo + bs]
            p = O.softplus(th)
            r = O.vmp_sweep(Xu, xi, yi, None, p[0], p[1:], w, mu0=mu, Sigma0=Sig)
            mu, Sig = r.mu_v, r.Sigma_v
            f = lambda q: O.theta_objective(Xu, xi, yi, q[0], q[1:], r.mu_v, r.Uv, w)
            g = np.array([(f(p + 1e-6 * e) - f(p - 1e-6 * e)) / 2e-6 for e in np.eye(1 + D)])
            opt.update(th, g * sigmoid(th))
    assert np.abs(theta - theta0).min() > 1e-4
    np.testing.assert_allclose(theta, th, rtol=1e-5, atol=1e-7)
    assert np.linalg.norm(qv.m - mu) / np.linalg.norm(mu) < 1e-5
    assert np.linalg.norm(qv.S - Sig) / np.linalg.norm(Sig) < 1e-5


# ------------------------------------------------------------------------------------------------
# 6. statistics reuse across a change of family; 7. defaults, errors, reproducibility

def _results(dev):
    Psi2, B, sc_data = dev.stats()
    mu, Sig, Uv = dev.posterior()
    s = dev.scalars()
    return [Psi2, B, sc_data, mu, Sig, Uv, np.array([s.sum_I1, s.sum_I2, s.energy, s.logdet_kuu])]


def _bitwise(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _setup(G, X, Xu, y, reuse=False, family=None):
    dev = G.SGPDevice(len(X), len(Xu), X.shape[1], reuse_stats=reuse)
    dev.set_inducing(Xu)
    dev.set_data(X, y)
    dev.set_kernel(0.9, np.linspace(1.5, 3.0, X.shape[1]), 1e-8, family=family)
    dev.set_prior_isotropic(50.0)
    dev.set_noise([[100.0]])
    return dev


@gpu
def test_a_change_of_family_is_not_a_reused_sweep(G):
    from gaussianprocessnode_amd._lib import SGP_SWEEP_FULL
    X, Xu, y, _, _, _ = case_inputs("reuse", 3000, 128, 8, False)
    with _setup(G, X, Xu, y, family="matern52") as fresh:
        fresh.sweep()
        m52 = _results(fresh)
        obj_m52 = fresh.theta_objective()
    with _setup(G, X, Xu, y, reuse=True) as dev:
        dev.sweep()
        se = _results(dev)
        obj_se = dev.theta_objective()
        dev.set_kernel_family("matern52")                         # same theta, same data
        assert dev.theta_objective() != obj_se                    # not the stale value of the SE sweep
        dev.sweep()
        assert dev.sweep_kind()[1] == SGP_SWEEP_FULL
        assert _bitwise(_results(dev), m52)
        assert dev.theta_objective() == obj_m52
        dev.set_kernel_family("se")
        dev.sweep()
        assert dev.sweep_kind()[1] == SGP_SWEEP_FULL
        assert _bitwise(_results(dev), se)


@gpu
def test_default_family_is_se_and_bad_ids_are_refused(G):
    X, Xu, y, _, _, _ = case_inputs("default", 800, 64, 3, False)
    with _setup(G, X, Xu, y) as a, _setup(G, X, Xu, y, family="se") as b:
        a.sweep()
        b.sweep()
        assert _bitwise(_results(a), _results(b))
        for bad in (-1, 4):
            with pytest.raises(G.SGPError):
                a.set_kernel_family(bad)
        with pytest.raises(ValueError):
            a.set_kernel(0.9, [1.0], 0.0, family="matern72")
    with pytest.raises(G.SGPError):
        G.kernelmatrix(X[:3], X[:4], 1.0, [1.0], family=4)


@gpu
def test_family_change_inside_a_training_run_is_refused(G):
    X, Xu, y, _, _, _ = case_inputs("train", 300, 16, 2, False)
    with G.SGPDevice(100, 16, 2) as dev:
        dev.set_inducing(Xu)
        dev.set_noise([[50.0]])
        dev.set_prior_isotropic(50.0)
        dev.set_kernel_family("matern32")
        dev.train_begin(X, y, np.zeros(3))
        with pytest.raises(G.SGPError):
            dev.set_kernel_family("se")
        dev.train_end()


@gpu
@pytest.mark.parametrize("family", MATERN)
def test_matern_sweeps_are_bitwise_reproducible(G, family):
    X, Xu, y, _, _, _ = case_inputs("kin40k-T", 1500, 512, 8, False)
    with _setup(G, X, Xu, y, family=family) as dev:
        dev.sweep()
        first = _results(dev)
        dev.sweep()
        assert _bitwise(_results(dev), first)
    with _setup(G, X, Xu, y, family=family) as dev:
        dev.sweep()
        assert _bitwise(_results(dev), first)


# ------------------------------------------------------------------------------------------------
# 8. two simulated ranks with uneven shards (test_gpu_shards) at Matern-3/2

@gpu
def test_uneven_shards_with_matern32_sweep_to_the_whole_data_posterior(G, monkeypatch):
    from tests.test_gpu_shards import _sharded_run, n_max_of
    monkeypatch.setattr(O, "kernelmatrix", matern("matern32"))
    plain = G.SGPDevice.set_kernel
    monkeypatch.setattr(G.SGPDevice, "set_kernel",
                        lambda self, s2, ell, jitter=0.0, family=None: plain(self, s2, ell, jitter, family="matern32"))
    world, N, M, D = 2, 19585, 512, 8
    r, (X, Xu, y, s2, ell, w) = _sharded_run(G, world, N, M, D, n_max_of(N, world))
    assert all(p == r["plans"][0] for p in r["plans"])
    ref = O.vmp_sweep(Xu, X, y, None, s2, ell, w, jitter=0.0, Lambda0=np.eye(M) / 50.0, xi0=np.zeros(M))
    Psi2, B, scal = r["stats"]
    assert relF(Psi2, ref.stats.Psi2) < 1e-13
    assert relF(B, np.reshape(ref.stats.b, B.shape)) < 1e-13
    tol = post_tol(np.linalg.cond(np.eye(M) / 50.0 + w * ref.stats.Psi2))
    for mu, Sig, Uv in r["posts"]:
        assert relF(mu, ref.mu_v) < tol and relF(Sig, ref.Sigma_v) < tol and relF(Uv, ref.Uv) < tol
    mu0, _, Uv0 = r["posts"][0]
    p0 = np.concatenate([[s2], ell])
    f = lambda p: O.theta_objective(Xu, X, y, p[0], p[1:], mu0, Uv0, w)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + D)])
    np.testing.assert_allclose(r["grad"], g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())
