"""Input dimensions outside {1, 2, 3, 4, 8}: every D-dependent entry point against the oracle for D up to MAXD = 32 -- the generic
Gram kernel k_gram_uf<MAXD> (D > 8), the generic prediction kernel k_predict<0> (D = 5, 6, 7, 9..32), the K_uu Gram kernels and
the theta-gradient kernels with up to 33 gradient slots, k_kernelmatrix, and the device-paced optimiser with 17 raw parameters.

The fixtures are built so that the comparisons can fail: the lengthscales grow with sqrt(D) (inputs U(-1.745, 1.745) would
otherwise drive every kernel value to 0 at large D), every dimension has its own lengthscale and the last one the shortest.
test_fixtures_are_discriminating (CPU only) proves with the oracle that dropping a dimension, dropping every dimension >= 8 or
swapping two lengthscales moves Psi2 and mu by at least 100 times the bounds the GPU tests apply."""
import math

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests.test_gpu_parity import kuu_tol, post_tol, relF
from tests.test_gpu_predict_var import reference as predict_reference

gpu = pytest.mark.gpu
DIMS = [5, 7, 9, 16, 31, 32]
S2, W, JIT, PSI2_TOL = 0.9, 100.0, 1e-8, 1e-13


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def lengthscales(D):
    """Distinct per dimension, the shortest on the last one, scaled with sqrt(D) (the D = 8 tests' 1.5 .. 3.0 at D = 8)."""
    return math.sqrt(D / 8.0) * np.linspace(3.0, 1.5, D)


def iso_lengthscale(D):
    return math.sqrt(D / 8.0) * 2.0


def synth(N, M, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.745, 1.745, (N, D))
    pool = X if N >= M else rng.uniform(-1.745, 1.745, (M, D))
    Xu = pool[rng.permutation(len(pool))[:M]].copy()
    y = np.sin(X.sum(axis=1) / math.sqrt(D)) + 0.1 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    return X, Xu, y


def oracle_sweep(Xu, X, y, ell):
    M = len(Xu)
    return O.vmp_sweep(Xu, X, y, None, S2, ell, W, E_logw=math.log(W) - 0.01, jitter=JIT, Lambda0=np.eye(M) / 50.0,
                       xi0=np.zeros(M))


# ------------------------------------------------------------------------------------------------
# the sweep: statistics, K_uu factor, posterior, scalars, per-point :w quantities and the theta objective
# (the bounds of test_gpu_parity.test_sweep_matches_oracle)

def check_sweep(G, N, M, D, iso, seed):
    X, Xu, y = synth(N, M, D, seed)
    ell_dev = np.array([iso_lengthscale(D)]) if iso else lengthscales(D)
    ell = np.full(D, ell_dev[0]) if iso else ell_dev
    E_logw = math.log(W) - 0.01
    with G.SGPDevice(N, M, D, keep_kuf=True) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(S2, ell_dev, JIT)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[W]], E_logw)
        dev.sweep()
        Psi2, B, sc_data = dev.stats()
        KuuL = dev.kuu_chol()
        mu, Sig, Uv = dev.posterior()
        sc = dev.scalars()
        I1, I2 = dev.w_stats()
        obj = dev.theta_objective()
    ref = oracle_sweep(Xu, X, y, ell)
    assert relF(Psi2, ref.stats.Psi2) < PSI2_TOL, relF(Psi2, ref.stats.Psi2)
    assert relF(B, np.reshape(ref.stats.b, B.shape)) < PSI2_TOL
    assert math.isclose(sc_data[0], ref.stats.s_yy[0, 0], rel_tol=1e-13)
    assert sc_data[1] == N and sc_data[2] == N
    Kuu = O.kernelmatrix(S2, ell, Xu) + JIT * np.eye(M)
    cond_K = np.linalg.cond(Kuu)
    assert relF(KuuL, ref.KuuL) < kuu_tol(cond_K), (relF(KuuL, ref.KuuL), cond_K)
    cond_L = np.linalg.cond(np.eye(M) / 50.0 + W * ref.stats.Psi2)
    tol_post = post_tol(cond_L)
    assert relF(mu, ref.mu_v) < tol_post, (relF(mu, ref.mu_v), cond_L)
    assert relF(Sig, ref.Sigma_v) < tol_post, (relF(Sig, ref.Sigma_v), cond_L)
    assert relF(Uv, ref.Uv) < tol_post
    tol_I1 = 50 * np.finfo(float).eps * cond_K * ref.stats.s_kk + 1e-12
    assert abs(sc.sum_I1 - ref.sum_I1) <= tol_I1
    assert math.isclose(sc.sum_I2, ref.sum_I2, rel_tol=max(1e-7, tol_post))
    assert abs(sc.energy - ref.energy) <= max(1e-7, tol_post) * abs(ref.energy) + 0.5 * W * tol_I1
    assert sc.info_kuu == 0 and sc.info_lambda == 0
    assert math.isclose(sc.logdet_kuu, 2 * np.log(np.diag(ref.KuuL)).sum(), rel_tol=1e-9, abs_tol=1e-7)
    rI1, rI2 = O.w_stats_perpoint(Xu, X, y, None, S2, ell, ref.KuuL, ref.mu_v, ref.Uv)
    np.testing.assert_allclose(I1, rI1, rtol=0, atol=tol_I1 / N + 1e-12)
    scale_I2 = float(np.max(y * y + np.sum((ref.Uv @ O.kernelmatrix(S2, ell, Xu, X)) ** 2, axis=0)))
    np.testing.assert_allclose(I2, rI2, rtol=1e-6, atol=max(1e-9, tol_post * scale_I2))
    ref_obj = O.theta_objective(Xu, X, y, S2, ell, ref.mu_v, ref.Uv, W, jitter=JIT)
    assert abs(obj - ref_obj) <= 1e-7 * abs(ref_obj) + 0.5 * W * tol_I1


# (N, M) per size: small = points x lower tiles < 10 000 (k_gram_uu, k_syrk_stream), gated = >= 10 000 (k_gram_uu_lds,
# k_syrk_direct; lower tiles = 3 at M = 128)
SIZES = {"small": (700, 100), "gated": (4000, 128)}


@gpu
@pytest.mark.parametrize("kern", ["ard", "iso"])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("D", DIMS)
def test_sweep_matches_oracle(G, D, size, kern):
    N, M = SIZES[size]
    check_sweep(G, N, M, D, kern == "iso", seed=100 * D + M)


@gpu
@pytest.mark.parametrize("N", [3333, 3334])
def test_sweep_straddling_the_gate_at_d32(G, N):
    """M = 128 (three lower tiles): 3 333 points are 9 999 < 10 000, the small path; 3 334 are 10 002, the gated path."""
    check_sweep(G, N, 128, 32, False, seed=N)


@gpu
@pytest.mark.parametrize("M", [63, 65, 129])
def test_sweep_at_ragged_m(G, M):
    check_sweep(G, 700, M, 9, False, seed=M)


# ------------------------------------------------------------------------------------------------
# theta gradient (33 slots at D = 32): the analytic device gradient against central differences of the oracle's objective
# (test_gpu_parity.test_theta_objective_and_gradient_at_fixed_posterior)

@gpu
@pytest.mark.parametrize("D,iso,weighted", [(9, False, False), (9, True, False), (16, False, False), (16, True, False),
                                            (32, False, False), (32, True, False), (32, False, True)])
def test_theta_gradient_matches_oracle(G, D, iso, weighted):
    N, M = 600, 48
    rng = np.random.default_rng(N + D)
    X, Xu, y = synth(N, M, D, seed=13 + D)
    w = 200.0
    ell = np.full(D, iso_lengthscale(D)) if iso else lengthscales(D)
    om = rng.integers(1, 4, N).astype(np.float64) if weighted else None
    s2n = 1.05
    elln = np.full(D, 0.95 * iso_lengthscale(D)) if iso else ell * rng.uniform(0.9, 1.1, D)
    n_ell = 1 if iso else D
    p0 = np.concatenate([[s2n], elln[:n_ell]])
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y, weights=om)
        dev.set_kernel(S2, ell[:n_ell], JIT)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[w]])
        dev.sweep()
        mu0, _, Uv0 = dev.posterior()
        dev.set_kernel(s2n, elln[:n_ell], JIT)
        val, grad = dev.theta_objective(want_grad=True, n_ell=n_ell)

        def f_dev(p):
            dev.set_kernel(p[0], p[1:], JIT)
            return dev.theta_objective(want_grad=False, n_ell=n_ell)
        g_dev = np.array([(f_dev(p0 + 1e-5 * e) - f_dev(p0 - 1e-5 * e)) / 2e-5 for e in np.eye(1 + n_ell)])
    assert len(grad) == 1 + n_ell
    np.testing.assert_allclose(grad, g_dev, rtol=5e-5, atol=1e-6 * np.abs(g_dev).max())
    full = lambda p: p[1:] if not iso else np.full(D, p[1])
    # integer point weights are repeated points: the oracle's objective of the repeated data set is the weighted objective
    Xr, yr = (np.repeat(X, om.astype(int), axis=0), np.repeat(y, om.astype(int))) if weighted else (X, y)
    f = lambda p: O.theta_objective(Xu, Xr, yr, p[0], full(p), mu0, Uv0, w, jitter=JIT)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + n_ell)])
    assert math.isclose(val, f(p0), rel_tol=1e-8), (val, f(p0))
    np.testing.assert_allclose(grad, g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())


# ------------------------------------------------------------------------------------------------
# prediction: sgp_predict (k_predict<0> for D = 5, 6, 7, 9..32) and sgp_predict_var (k_gram_uf<MAXD> for D > 8) against the
# reference of test_gpu_predict_var.py; k_kernelmatrix

@gpu
@pytest.mark.parametrize("D", [5, 6, 7, 9, 32])
def test_predict_and_predict_var_match_the_reference(G, D):
    N, M = 700, 100
    X, Xu, y = synth(N, M, D, seed=7 * D)
    ell = lengthscales(D)
    rng = np.random.default_rng(D)
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(S2, ell, JIT)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[W]])
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        for ns in [1, 255, 257, 1000]:
            Xs = rng.uniform(-2.0, 2.0, (ns, D))
            m = dev.predict(Xs)
            mv, v = dev.predict_var(Xs)
            m_ref, v_ref, tol = predict_reference(Xu, Xs, S2, ell, JIT, mu, Sig)
            assert m.shape == mv.shape == v.shape == (ns,)
            np.testing.assert_allclose(m, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())
            np.testing.assert_allclose(m, O.predict_mean(Xu, Xs, mu, S2, ell), rtol=0, atol=1e-9 * np.abs(m_ref).max())
            np.testing.assert_allclose(mv, m_ref, rtol=0, atol=1e-9 * np.abs(m_ref).max())
            assert np.all(np.abs(v - v_ref) <= tol), (ns, (np.abs(v - v_ref) / tol).max())


@gpu
@pytest.mark.parametrize("D", [5, 9, 32])
def test_kernelmatrix_matches_oracle(G, D):
    rng = np.random.default_rng(D)
    for na, nb in [(1, 1), (7, 13), (257, 64)]:
        A, B = rng.uniform(-1.745, 1.745, (na, D)), rng.uniform(-1.745, 1.745, (nb, D))
        K = G.kernelmatrix(A, B, 0.37, lengthscales(D))
        np.testing.assert_allclose(K, O.kernelmatrix(0.37, lengthscales(D), A, B), rtol=1e-13, atol=1e-300)
        K1 = G.kernelmatrix(A, B, 2.0, [iso_lengthscale(D)])
        np.testing.assert_allclose(K1, O.kernelmatrix(2.0, iso_lengthscale(D), A, B), rtol=1e-13, atol=1e-300)


# ------------------------------------------------------------------------------------------------
# MultiSGP at input dimensions 9 and 32 (test_gpu_parity.test_multisgp_sweep_matches_oracle's checks)

@gpu
@pytest.mark.parametrize("Din,T,M,Do", [(9, 30, 48, 2), (32, 40, 65, 3)])
def test_multisgp_sweep_matches_oracle(G, Din, T, M, Do):
    rng = np.random.default_rng(Din + T)
    Xu = rng.uniform(-1.745, 1.745, (M, Din))
    s2, ell = 0.8, lengthscales(Din)
    means = rng.uniform(-1.5, 1.5, (T, Din))
    covs = [np.diag(rng.uniform(0.02, 0.2, Din)) for _ in range(T)]
    cub = [O.srcubature(means[t], covs[t]) for t in range(T)]
    pts = np.stack([c[0] for c in cub])
    wts = np.stack([c[1] for c in cub])
    S = pts.shape[1]
    Y = rng.normal(size=(T, Do))
    Sig_y = np.stack([np.diag(rng.uniform(0.01, 0.1, Do)) for _ in range(T)])
    A = rng.normal(size=(Do, Do))
    Wm = A @ A.T + Do * np.eye(Do)
    E_logdetW = float(np.linalg.slogdet(Wm)[1]) - 0.1
    Q = Do * M
    Lam0 = np.eye(Q) / 10.0
    xi0 = 0.01 * rng.normal(size=Q)
    ms = O.multi_suff_stats(Xu, pts, wts, Y, Sig_y, s2, ell)
    mu_ref, Sig_ref = O.multi_v_update(ms, Wm, Lam0, xi0)
    Kinv = O.cholinv(O.kernelmatrix(s2, ell, Xu) + 1e-10 * np.eye(M))
    S_ref = O.multi_w_update(ms, mu_ref, Sig_ref, Kinv)
    U_ref = 0.0
    for t in range(T):
        P0, P1, P2 = O.psi_statistics(Xu, pts[t], wts[t], s2, ell)
        U_ref += O.multi_average_energy(P0, P1, P2, Y[t], Sig_y[t], mu_ref, Sig_ref, Wm, E_logdetW, Kinv)
    with G.SGPDevice(T * S, M, Din, d_out=Do) as dev:
        dev.set_inducing(Xu)
        dev.set_data(pts.reshape(T * S, Din), np.repeat(Y, S, axis=0), None, wts.reshape(-1), n_nodes=T)
        dev.set_output_cov_sum(Sig_y.sum(axis=0))
        dev.set_kernel(s2, ell, 1e-10)
        dev.set_prior_precision(xi0, Lam0)
        dev.set_noise(Wm, E_logdetW)
        dev.sweep()
        Psi2, B, sc = dev.stats()
        mu, Sig, Uv = dev.posterior()
        Sw = dev.wishart_invscale()
        energy = dev.scalars().energy
    assert relF(Psi2, ms.Psi2) < 1e-12 and relF(B, ms.B) < 1e-12
    assert sc[2] == T and math.isclose(sc[1], T, rel_tol=1e-12)
    assert relF(mu, mu_ref) < 1e-8 and relF(Sig, Sig_ref) < 1e-8
    np.testing.assert_allclose(Uv.T @ Uv, Sig_ref + np.outer(mu_ref, mu_ref), rtol=1e-7, atol=1e-10)
    Kuu = O.kernelmatrix(s2, ell, Xu) + 1e-10 * np.eye(M)
    tol_I1 = 50 * np.finfo(float).eps * np.linalg.cond(Kuu) * s2 * T
    assert np.abs(Sw - S_ref).max() <= 1e-7 * np.abs(S_ref).max() + tol_I1, (Sw, S_ref)
    off = ~np.eye(Do, dtype=bool)
    np.testing.assert_allclose(Sw[off], S_ref[off], rtol=1e-7, atol=1e-9)
    assert abs(energy - U_ref) <= 1e-7 * abs(U_ref) + 0.5 * np.trace(Wm) * tol_I1, (energy, U_ref)


# ------------------------------------------------------------------------------------------------
# training at D = 16, ARD: 17 raw parameters through k_train_adamax / TrainState (device-paced) and the host-paced loop,
# against the oracle loop (test_gpu_rules.test_streaming_driver_matches_oracle_loop)

@gpu
@pytest.mark.parametrize("device_paced", [True, False])
def test_streaming_driver_matches_oracle_loop_at_d16(G, device_paced):
    from gaussianprocessnode_amd.train import AdaMax, perform_inference, sigmoid
    rng = np.random.default_rng(16)
    N, M, D, bs = 230, 16, 16, 100
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[:M].copy()
    y = np.sin(X.sum(axis=1) / math.sqrt(D)) + 0.1 * rng.normal(size=N)
    theta0 = O.invsoftplus(np.concatenate([[1.0], lengthscales(D)]))
    w = 50.0
    with G.SGPDevice(bs, M, D) as eng:
        qv, theta = perform_inference(theta0, X, y, Xu, eng, batch_size=bs, epochs=2, w_val=w, optimizer=AdaMax(eta=0.01),
                                      device_paced=device_paced)
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
    assert len(theta) == 1 + D
    assert np.abs(theta - theta0).min() > 1e-4                 # every raw parameter moved
    np.testing.assert_allclose(theta, th, rtol=1e-5, atol=1e-7)
    assert np.linalg.norm(qv.m - mu) / np.linalg.norm(mu) < 1e-5
    assert np.linalg.norm(qv.S - Sig) / np.linalg.norm(Sig) < 1e-5


@gpu
def test_create_accepts_d32_and_refuses_d33(G):
    with G.SGPDevice(10, 8, 32) as dev:
        assert dev.D == 32
    with pytest.raises(G.SGPError):
        G.SGPDevice(10, 8, 33)


# ------------------------------------------------------------------------------------------------
# CPU only: the fixtures above can fail

def _sensitivity(N, M, D, seed):
    """Relative changes of Psi2 and mu under each perturbation, the GPU bounds they must beat, and the median K_uf entry."""
    X, Xu, y = synth(N, M, D, seed)
    ell = lengthscales(D)
    ref = oracle_sweep(Xu, X, y, ell)
    tol_post = post_tol(np.linalg.cond(np.eye(M) / 50.0 + W * ref.stats.Psi2))
    perturbed = {}
    for d in range(D):                                       # a kernel that ignores dimension d: an infinite lengthscale there
        e = ell.copy(); e[d] = np.inf
        perturbed[f"drop {d}"] = e
    if D > 8:
        e = ell.copy(); e[8:] = np.inf
        perturbed["drop >= 8"] = e
    for a, b in [(0, D - 1), (D - 2, D - 1), (7, 8)] if D > 8 else [(0, D - 1), (D - 2, D - 1)]:
        e = ell.copy(); e[[a, b]] = e[[b, a]]
        perturbed[f"swap {a} {b}"] = e
    out = {}
    for k, e in perturbed.items():
        r = oracle_sweep(Xu, X, y, e)
        out[k] = (relF(r.stats.Psi2, ref.stats.Psi2), relF(r.mu_v, ref.mu_v))
    return out, (PSI2_TOL, tol_post), float(np.median(O.kernelmatrix(S2, ell, Xu, X)))


@pytest.mark.parametrize("D", DIMS)
def test_fixtures_are_discriminating(D):
    """Each perturbation a subtly wrong kernel would make (a dimension dropped, the dimensions >= 8 dropped, two lengthscales
    swapped) moves Psi2 and mu by >= 100 x the bound the GPU sweep test applies, at the small and the D = 32 straddle sizes;
    kernel values stay far from 0."""
    cases = [(*SIZES["small"], 100 * D + SIZES["small"][1])] + ([(3333, 128, 3333)] if D == 32 else [])
    for N, M, seed in cases:
        out, (tol_psi2, tol_mu), med = _sensitivity(N, M, D, seed)
        assert med > 1e-3, med
        weak = {k: v for k, v in out.items() if v[0] < 100 * tol_psi2 or v[1] < 100 * tol_mu}
        assert not weak, (N, M, tol_psi2, tol_mu, weak)
