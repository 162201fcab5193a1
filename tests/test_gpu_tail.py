"""The sweep's tail: mu = P W'^T t is summed block row by block row during the factorisation (mu_row_tile), the Sigma launch adds
the last block row's term and recomputes the alpha scan per tile of Uv (k_gemm32 / uv_cols_role).  The shapes are the smallest at
which that summation can go wrong: no ride-along row at all (T = 1), one and two rows with a padded last tile (T = 2, 3), forming
steps and the role in one launch (T = 8, overlapped), Q = d_out M with and without padding, a dense prior with xi0 != 0.

Reference: oracle.sgp_oracle (vmp_sweep; multi_v_update for d_out > 1, whose Uv is chol(Sigma_v + mu mu^T).U as in v_update).
Bound: the project's min(1e-5, max(1e-9, 20 eps cond(Lambda))) on the relative Frobenius error of mu, Sigma and Uv, and on the
identity Uv^T Uv = Sigma + mu mu^T of the device's own outputs.
"""
import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu

FULL, REUSED = 0, 2


def relF(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def post_tol(cond_L):
    return min(1e-5, max(1e-9, 20 * np.finfo(float).eps * cond_L))


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def synth(N, M, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = rng.uniform(-1.745, 1.745, (M, D))
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    return X, Xu, (y - y.mean()) / y.std()


def check_posterior(mu, Sig, Uv, mu_ref, Sig_ref, Uv_ref, cond_L):
    tol = post_tol(cond_L)
    errs = {"mu": relF(mu, mu_ref), "Sigma": relF(Sig, Sig_ref), "Uv": relF(Uv, Uv_ref),
            "UvTUv": relF(Uv.T @ Uv, Sig + np.outer(mu, mu))}
    print("cond", "%.3g" % cond_L, "tol", "%.3g" % tol, {k: "%.3g" % v for k, v in errs.items()})
    assert np.array_equal(Uv, np.triu(Uv))
    for k, v in errs.items():
        assert v < tol, (k, v, tol)


S2, W = 0.8, 40.0


def uni_sweeps(G, N, M, D, seed, sweeps=1, reuse=False, meancov=None, w_seq=None):
    """`sweeps` sweeps on a fresh handle (w_seq: the noise precision of each); returns inputs and the outputs of every sweep."""
    X, Xu, y = synth(N, M, D, seed)
    ell = np.linspace(1.2, 2.0, D)
    outs = []
    with G.SGPDevice(N, M, D, reuse_stats=reuse) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        dev.set_kernel(S2, ell, 1e-8)
        if meancov is None:
            dev.set_prior_isotropic(50.0)
        else:
            dev.set_prior_meancov(*meancov)
        for i in range(sweeps):
            dev.set_noise([[w_seq[i] if w_seq else W]])
            dev.sweep()
            outs.append(dev.posterior() + (dev.scalars().energy, dev.sweep_kind()[1], dev.overlap_plan()))
    return (X, Xu, y, ell), outs


@pytest.mark.parametrize("N,M,D", [(200, 64, 2), (300, 65, 3), (400, 130, 3)])
def test_one_two_and_three_block_rows_match_the_oracle(G, N, M, D):
    (X, Xu, y, ell), outs = uni_sweeps(G, N, M, D, seed=M)
    ref = O.vmp_sweep(Xu, X, y, None, S2, ell, W, jitter=1e-8, Lambda0=np.eye(M) / 50.0, xi0=np.zeros(M))
    mu, Sig, Uv = outs[0][:3]
    check_posterior(mu, Sig, Uv, ref.mu_v, ref.Sigma_v, ref.Uv, np.linalg.cond(np.eye(M) / 50.0 + W * ref.stats.Psi2))
    # the energy carries 0.5 w sum I1, and sum I1 = s_kk - tr(Kuu^-1 Psi2) cancels: attainable accuracy cond(Kuu) eps s_kk, the
    # bound of test_gpu_parity.test_sweep_matches_oracle
    cond_K = np.linalg.cond(O.kernelmatrix(S2, ell, Xu) + 1e-8 * np.eye(M))
    tol_I1 = 50 * np.finfo(float).eps * cond_K * ref.stats.s_kk + 1e-12
    assert abs(outs[0][3] - ref.energy) <= 1e-6 * abs(ref.energy) + 0.5 * W * tol_I1, (outs[0][3], ref.energy, cond_K)


def test_eight_block_rows_in_overlapped_order_match_the_oracle(G, monkeypatch):
    N, M, D = 3000, 512, 4
    monkeypatch.setenv("SGP_OVERLAP", "1")
    monkeypatch.setenv("SGP_OVERLAP_COLS", "3")
    (X, Xu, y, ell), outs = uni_sweeps(G, N, M, D, seed=8)
    plan = outs[0][5]
    assert len(plan) == 2 and plan[0]["col_end"] == 3          # tile columns 3 .. 7 are formed by a later step than step 0
    ref = O.vmp_sweep(Xu, X, y, None, S2, ell, W, jitter=1e-8, Lambda0=np.eye(M) / 50.0, xi0=np.zeros(M))
    mu, Sig, Uv = outs[0][:3]
    check_posterior(mu, Sig, Uv, ref.mu_v, ref.Sigma_v, ref.Uv, np.linalg.cond(np.eye(M) / 50.0 + W * ref.stats.Psi2))


def test_dense_prior_with_nonzero_xi0_matches_the_oracle(G):
    N, M, D = 400, 130, 3
    rng = np.random.default_rng(3)
    A = rng.normal(size=(M, M))
    Sigma0 = A @ A.T / M + 0.5 * np.eye(M)
    mu0 = rng.normal(size=M)
    (X, Xu, y, ell), outs = uni_sweeps(G, N, M, D, seed=M, meancov=(mu0, Sigma0))
    ref = O.vmp_sweep(Xu, X, y, None, S2, ell, W, jitter=1e-8, mu0=mu0, Sigma0=Sigma0)
    mu, Sig, Uv = outs[0][:3]
    check_posterior(mu, Sig, Uv, ref.mu_v, ref.Sigma_v, ref.Uv, np.linalg.cond(np.linalg.inv(Sigma0) + W * ref.stats.Psi2))


@pytest.mark.parametrize("T,M,Do", [(30, 48, 2), (25, 43, 3)])
def test_multisgp_event_join_and_ragged_q_match_the_oracle(G, T, M, Do):
    rng = np.random.default_rng(T + M)
    Din = 2
    Xu = rng.uniform(-2, 2, (M, Din))
    s2, ell = 0.8, np.array([1.3, 0.9])
    means = rng.normal(size=(T, Din))
    cub = [O.srcubature(means[t], np.diag(rng.uniform(0.02, 0.2, Din))) for t in range(T)]
    pts, wts = np.stack([c[0] for c in cub]), np.stack([c[1] for c in cub])
    S = pts.shape[1]
    Y = rng.normal(size=(T, Do))
    A = rng.normal(size=(Do, Do))
    Wm = A @ A.T + Do * np.eye(Do)
    Q = Do * M
    Lam0, xi0 = np.eye(Q) / 10.0, 0.01 * rng.normal(size=Q)
    ms = O.multi_suff_stats(Xu, pts, wts, Y, None, s2, ell)
    mu_ref, Sig_ref = O.multi_v_update(ms, Wm, Lam0, xi0)
    Uv_ref = np.linalg.cholesky(Sig_ref + np.outer(mu_ref, mu_ref)).T
    with G.SGPDevice(T * S, M, Din, d_out=Do) as dev:
        dev.set_inducing(Xu)
        dev.set_data(pts.reshape(T * S, Din), np.repeat(Y, S, axis=0), None, wts.reshape(-1), n_nodes=T)
        dev.set_kernel(s2, ell, 1e-10)
        dev.set_prior_precision(xi0, Lam0)
        dev.set_noise(Wm, float(np.linalg.slogdet(Wm)[1]))
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
    check_posterior(mu, Sig, Uv, mu_ref, Sig_ref, Uv_ref, np.linalg.cond(np.linalg.inv(Sig_ref)))


def test_sweeps_are_bitwise_reproducible_and_reused_equals_full(G):
    N, M, D = 400, 130, 3
    ws = [W, 55.0]
    _, a = uni_sweeps(G, N, M, D, seed=M, sweeps=2)                       # two consecutive sweeps ...
    _, b = uni_sweeps(G, N, M, D, seed=M, sweeps=1)                       # ... and a fresh handle
    for other in (a[1], b[0]):
        for x, z in zip(a[0][:4], other[:4]):                            # mu, Sigma, Uv, energy
            assert np.array_equal(x, z)
    _, r = uni_sweeps(G, N, M, D, seed=M, sweeps=2, reuse=True, w_seq=ws)
    _, f = uni_sweeps(G, N, M, D, seed=M, sweeps=2, w_seq=ws)
    assert r[1][4] == REUSED and f[1][4] == FULL
    for x, z in zip(r[1][:4], f[1][:4]):
        assert np.array_equal(x, z)
