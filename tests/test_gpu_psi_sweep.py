"""sgp_sweep_local_psi + sgp_sweep_finish against oracle.sgp_oracle's update functions fed the restatement's statistics
(tests/psi_stats_ref.py), with the bounds tests/test_gpu_parity.py and tests/test_gpu_tail.py use for the same quantities: 1e-13 on
Psi2 / B (relative to the largest entry), min(1e-5, max(1e-9, 20 eps cond(Lambda))) on mu_v, Sigma_v and Uv (relative Frobenius),
50 eps cond(K_uu) s_kk + 1e-12 on sum I1 and what follows from it for the energy and the Wishart inverse scale.
"""
import math

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import psi_stats_ref as R

pytestmark = pytest.mark.gpu

S2, JIT = 0.8, 1e-8
SHAPES = [(1, 20, 1, 50), (2, 48, 2, 12), (2, 48, 2, 300), (4, 65, 3, 65)]      # d_out, M, D, T


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def relF(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def post_tol(cond_L):
    return min(1e-5, max(1e-9, 20 * np.finfo(float).eps * cond_L))


def problem(d_out, M, D, T, zero_cov=False):
    rng = np.random.default_rng(1000 * d_out + M + T)
    Xu = rng.uniform(-2.0, 2.0, (M, D))
    ell = np.linspace(1.1, 1.7, D)
    mean = rng.uniform(-2.0, 2.0, (T, D))
    A = rng.normal(size=(T, D, D)) * 0.4
    S = np.zeros((T, D, D)) if zero_cov else A @ A.transpose(0, 2, 1) + 0.01 * np.eye(D)
    Y = rng.normal(size=(T, d_out))
    B = rng.normal(size=(d_out, d_out))
    W = B @ B.T + d_out * np.eye(d_out) if d_out > 1 else np.array([[12.0]])
    return Xu, ell, mean, S, Y, W


def setup(dev, Xu, ell, W):
    Q = dev.Q
    dev.set_inducing(Xu)
    dev.set_kernel(S2, ell, JIT)
    dev.set_noise(W, float(np.linalg.slogdet(W)[1]))
    dev.set_prior_precision(np.zeros(Q), np.eye(Q) / 10.0)


def results(dev):
    return dev.stats() + dev.posterior() + (dev.scalars(), dev.wishart_invscale() if dev.d_out > 1 else None)


def y_variances(d_out, T):
    """var(q_out) per node for the single-output shape (the classification rules' targets); none for d_out > 1"""
    return np.random.default_rng(T).uniform(0.1, 0.5, T) if d_out == 1 else None


def exact_sweep(G, d_out, M, D, T, zero_cov=False, cov_sum=None, y_var=None):
    Xu, ell, mean, S, Y, W = problem(d_out, M, D, T, zero_cov)
    with G.SGPDevice(T, M, D, d_out=d_out) as dev:
        setup(dev, Xu, ell, W)
        dev.sweep_local_psi(mean, S, Y, y_var)
        if cov_sum is not None:
            dev.set_output_cov_sum(cov_sum)
        dev.sweep_finish()
        return (Xu, ell, mean, S, Y, W), results(dev)


@pytest.mark.parametrize("d_out,M,D,T", SHAPES)
def test_exact_sweep_matches_the_oracle_on_the_restated_statistics(G, d_out, M, D, T):
    cov_sum = None if d_out == 1 else 0.3 * np.eye(d_out)
    y_var = y_variances(d_out, T)
    (Xu, ell, mean, S, Y, W), (Psi2, B, sc, mu, Sig, Uv, scal, wish) = exact_sweep(G, d_out, M, D, T, cov_sum=cov_sum, y_var=y_var)
    uni, multi = R.exact_suff_stats(Xu, S2, ell, mean, S, Y, y_var=y_var, cov_sum=cov_sum)
    e2, eb = rel_max(Psi2, uni.Psi2), rel_max(B, uni.b)
    print(f"psi sweep d_out={d_out} M={M} D={D} T={T}: Psi2 {e2:.3g} B {eb:.3g}")
    assert e2 < 1e-13 and eb < 1e-13
    assert np.array_equal(Psi2, Psi2.T)
    assert sc[1] == T and sc[2] == T
    Q = d_out * M
    Lam0, xi0 = np.eye(Q) / 10.0, np.zeros(Q)
    Kuu, L = O.kuu_and_chol(Xu, S2, ell, JIT)
    cond_K = np.linalg.cond(Kuu)
    tol_I1 = 50 * np.finfo(float).eps * cond_K * uni.s_kk + 1e-12
    if d_out == 1:
        assert math.isclose(sc[0], uni.s_yy[0, 0], rel_tol=1e-13)
        ref = O.vmp_sweep(Xu, None, None, None, S2, ell, W[0, 0], jitter=JIT, Lambda0=Lam0, xi0=xi0, stats=uni)
        mu_ref, Sig_ref, Uv_ref = ref.mu_v, ref.Sigma_v, ref.Uv
    else:
        mu_ref, Sig_ref = O.multi_v_update(multi, W, Lam0, xi0)
        Uv_ref = np.linalg.cholesky(Sig_ref + np.outer(mu_ref, mu_ref)).T
    tol = post_tol(np.linalg.cond(Lam0 + np.kron(W, uni.Psi2)))
    errs = {"mu": relF(mu, mu_ref), "Sigma": relF(Sig, Sig_ref), "Uv": relF(Uv, Uv_ref)}
    print("   tol %.3g" % tol, {k: "%.3g" % v for k, v in errs.items()})
    assert all(v < tol for v in errs.values()), (errs, tol)
    assert scal.info_kuu == 0 and scal.info_lambda == 0
    if d_out == 1:
        assert abs(scal.sum_I1 - ref.sum_I1) <= tol_I1
        assert math.isclose(scal.sum_I2, ref.sum_I2, rel_tol=max(1e-7, tol))
        assert abs(scal.energy - ref.energy) <= max(1e-7, tol) * abs(ref.energy) + 0.5 * W[0, 0] * tol_I1
    else:
        # MultiSGP: sum I1 = s_kk - tr(Kuu^-1 Psi2) as for d_out = 1; the second scalar is not defined there (the device reports 0,
        # its content is the Wishart inverse scale); the energy is the sum over the nodes of GPnode/MultiSGPnode.jl:544-632,
        # 1/2 (tr(W sum_t (I1_t + I2_t)) - T E[logdet W] + T d_out log 2 pi), with the bounds tests/test_gpu_envelope.py uses
        Kinv = np.linalg.inv(Kuu)
        wish_ref = O.multi_w_update(multi, mu_ref, Sig_ref, Kinv)
        energy_ref = 0.5 * (np.trace(W @ wish_ref) - T * np.linalg.slogdet(W)[1] + T * d_out * math.log(2 * math.pi))
        sum_I1_ref = multi.s_kk - np.sum(Kinv * multi.Psi2)
        print("   sum_I1 %.3g (tol %.3g) energy %.3g wishart %.3g" % (abs(scal.sum_I1 - sum_I1_ref), tol_I1,
              abs(scal.energy - energy_ref) / abs(energy_ref), np.max(np.abs(wish - wish_ref)) / np.max(np.abs(wish_ref))))
        assert abs(scal.sum_I1 - sum_I1_ref) <= tol_I1 and scal.sum_I2 == 0.0
        assert np.max(np.abs(wish - wish_ref)) <= max(1e-7, tol) * np.max(np.abs(wish_ref)) + tol_I1, (wish, wish_ref)
        assert abs(scal.energy - energy_ref) <= max(1e-7, tol) * abs(energy_ref) + 0.5 * np.trace(W) * tol_I1


@pytest.mark.parametrize("d_out,M,D,T", SHAPES)
def test_zero_covariances_equal_an_ordinary_sweep_over_the_means(G, d_out, M, D, T):
    (Xu, ell, mean, S, Y, W), ex = exact_sweep(G, d_out, M, D, T, zero_cov=True)
    with G.SGPDevice(T, M, D, d_out=d_out) as dev:
        setup(dev, Xu, ell, W)
        dev.set_data(mean, Y)
        dev.sweep()
        pt = results(dev)
    assert rel_max(ex[0], pt[0]) < 1e-13 and rel_max(ex[1], pt[1]) < 1e-13
    assert np.allclose(ex[2][:3], pt[2][:3], rtol=1e-13)
    tol = post_tol(np.linalg.cond(np.eye(d_out * M) / 10.0 + np.kron(W, pt[0])))
    for a, b in zip(ex[3:6], pt[3:6]):
        assert relF(a, b) < tol
    assert math.isclose(ex[6].energy, pt[6].energy, rel_tol=1e-6, abs_tol=1e-6)


def test_follow_up_calls_are_refused_and_set_data_restores_the_handle(G):
    d_out, M, D, T = 1, 20, 1, 50
    Xu, ell, mean, S, Y, W = problem(d_out, M, D, T)
    rng = np.random.default_rng(0)
    X, y = rng.normal(size=(40, D)), rng.normal(size=40)
    text = "exact Psi-statistics (sgp_sweep_local_psi)"

    def plain(dev):
        dev.set_data(X, y)
        dev.sweep()
        return dev.stats() + dev.posterior() + (dev.scalars().energy,)

    with G.SGPDevice(T, M, D, keep_kuf=True) as dev:
        setup(dev, Xu, ell, W)
        dev.sweep_local_psi(mean, S, Y[:, 0])
        dev.sweep_finish()
        for call in (dev.w_stats, dev.theta_objective, lambda: dev.theta_descend(np.zeros(2), 1),
                     lambda: dev.set_targets(np.zeros(T))):
            with pytest.raises(G.SGPError) as ei:
                call()
            assert "status -1" in str(ei.value) and text in str(ei.value), str(ei.value)
        with pytest.raises(G.SGPError) as ei:
            dev.sweep()
        assert "set_data" in str(ei.value)
        after = plain(dev)
        assert dev.sweep_kind()[1] == 0
    with G.SGPDevice(T, M, D, keep_kuf=True) as dev:
        setup(dev, Xu, ell, W)
        fresh = plain(dev)
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)


def test_hook_family_and_indefinite_node_are_refused(G):
    d_out, M, D, T = 1, 20, 1, 50
    Xu, ell, mean, S, Y, W = problem(d_out, M, D, T)
    with G.SGPDevice(T, M, D) as dev:
        setup(dev, Xu, ell, W)
        dev.set_allreduce(lambda buf, count, stream: 0)
        with pytest.raises(G.SGPError) as ei:
            dev.sweep_local_psi(mean, S, Y[:, 0])
        assert "status -1" in str(ei.value) and "all-reduce hook" in str(ei.value)
        dev.set_allreduce(None)
        nan_mean = mean.copy()
        nan_mean[3, 0] = np.nan
        inf_cov = S.copy()
        inf_cov[2, 0, 0] = np.inf
        for args, text in (((nan_mean, S, Y[:, 0]), "mean must be finite"), ((mean, inf_cov, Y[:, 0]), "cov must be finite")):
            with pytest.raises(G.SGPError) as ei:
                dev.sweep_local_psi(*args)
            assert "status -1" in str(ei.value) and text in str(ei.value)
        dev.set_kernel_family("matern52")
        with pytest.raises(G.SGPError) as ei:
            dev.sweep_local_psi(mean, S, Y[:, 0])
        assert "status -1" in str(ei.value) and "SGP_KERNEL_SE only" in str(ei.value)
        dev.set_kernel_family("se")
        bad = S.copy()
        bad[7] = -10.0
        with pytest.raises(G.PosDefException) as ei:
            dev.sweep_local_psi(mean, bad, Y[:, 0])
        assert ei.value.info == 8 and "node 7" in str(ei.value)
        with pytest.raises(G.SGPError):
            dev.sweep_finish()
        dev.sweep_local_psi(mean, S, Y[:, 0])
        dev.sweep_finish()
        assert np.all(np.isfinite(dev.posterior()[0]))


def test_unset_kernel_training_run_and_y_var_with_outputs_are_refused(G):
    Xu, ell, mean, S, Y, W = problem(2, 20, 1, 50)
    with G.SGPDevice(50, 20, 1, d_out=2) as dev:
        dev.set_inducing(Xu)
        with pytest.raises(G.SGPError) as ei:
            dev.sweep_local_psi(mean, S, Y)
        assert "status -1" in str(ei.value) and "set_inducing and set_kernel first" in str(ei.value)
        setup(dev, Xu, ell, W)
        with pytest.raises(G.SGPError) as ei:
            dev.sweep_local_psi(mean, S, Y, np.ones(50))
        assert "status -1" in str(ei.value) and "y_var is only defined for d_out = 1" in str(ei.value)
    with G.SGPDevice(50, 20, 1) as dev:
        setup(dev, Xu, ell, np.array([[12.0]]))
        dev.train_begin(mean, Y[:, 0], np.zeros(2))
        with pytest.raises(G.SGPError) as ei:
            dev.sweep_local_psi(mean, S, Y[:, 0])
        assert "status -1" in str(ei.value) and "a device-paced training run is open" in str(ei.value)
        dev.train_end()


def test_a_failed_call_leaves_the_handles_data_in_place(G):
    """An indefinite node is found before the handle's state is touched: the resident data and the next sweep are those of a
    handle that never made the call."""
    Xu, ell, mean, S, Y, W = problem(1, 20, 1, 50)
    rng = np.random.default_rng(1)
    X, y = rng.normal(size=(40, 1)), rng.normal(size=40)
    bad = S.copy()
    bad[7] = -10.0
    outs = []
    for fail in (False, True):
        with G.SGPDevice(50, 20, 1) as dev:
            setup(dev, Xu, ell, W)
            dev.set_data(X, y)
            dev.sweep()
            if fail:
                with pytest.raises(G.PosDefException):
                    dev.sweep_local_psi(mean, bad, Y[:, 0])
            dev.set_noise([[9.0]])
            dev.sweep()
            outs.append(dev.stats() + dev.posterior() + (dev.scalars().energy,))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_psi_stats_uses_the_posterior_of_an_exact_sweep_when_mu_v_is_null(G):
    Xu, ell, mean, S, Y, W = problem(2, 48, 2, 12)
    with G.SGPDevice(12, 48, 2, d_out=2) as dev:
        setup(dev, Xu, ell, W)
        dev.sweep_local_psi(mean, S, Y)
        dev.sweep_finish()
        mu = dev.posterior()[0]
        implicit = dev.psi_stats(mean, S, want_out=True)
        explicit = dev.psi_stats(mean, S, None, mu, want_out=True)
    for a, b in zip(implicit, explicit):
        assert np.array_equal(a, b)
    ref = np.stack([implicit[0] @ mu[d * 48:(d + 1) * 48] for d in range(2)], axis=1)
    assert rel_max(implicit[2], ref) < 1e-13


def test_the_node_rules_return_the_exact_statistics_results(G):
    """multisgp.rule_v / rule_out / rule_out_batch and UniSGP's uncertain-input :v / :out pair with meta.method = ExactSE()
    against the restatement: Psi1, Psi2 of the node, Psi1' mu_v^(d), and the q(v) of the N-fold product."""
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd import unisgp as U
    from gaussianprocessnode_amd.cubature import ExactSE
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, NormalMeanVariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel, UniSGPMeta
    rng = np.random.default_rng(8)
    M, D, d_out = 9, 2, 2
    Xu, theta = rng.uniform(-2, 2, (M, D)), np.array([0.8, 1.1, 0.9])
    q_theta = PointMass(theta)
    meta = MultiSGPMeta(ExactSE(), Xu, None, None, None, None, SEARDKernel(), jitter=1e-8)
    A = rng.normal(size=(3, D, D)) * 0.4
    q_ins = [MvNormalMeanCovariance(rng.normal(size=D), A[t] @ A[t].T + 0.01 * np.eye(D)) for t in range(2)] + [PointMass(rng.normal(size=D))]
    covs = [q_ins[0].S, q_ins[1].S, np.zeros((D, D))]
    means = [np.asarray(q.mean()) for q in q_ins]
    mu_v = rng.normal(size=d_out * M)
    q_v = MvNormalMeanCovariance(mu_v, np.eye(d_out * M))
    Wm = np.array([[3.0, 0.5], [0.5, 2.0]])
    q_w = PointMass(Wm)
    try:
        q_out = PointMass(np.array([0.3, -0.7]))
        msg = MS.rule_v(q_out, q_ins[0], q_w, q_theta, meta)
        p1, p2 = R.psi1_node(Xu, theta[0], theta[1:], means[0], covs[0]), R.psi2_node(Xu, theta[0], theta[1:], means[0], covs[0])
        row = q_out.value @ Wm
        assert rel_max(msg.W, np.kron(Wm, p2)) < 1e-13 and rel_max(msg.xi, np.concatenate([p1 * row[d] for d in range(d_out)])) < 1e-13
        batch = MS.rule_out_batch(q_ins, q_v, q_w, q_theta, meta)
        for t in range(3):
            ref = mu_v.reshape(d_out, M) @ R.psi1_node(Xu, theta[0], theta[1:], means[t], covs[t])
            one = MS.rule_out(q_ins[t], q_v, q_w, q_theta, meta)
            assert rel_max(batch[t].m, ref) < 1e-13 and np.array_equal(one.m, batch[t].m) and np.array_equal(one.W, Wm)
    finally:
        meta.engine.close()
    # UniSGP, D = 1: three nodes with Gaussian inputs through rule_v + prod, then :out
    Xu1 = np.linspace(-2, 2, 7)[:, None]
    th1 = np.array([0.8, 1.2])
    um = UniSGPMeta(ExactSE(), Xu1, None, None, None, None, SEARDKernel(), None, N=3, jitter=1e-8)
    xs = [NormalMeanVariance(float(m), float(v)) for m, v in zip(rng.normal(size=3), (0.2, 0.05, 0.4))]
    ys = rng.normal(size=3)
    prior = MvNormalMeanCovariance(np.zeros(7), 5.0 * np.eye(7))
    try:
        acc = prior
        for x, yv in zip(xs, ys):
            acc = U.prod(acc, U.rule_v(PointMass(float(yv)), x, PointMass(4.0), PointMass(th1), um))
        mean1 = np.array([[q.m] for q in xs])
        cov1 = np.array([[[q.v]] for q in xs])
        psi1, psi2 = R.psi_stats(Xu1, th1[0], th1[1:], mean1, cov1)
        Lam = np.eye(7) / 5.0 + 4.0 * (psi2 + 3 * 1e-8 * np.eye(7))                 # every message carries Psi2 + 1e-8 I (:135)
        Sig_ref = np.linalg.inv(Lam)
        mu_ref = Sig_ref @ (4.0 * psi1.T @ ys)
        tol = post_tol(np.linalg.cond(Lam))
        assert relF(acc.m, mu_ref) < tol and relF(acc.S, Sig_ref) < tol
        q_v1 = MvNormalMeanCovariance(mu_ref, Sig_ref)
        outs = U.rule_out_batch(xs, q_v1, PointMass(4.0), PointMass(th1), um)
        for t in range(3):
            assert abs(outs[t].mean() - psi1[t] @ mu_ref) <= 1e-13 * np.abs(psi1[t]) @ np.abs(mu_ref)
            assert U.rule_out(xs[t], q_v1, PointMass(4.0), PointMass(th1), um).mean() == outs[t].mean()
        with pytest.raises(NotImplementedError):
            U.rule_w(PointMass(float(ys[0])), xs[0], q_v1, PointMass(th1), um)
    finally:
        um.engine.close()


@pytest.mark.parametrize("iterations", [1, 3])
def test_vmp_gpssm_exact_matches_its_restated_schedule(G, iterations):
    """T = 12, M = 10, d = 2: mean and cov of every q(x_t), mean(q(v)), mean(q(W)) (max |device - reference| / max |reference|) and
    the free energies against psi_stats_ref.vmp_gpssm_exact_ref.  Tolerance per quantity, as tests/test_gpu_gpssm.py derives it:
    10 x its relative change between two CPU runs of the restatement, as is and with every :out mean displaced by + its rounding
    bound -- which is 0 after one iteration (mu_v starts at 0: every :out mean is 0) and 6e-15 .. 1.7e-14 after three -- plus the
    bound the project holds a sweep's q(v) to, 20 eps cond(Lambda) = 3.2e-13 at cond(Lambda) = 72, because the device's sweep and
    :in steps differ from NumPy's too and the later iterations' q(x), q(W) are smooth functions of that q(v).  Free energy: 1e-8
    relative, the bound of tests/test_gpu_gpssm.py."""
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    from tests import gpssm_ref as GR
    p = R.GPSSM
    y, Xu, plain, moved = R.gpssm_reference(iterations)
    ref, alt = GR.compared(plain), GR.compared(moved)
    sweep_tol = 20 * np.finfo(float).eps * np.linalg.cond(np.linalg.inv(plain["q_v"].S))
    tol = {k: 10.0 * float(np.max(np.abs(ref[k] - alt[k])) / np.max(np.abs(ref[k]))) + sweep_tol for k in ref}
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(), jitter=p["jitter"])
    try:
        q_x, q_v, q_w, fe = train.vmp_gpssm(np.concatenate([[p["sigma2"]], p["ell"]]), y, meta, P=GR.P_OBS, x0_prior=GR.X0_PRIOR,
                                            iterations=iterations, free_energy=True, psi="exact", **GR.TEST_PRIORS)
    finally:
        meta.engine.close()
    assert type(meta.method).__name__ == "SphericalRadialCubature"
    got = GR.compared(dict(q_x=q_x, q_v=q_v, q_w=q_w))
    err = {k: float(np.max(np.abs(got[k] - ref[k])) / np.max(np.abs(ref[k]))) for k in ref}
    fe_err = float(np.max(np.abs(np.array(fe) - np.array(plain["fe"])) / np.abs(plain["fe"])))
    print(f"vmp_gpssm exact, {iterations} iterations: " + " ".join(f"{k} {err[k]:.3g} (tol {tol[k]:.3g})" for k in ref)
          + f"; free energy rel {fe_err:.3g}")
    assert len(q_x) == p["T"] + 1 and len(fe) == iterations
    assert fe_err <= 1e-8
    for k in ref:
        assert err[k] <= tol[k], (k, err[k], tol[k])


def gpssm_problem():
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    rng = np.random.default_rng(12)
    T, M, d = 12, 10, 2
    Xu = rng.uniform(-2.0, 2.0, (M, d))
    y = np.cumsum(0.3 * rng.normal(size=(T, d)), axis=0)
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-8)
    kw = dict(P=0.1 * np.eye(d), x0_prior=(np.zeros(d), 0.5 * np.eye(d)))
    return np.log(np.expm1(np.ones(3))), y, meta, kw


def flat(res):
    q_x, q_v, q_w, fe = res
    return [np.concatenate([np.ravel(q.m) for q in q_x] + [np.ravel(q.S) for q in q_x]), np.ravel(q_v.m), np.ravel(q_v.S),
            np.ravel(q_w.invS), np.asarray(fe)]


def test_psi_cubature_is_bitwise_the_default_and_exact_differs(G):
    from gaussianprocessnode_amd.train import vmp_gpssm
    runs = {}
    for name, extra in (("default", {}), ("cubature", {"psi": "cubature"}), ("exact", {"psi": "exact"})):
        theta, y, meta, kw = gpssm_problem()
        try:
            runs[name] = flat(vmp_gpssm(theta, y, meta, iterations=3, free_energy=True, **kw, **extra))
        finally:
            if meta.engine is not None:
                meta.engine.close()
    for a, b in zip(runs["default"], runs["cubature"]):
        assert np.array_equal(a, b)
    assert all(np.all(np.isfinite(a)) for a in runs["exact"])
    assert not np.array_equal(runs["exact"][1], runs["default"][1])
    with pytest.raises(ValueError):
        theta, y, meta, kw = gpssm_problem()
        vmp_gpssm(theta, y, meta, iterations=1, psi="other", **kw)


def test_exact_method_with_a_non_se_kernel_raises(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import ExactSE
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    Xu = np.random.default_rng(0).normal(size=(6, 2))
    kern = SEARDKernel(softplus_params=True)
    kern.family = "matern32"
    meta = MultiSGPMeta(ExactSE(), Xu, None, None, None, None, kern, jitter=1e-8)
    q_in = MvNormalMeanCovariance(np.zeros(2), 0.1 * np.eye(2))
    q_v = MvNormalMeanCovariance(np.zeros(12), np.eye(12))
    with pytest.raises(ValueError):
        MS.rule_out(q_in, q_v, PointMass(np.eye(2)), PointMass(np.zeros(3)), meta)
