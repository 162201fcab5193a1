"""sgp_predict_joint and sgp_sample_f on the device against the float64 reference of tests/predict_joint_ref.py at its bounds
(tests/test_predict_joint_host.py holds those against mpmath and shows that they see the faults of predict_joint_ref.FAULTS).

    tile{ns}x{M}x{d_out}   ns, M in {1, 63, 64, 65, 129}, d_out 1 and 3: one ragged point block, a full one, one point into the second,
                           one into the third, against one ragged tile of Z / U, a full one, a second and a third -- with d_out = 3
                           the block rows of L_S start off the tile grid
    {family}x{d_out}       every family's k_joint_cov with every output count at (ns, M, D) = (70, 65, 9)
    dim{1,5,32}[iso]       the coordinate staging of k_joint_cov at D = 1, 5 and MAXD, ARD and isotropic, (ns, M) = (130, 70)
    limit                  d_out M = 4032 at ns = 70: 63 tile columns of every panel
    dup                    two identical test points: a singular cov; sampling succeeds with sample_jitter = 1e-6 sigma2
    ill_*                  jitter 1e-8
    chunk130, chunk257     bitwise equality under SGP_PREDICT_CHUNK = 64 against the default (the variable is read per handle)

Every comparison prints its worst error / bound ratio before it asserts.  Every entry of the R x R matrix is compared."""
import ctypes as C

import numpy as np
import pytest

from tests import predict_joint_ref as J

pytestmark = pytest.mark.gpu
EPS = J.EPS


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


def joint(dev, c):
    """(mean, cov, cov with noise) at the case's explicit q(v); the mean is bitwise sgp_predict's, both matrices exactly symmetric."""
    q = (c["mu_v"], c["Sigma_v"])
    pm = dev.predict(c["X"], c["mu_v"])
    m, cov = dev.predict_joint(c["X"], *q)
    mn, covn = dev.predict_joint(c["X"], *q, noise=True)
    assert np.array_equal(pm, m) and np.array_equal(m, mn)
    assert np.array_equal(cov, cov.T) and np.array_equal(covn, covn.T)
    return m, cov, covn


def check(name, c, out, dev=None):
    m, cov, covn = out
    R = len(c["X"]) * c["d_out"]
    assert cov.shape == covn.shape == (R, R) and np.isfinite(cov).all() and np.isfinite(covn).all()
    r = dict(cov=J.cov_ratio(c, cov), noise=J.noise_ratio(c, covn, cov))
    if dev is not None:                                      # the diagonal blocks against sgp_predict_var: the sum of the two bounds
        _, var = dev.predict_var(c["X"], c["mu_v"], c["Sigma_v"])
        ns, d = len(c["X"]), c["d_out"]
        r["predict_var"] = J.worst(np.abs(J.diag_blocks(cov, ns, d) - var.reshape(ns, d, d)), 2 * J.diag_block_bounds(c))
    print(f"case {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, (name, k, v)


def run_case(G, name):
    c = J.reference(name)
    with device_for(G, c) as dev:
        out = joint(dev, c)
        check(name, c, out, dev)
    return c, out


@pytest.mark.parametrize("name", J.group("tile"))
def test_tile_edges_of_points_and_inducing_inputs(G, name):
    run_case(G, name)


@pytest.mark.parametrize("name", J.group("family"))
def test_families_and_output_counts(G, name):
    run_case(G, name)


@pytest.mark.parametrize("name", J.group("dims"))
def test_input_dimensions(G, name):
    run_case(G, name)


def test_the_size_limit(G):
    run_case(G, "limit")


@pytest.mark.parametrize("name", J.group("ill"))
def test_ill_conditioned_kuu(G, name):
    run_case(G, name)


def test_two_identical_points(G):
    c, (m, cov, covn) = run_case(G, "dup")
    a, b = J.DUP_PAIR
    assert np.array_equal(m[a], m[b])


@pytest.mark.parametrize("name", J.group("chunk"))
def test_repeats_and_chunks_agree_bitwise(G, monkeypatch, name):
    c = J.reference(name)
    eps = J.general_eps(c)
    out = []
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        with device_for(G, c) as dev:
            for _ in range(2):
                m, cov, covn = joint(dev, c)
                _, smp = dev.sample_f(c["X"], eps, J.sample_jitter(c), c["mu_v"], c["Sigma_v"])
                out.append((m, cov, covn, smp))
            if chunk is None:
                check(name, c, out[0][:3], dev)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes(), name


def test_the_handle_s_own_posterior(G):
    """mu_v = Sigma_v = NULL after a sweep: k_pad_square's copy of the last sweep's Sigma_v (Q = 189, Q_p = 192) against the same
    call with that q(v) passed explicitly, and against the reference evaluated at it."""
    c = dict(J.reference("tile65x63x3"))
    rng = np.random.default_rng(77)
    N = 200
    X = rng.uniform(-1.5, 1.5, (N, c["D"]))
    Y = rng.normal(size=(N, c["d_out"]))
    with G.SGPDevice(N, c["M"], c["D"], c["d_out"]) as dev:
        dev.set_inducing(c["Xu"])
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
        dev.set_noise(c["W"])
        dev.set_data(X, Y)
        dev.set_prior_isotropic(2.0)
        dev.sweep()
        mu, Sig, _ = dev.posterior()
        own = dev.predict_joint(c["X"])
        given = dev.predict_joint(c["X"], mu, Sig)
        e = np.eye(len(own[1]))[:, :3]
        s_own = dev.sample_f(c["X"], e, 1e-9 * c["sigma2"])
        s_given = dev.sample_f(c["X"], e, 1e-9 * c["sigma2"], mu, Sig)
    for a, b in zip(own + s_own, given + s_given):
        assert a.tobytes() == b.tobytes()
    c.update(mu_v=mu, Sigma_v=Sig)
    ref = J.evaluate(c)
    cond_sigma = float(np.linalg.cond(Sig))
    b = J.bounds(c, ref, c["cond_kuu"], cond_sigma)
    ratio = J.worst(np.abs(own[1] - ref["C"]), b["b_cov"])
    print(f"own q(v): cond(Sigma_v) {cond_sigma:.3g}, error / bound {ratio:.3g}")
    assert ratio <= 1.0


# ---- samples --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.SAMPLE_CASES)
def test_the_factor_through_unit_normals(G, name):
    """eps = I with mu_v = 0 (the mean is then exactly 0, so that the samples ARE the columns of L_C): rows above the diagonal are
    the mean bitwise, and L_C meets the backward-error bound against the device's own cov."""
    c = J.reference(name)
    R = len(c["C"])
    assert R <= 260
    zero = np.zeros_like(c["mu_v"])
    s = J.sample_jitter(c)
    with device_for(G, c) as dev:
        _, cov = dev.predict_joint(c["X"], zero, c["Sigma_v"])
        mean, L = dev.sample_f(c["X"], np.eye(R), s, zero, c["Sigma_v"])
        mean2, Lm = dev.sample_f(c["X"], np.eye(R), s, c["mu_v"], c["Sigma_v"])
        pm = dev.predict(c["X"], c["mu_v"])
    assert not mean.any() and np.array_equal(mean2, pm)
    upper = np.triu_indices(R, 1)
    assert not L[upper].any()
    vec = np.reshape(mean2, (len(c["X"]), -1)).T.reshape(-1)
    assert np.array_equal(Lm[upper], np.broadcast_to(vec[:, None], (R, R))[upper])
    ratio = J.chol_ratio(L, cov + s * np.eye(R)) / J.CHOL_C
    print(f"case {name}: R {R}, |L L' - (cov + s I)| / (c R eps |L||L'|) = {ratio:.3g} (c = {J.CHOL_C})")
    assert np.isfinite(L).all() and ratio <= 1.0


@pytest.mark.parametrize("name", J.SAMPLE_CASES)
def test_general_normals(G, name):
    """samples - mean against L_dev eps within 50 eps |L_dev| |eps| -- taken at mu_v = 0, where the mean is exactly 0 and
    samples - mean IS what the device's product returned: at a non-zero mean the sum mean + L eps rounds once more (eps |sample| / 2,
    which the product's bound does not hold where a row of |L| |eps| is small against the mean: 2.8 x the bound at sex3), so the call
    with the case's own mu_v is held to something sharper instead -- bitwise mean + (the samples at mu_v = 0), one IEEE addition."""
    c = J.reference(name)
    R = len(c["C"])
    eps = J.general_eps(c)
    s = J.sample_jitter(c)
    zero = np.zeros_like(c["mu_v"])
    with device_for(G, c) as dev:
        _, L = dev.sample_f(c["X"], np.eye(R), s, zero, c["Sigma_v"])
        mean0, smp0 = dev.sample_f(c["X"], eps, s, zero, c["Sigma_v"])
        mean, smp = dev.sample_f(c["X"], eps, s, c["mu_v"], c["Sigma_v"])
        mean_b, smp_b = dev.sample_f(c["X"], eps, s, c["mu_v"], c["Sigma_v"])
        pm = dev.predict(c["X"], c["mu_v"])
    assert smp.shape == smp0.shape == (R, J.N_GENERAL) and np.array_equal(mean, pm) and not mean0.any()
    assert smp.tobytes() == smp_b.tobytes() and mean.tobytes() == mean_b.tobytes()
    ratio = J.worst(np.abs(smp0 - L @ eps), 50 * EPS * (np.abs(L) @ np.abs(eps)))
    print(f"case {name}: samples - mean against L_dev eps, error / bound {ratio:.3g}")
    assert ratio <= 1.0
    vec = np.reshape(mean, (len(c["X"]), -1)).T.reshape(-1)[:, None]
    assert np.array_equal(smp, vec + smp0)


# ---- state ----------------------------------------------------------------------------------------------------------------------
def _swept_state(dev):
    mu, Sig, Uv = dev.posterior()
    return [mu, Sig, Uv, np.array(dev.sweep_kind()), *dev.stats(), np.array([dev.theta_objective()]).ravel()]


def test_both_calls_change_nothing_of_the_handle(G):
    rng = np.random.default_rng(12)
    N, M, D = 400, 48, 3
    X, y = rng.uniform(-1.5, 1.5, (N, D)), rng.normal(size=N)
    Xu, ell = X[rng.permutation(N)[:M]], np.array([0.9, 1.1, 1.3])
    Xs = rng.uniform(-1.5, 1.5, (70, D))
    eps = rng.normal(size=(70, 3))
    calls = []

    def hook(buf, count, stream):                           # (one rank: the sum over ranks is the buffer as it is)
        calls.append(count)
        return 0

    def run(with_calls):
        with G.SGPDevice(N, M, D, reuse_stats=True) as dev:
            dev.set_inducing(Xu)
            dev.set_data(X, y)
            dev.set_kernel(0.8, ell, 1e-6, family="matern32")
            dev.set_prior_isotropic(50.0)
            dev.set_noise([[20.0]])
            dev.set_allreduce(hook)
            dev.sweep()
            before = _swept_state(dev)
            if with_calls:
                n_calls = len(calls)
                dev.predict_joint(Xs, noise=True)
                dev.sample_f(Xs, eps, 1e-9)
                assert len(calls) == n_calls                 # an installed hook is neither called nor a reason to refuse
                between = _swept_state(dev)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(before, between))
            dev.sweep()
            return before + _swept_state(dev)

    plain, called = run(False), run(True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, called))


# ---- the Python layers ------------------------------------------------------------------------------------------------------------
def _close(meta):
    for eng in (getattr(meta, "engine", None),):
        if eng is not None:
            eng.close()


def test_predictive_joint_and_sample_posterior_multi(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    c = J.reference("tile65x63x3")
    ns, d = len(c["X"]), c["d_out"]
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    q_v, q_w = MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(c["W"])
    q_theta = PointMass(np.concatenate([[c["sigma2"]], c["ell"]]))
    try:
        m, C = MS.predictive(c["X"], q_v, q_w, q_theta, meta, noise=False, joint=True)
        mn, Cn = MS.predictive(c["X"], q_v, q_w, q_theta, meta, joint=True)
        mean, smp = train.sample_posterior(meta, c["X"], 5, np.random.default_rng(3), q_v=q_v, q_theta=q_theta)
        mean_b, smp_b = train.sample_posterior(meta, c["X"], 5, np.random.default_rng(3), q_v=q_v, q_theta=q_theta)
        eps = np.random.default_rng(3).standard_normal((ns * d, 5))
        _, direct = meta.engine.sample_f(c["X"], eps, 1e-9 * c["sigma2"], c["mu_v"], c["Sigma_v"])
        with pytest.raises(ValueError):
            MS.predictive(MvNormalMeanCovariance(c["X"][0], np.eye(c["D"])), q_v, q_w, q_theta, meta, joint=True)
    finally:
        _close(meta)
    assert m.shape == mn.shape == (ns, d) and C.shape == Cn.shape == (ns * d, ns * d)
    assert J.cov_ratio(c, C) <= 1.0 and J.noise_ratio(c, Cn, C) <= 1.0
    assert smp.shape == (5, ns, d) and mean.shape == (ns, d) and np.array_equal(mean, m)
    assert smp.tobytes() == smp_b.tobytes()
    assert np.array_equal(smp, direct.T.reshape(5, d, ns).transpose(0, 2, 1))


def test_predictive_joint_and_sample_posterior_uni(G):
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd import unisgp as US
    from gaussianprocessnode_amd.distributions import GammaShapeRate, MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import SEARDKernel, UniSGPMeta
    c = J.reference("tile65x64x1")
    ns = len(c["X"])
    meta = UniSGPMeta(None, c["Xu"], None, None, None, None, SEARDKernel(), None, 0, 8, jitter=c["jitter"])
    q_v, q_theta = MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(np.concatenate([[c["sigma2"]], c["ell"]]))
    w = float(c["W"][0, 0])
    try:
        m, C = US.predictive(c["X"], q_v, GammaShapeRate(w, 1.0), q_theta, meta, noise=False, joint=True)
        mn, Cn = US.predictive(c["X"], q_v, GammaShapeRate(w, 1.0), q_theta, meta, joint=True)
        mean, smp = train.sample_posterior(meta, c["X"], 4, np.random.default_rng(8), q_v=q_v, q_theta=q_theta)
        with pytest.raises(ValueError):
            US.predictive(PointMass(c["X"][0]), q_v, GammaShapeRate(w, 1.0), q_theta, meta, joint=True)
    finally:
        _close(meta)
    assert m.shape == (ns,) and C.shape == Cn.shape == (ns, ns) and np.array_equal(m, mn)
    assert J.cov_ratio(c, C) <= 1.0 and J.noise_ratio(c, Cn, C) <= 1.0
    assert smp.shape == (4, ns, 1) and np.array_equal(mean[:, 0], m)
