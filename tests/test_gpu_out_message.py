"""sgp_out_message on the device: the :out message means of many nodes in one call, against the NumPy restatement of
tests/gpssm_ref.py at its bound tol[t, d] = 50 eps sum_s |w_s| |k_s|'|mu_v^(d)|; then the per-point values against sgp_predict,
repeatability and chunking (bitwise), the posterior rule, the guarantee that the call leaves the sweep's state alone, every status,
and the node mirrors' batch functions against the loop of the existing per-node rules.

Every comparison prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import gpssm_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG = -1
REUSED = 2


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_for(G, c, n_max=64, **kw):
    dev = G.SGPDevice(n_max, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell"], c["jitter"], family=c["family"])
    return dev


def worst(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


@pytest.mark.parametrize("name", sorted(R.OUT_CASES))
def test_cases_match_the_reference(G, name):
    c, mean_ref, tol, point_ref = R.out_reference(name)
    with device_for(G, c) as dev:
        mean, point = dev.out_message(c["X"], c["start"], c["wts"], c["mu_v"], want_points=True)
        again = dev.out_message(c["X"], c["start"], c["wts"], c["mu_v"], want_points=True)
        predicted = np.asarray(dev.predict(c["X"], c["mu_v"])).reshape(len(c["X"]), c["d_out"])
        ones = dev.out_message(c["X"], c["start"], np.ones(len(c["X"])), c["mu_v"])
        unweighted = dev.out_message(c["X"], c["start"], None, c["mu_v"])
    ratio = worst(np.abs(mean - mean_ref), tol)
    K = np.abs(R.kernel(c["family"], c["sigma2"], c["ell"], c["Xu"], c["X"]))             # M x n
    point_tol = 50 * R.EPS * K.T @ np.abs(c["mu_v"]).reshape(c["d_out"], c["M"]).T          # tol's summand: 50 eps |k_s|'|mu_v^(d)|
    point_ratio = worst(np.abs(point - point_ref), point_tol)
    print(f"case {name}: worst |mean - reference| / tol {ratio:.3g}, per point {point_ratio:.3g}")
    assert mean.shape == mean_ref.shape and np.isfinite(mean).all() and np.isfinite(point).all()
    assert ratio <= 1.0
    assert point.shape == point_ref.shape and point_ratio <= 1.0
    assert np.array_equal(point, predicted)                                # bitwise sgp_predict's values
    assert np.array_equal(mean, again[0]) and np.array_equal(point, again[1])        # repeated calls agree bitwise
    assert np.array_equal(ones, unweighted)


def test_chunked_calls_are_bitwise_the_unchunked_one(G, monkeypatch):
    c, mean_ref, tol, _ = R.out_reference("d")
    out = {}
    for chunk in (None, "64", "128"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)                 # 158 points: 2 chunks and 30, 1 chunk and 30
        with device_for(G, c) as dev:
            out[chunk] = dev.out_message(c["X"], c["start"], c["wts"], c["mu_v"], want_points=True)
    for chunk in ("64", "128"):
        assert np.array_equal(out[None][0], out[chunk][0]) and np.array_equal(out[None][1], out[chunk][1]), chunk
    assert worst(np.abs(out["64"][0] - mean_ref), tol) <= 1.0


def swept(G, c, seed, **kw):
    rng = np.random.default_rng(seed)
    N = 300
    X = rng.uniform(-1.8, 1.8, (N, c["D"]))
    y = np.stack([np.sin(X.sum(axis=1) + o) for o in range(c["d_out"])], axis=1) + 0.1 * rng.normal(size=(N, c["d_out"]))
    dev = device_for(G, c, n_max=N, **kw)
    dev.set_noise(2.0 * np.eye(c["d_out"]))
    dev.set_data(X, y[:, 0] if c["d_out"] == 1 else y)
    dev.set_prior_isotropic(50.0)
    dev.sweep()
    return dev


def test_null_mu_is_the_last_sweeps_and_the_sweep_state_is_untouched(G):
    c = R.make_out_case("a")
    results = []
    for with_call in (False, True):
        with swept(G, c, seed=41, reuse_stats=True) as dev:
            dev.set_noise(3.0 * np.eye(c["d_out"]))
            before = dev.sweep_kind()
            assert before[0] == REUSED
            if with_call:
                mu = dev.posterior(want_cov=False, want_uv=False)[0]
                a = dev.out_message(c["X"], c["start"], c["wts"], want_points=True)
                b = dev.out_message(c["X"], c["start"], c["wts"], mu, want_points=True)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert dev.sweep_kind() == before
            value, grad = dev.theta_objective(want_grad=True)
            results.append((value, np.asarray(grad)))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])


def raw(dev, X, start, w, mu, want_mean=True, n=None, n_nodes=None):
    """The C entry point itself: its status, no exception."""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    X = as_f64(X)
    start = np.ascontiguousarray(start, dtype=np.int64)
    n = len(X) if n is None else n
    n_nodes = len(start) - 1 if n_nodes is None else n_nodes
    mean = np.empty(max(n_nodes, 1) * dev.d_out)
    return dev._lib.sgp_out_message(dev._h, ptr(X), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes,
                                    None if w is None else ptr(as_f64(w)), None if mu is None else ptr(as_f64(mu)),
                                    ptr(mean) if want_mean else None, None)


def refused(dev, *args, **kw):
    rc = raw(dev, *args, **kw)
    msg = dev._lib.sgp_last_error(dev._h).decode()
    return rc == ERR_ARG and "sgp_out_message" in msg


def test_statuses(G):
    c = R.make_out_case("a")
    X, st, w, mu = c["X"], c["start"], c["wts"], c["mu_v"]
    with device_for(G, c) as dev:
        assert raw(dev, X, st, w, mu) == 0
        for bad in ([1] + list(st[1:]), list(st[:-1]) + [st[-1] + 1], [0, 5, 5] + list(st[3:])):     # not from 0, not to n, an empty node
            assert refused(dev, X, bad, w, mu), bad
        wb = np.array(w)
        wb[7] = np.nan
        assert refused(dev, X, st, wb, mu)
        wb[7] = -3.0                                                      # (any finite weight is fine)
        assert raw(dev, X, st, wb, mu) == 0
        assert refused(dev, X, st, w, mu, want_mean=False)
        assert refused(dev, X, st, w, None)                               # no sweep yet: no posterior in the handle
        assert raw(dev, X[:0], [0], w[:0], mu, n=0, n_nodes=0) == 0       # n = 0: nothing to do
        assert dev._lib.sgp_out_message(dev._h, None, 0, None, 0, None, None, None, None) == 0
    u = dict(R.make_out_case("b"), family="se")
    with device_for(G, u, n_max=200) as dev:                              # an open device-paced training run (UniSGP only)
        rng = np.random.default_rng(42)
        Xt = rng.uniform(-1.8, 1.8, (200, 1))
        dev.set_noise([[100.0]])
        dev.set_prior_isotropic(50.0)
        dev.train_begin(Xt, np.sin(Xt[:, 0]), np.array([0.5, 1.0]), jitter=1e-6)
        assert refused(dev, u["X"], u["start"], u["wts"], u["mu_v"])
        dev.train_end()
        dev.set_kernel(u["sigma2"], u["ell"], u["jitter"], family=u["family"])
        assert raw(dev, u["X"], u["start"], u["wts"], u["mu_v"]) == 0


def test_rule_out_batch_is_the_loop_of_rule_out(G):
    """multisgp (case a's model, Gaussian and PointMass inputs mixed) and unisgp (case b's model): one device call against the
    loop of the existing per-node rule, at the sum of the two calls' bounds (rule_out sums on the host: not bitwise)."""
    from gaussianprocessnode_amd import multisgp as MS, unisgp as US
    from gaussianprocessnode_amd.cubature import ghcubature, srcubature
    from gaussianprocessnode_amd.distributions import (MvNormalMeanCovariance, NormalMeanVariance, PointMass)
    from gaussianprocessnode_amd.meta import MaternARDKernel, MultiSGPMeta, SEARDKernel, make_uni_meta
    rng = np.random.default_rng(43)
    c = R.make_out_case("a")
    M, d = c["M"], c["d_out"]
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    q_ins = []
    for t in range(9):
        L = rng.normal(size=(2, 2))
        q_ins.append(PointMass(rng.uniform(-1.5, 1.5, 2)) if t % 4 == 3 else
                     MvNormalMeanCovariance(rng.uniform(-1.5, 1.5, 2), 0.05 * (L @ L.T / 2 + np.eye(2))))
    q_v = MvNormalMeanCovariance(c["mu_v"], np.eye(M * d))
    q_w, theta = PointMass(np.array([[2.0, 0.3], [0.3, 1.5]])), PointMass(np.concatenate([[c["sigma2"]], c["ell"]]))
    mus = np.abs(c["mu_v"]).reshape(d, M)
    try:
        batch = MS.rule_out_batch(q_ins, q_v, q_w, theta, meta)
        ratio = 0.0
        for t, q in enumerate(q_ins):
            one = MS.rule_out(q, q_v, q_w, theta, meta)
            p, w = (np.atleast_2d(q.mean()), np.ones(1)) if isinstance(q, PointMass) else srcubature().points_weights(*q.mean_cov())
            K = np.abs(R.kernel("se", c["sigma2"], c["ell"], c["Xu"], p))
            bound = 2 * 50 * R.EPS * (mus @ (K @ np.abs(w)))
            ratio = max(ratio, worst(np.abs(batch[t].m - one.m), bound))
            assert np.array_equal(batch[t].W, one.W)
        print(f"multisgp.rule_out_batch vs rule_out loop: error / bound {ratio:.3g}")
        assert len(batch) == len(q_ins) and ratio <= 1.0
    finally:
        meta.engine.close()
    u = R.make_out_case("b")
    umeta = make_uni_meta(ghcubature(21), u["Xu"], MaternARDKernel(2.5), 4, jitter=u["jitter"])
    u_ins = [NormalMeanVariance(0.4, 0.05), PointMass(-0.7), NormalMeanVariance(-1.1, 0.02), NormalMeanVariance(1.3, 0.08)]
    u_v = MvNormalMeanCovariance(u["mu_v"], np.eye(u["M"]))
    u_w, u_theta = PointMass(7.0), PointMass(np.concatenate([[u["sigma2"]], u["ell"]]))
    try:
        batch = US.rule_out_batch(u_ins, u_v, u_w, u_theta, umeta)
        ratio = 0.0
        for t, q in enumerate(u_ins):
            one = US.rule_out(q, u_v, u_w, u_theta, umeta)
            p, w = (np.array([[q.mean()]]), np.ones(1)) if isinstance(q, PointMass) else ghcubature(21).points_weights(q.mean(), q.var())
            K = np.abs(R.kernel("matern52", u["sigma2"], u["ell"], u["Xu"], p))
            bound = 2 * 50 * R.EPS * float(np.abs(u["mu_v"]) @ (K @ np.abs(w)))
            ratio = max(ratio, worst(abs(batch[t].mean() - one.mean()), bound))
            assert batch[t].precision() == one.precision()
        print(f"unisgp.rule_out_batch vs rule_out loop: error / bound {ratio:.3g}")
        assert ratio <= 1.0
    finally:
        umeta.engine.close()
