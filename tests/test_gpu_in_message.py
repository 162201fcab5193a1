"""sgp_in_message on the device: closure values and moment-matched marginals of many nodes in one call, against the NumPy
restatement of tests/in_message_ref.py at its bounds (per point tol_p = 50 eps [1/2 tr(W) cond(K_uu) sigma2 + 1/2 cond(S) k'Sk +
|k|'|s_t|]; per node 2 tau, 4 tau r, 8 tau r^2 plus 1e-13 relative), then chunking, the posterior rules, the guarantee that the
call leaves the sweep's state alone, repeatability, every status, and the node mirrors' batch functions.

Every comparison prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import in_message_ref as R

pytestmark = pytest.mark.gpu

FULL, TARGETS, REUSED = 0, 1, 2
ERR_ARG = -1


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_for(G, c, n_max=64, **kw):
    dev = G.SGPDevice(n_max, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    return dev


def check_against_reference(name, c, lp, log_norm, mean, cov):
    T = c["nodes"]
    b0, b1, b2 = c["bounds"]
    def worst(err, bound):                                              # (a one-point node has r = 0: its bound and its error are both 0)
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
    ratios = dict(logpdf=worst(np.abs(lp - c["lp"]), c["tol"]),
                  log_norm=worst(np.abs(log_norm - c["log_norm"]), b0),
                  mean=worst(np.abs(mean - c["mean"]).reshape(T, -1).max(axis=1), b1),
                  cov=worst(np.abs(cov - c["cov"]).reshape(T, -1).max(axis=1), b2))
    print(f"case {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(np.isfinite(x).all() for x in (lp, log_norm, mean, cov))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cases_match_the_reference(G, name):
    c = R.reference(name)
    with device_for(G, c) as dev:
        out = dev.in_message(c["X"], c["start"], c["Y"], c["wts"], c["mu_v"], c["Sigma_v"])
        again = dev.in_message(c["X"], c["start"], c["Y"], c["wts"], c["mu_v"], c["Sigma_v"])
        lp_only = dev.in_message(c["X"], c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])
    check_against_reference(name, c, *out)
    for a, b in zip(out, again):                                       # repeated calls agree bitwise
        assert np.array_equal(a, b)
    assert np.array_equal(lp_only, out[0])


def test_case_e_falls_back_to_the_left_message_like_the_reference(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    from gaussianprocessnode_amd.unisgp import reference_moments_are_nan
    c = R.reference("e")
    st = c["start"]
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    lefts = [MvNormalMeanCovariance(c["means"][t], c["covs"][t]) for t in range(c["nodes"])]
    q_outs = [PointMass(y) for y in c["Y"]]
    args = (q_outs, lefts, MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(c["W"]),
            PointMass(np.concatenate([[c["sigma2"]], c["ell"]])), meta)
    try:
        out = MS.marginal_in_batch(*args)
        shifted = MS.marginal_in_batch(*args, reference_fallback=False)
    finally:
        meta.engine.close()
    nan_ref = [reference_moments_are_nan(c["lp"][st[t]:st[t + 1]]) for t in range(c["nodes"])]
    assert any(nan_ref)
    b0, b1, b2 = c["bounds"]
    for t in range(c["nodes"]):
        if nan_ref[t]:
            assert out[t] is lefts[t]
        else:
            assert np.max(np.abs(out[t].m - c["mean"][t])) <= b1[t]
        assert np.max(np.abs(shifted[t].m - c["mean"][t])) <= b1[t] and np.max(np.abs(shifted[t].S - c["cov"][t])) <= b2[t]


def test_chunked_call_is_bitwise_the_unchunked_one(G, monkeypatch):
    c = R.reference("a")
    rng = np.random.default_rng(20)
    sizes = [1, 64, 65, 20]                                              # nodes that fill, straddle and share 64-point chunks
    start = np.concatenate([[0], np.cumsum(sizes)])
    X = rng.uniform(-1.8, 1.8, (150, c["D"]))
    w = rng.uniform(0.1, 1.0, 150)
    Y = rng.normal(size=(4, c["d_out"]))
    out = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)                # 150 points = 2 full chunks and 22
        with device_for(G, c) as dev:
            out[chunk] = dev.in_message(X, start, Y, w, c["mu_v"], c["Sigma_v"])
    for a, b in zip(out[None], out["64"]):
        assert np.array_equal(a, b)
    # and the values are the closure's: against the restatement, at its bound
    cc = dict(R.make_case("a"), X=X, wts=w, start=start, Y=Y, nodes=4)
    lp_ref, tol, _ = R.logpdf_and_bound(cc)
    mom = R.node_moments(X, w, start, lp_ref)
    cc.update(lp=lp_ref, tol=tol, log_norm=mom[0], mean=mom[1], cov=mom[2], bounds=R.moment_bounds(X, start, tol, *mom))
    check_against_reference("a/chunked", cc, *out["64"])


def swept_multi(G, c, seed, **kw):
    """A handle of case c's model with data on it and one sweep done."""
    rng = np.random.default_rng(seed)
    N = 300
    X = rng.uniform(-1.8, 1.8, (N, c["D"]))
    y = np.stack([np.sin(X.sum(axis=1) + o) for o in range(c["d_out"])], axis=1) + 0.1 * rng.normal(size=(N, c["d_out"]))
    dev = device_for(G, c, n_max=N, **kw)
    dev.set_data(X, y[:, 0] if c["d_out"] == 1 else y)
    dev.set_prior_isotropic(50.0)
    dev.sweep()
    return dev, X, y


def test_null_posterior_is_the_last_sweeps(G):
    c = R.reference("a")
    dev, _, _ = swept_multi(G, c, seed=21)
    with dev:
        mu, Sig, Uv = dev.posterior()
        a = dev.in_message(c["X"], c["start"], c["Y"], c["wts"])
        b = dev.in_message(c["X"], c["start"], c["Y"], c["wts"], mu, Sig)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        dev.set_posterior(mu, Uv)
        with pytest.raises(G.SGPError):                                   # set_posterior gives no Sigma_v
            dev.in_message(c["X"], c["start"], c["Y"], c["wts"])
        dev.in_message(c["X"], c["start"], c["Y"], c["wts"], mu, Sig)     # (the explicit one is fine)
        dev.sweep()
        dev.in_message(c["X"], c["start"], c["Y"], c["wts"])


def _snapshot(dev):
    mu, Sig, Uv = dev.posterior()
    Psi2, B, sc = dev.stats()
    return dict(mu=mu, Sigma=Sig, Uv=Uv, Psi2=Psi2, B=B, sc=sc, KuuL=dev.kuu_chol(), wishart=dev.wishart_invscale(),
                scalars=np.array([getattr(dev.scalars(), f) for f in ("sum_I1", "sum_I2", "energy", "logdet_kuu", "logdet_lambda")]))


def test_reused_sweep_is_untouched_by_the_call(G):
    c = R.reference("a")
    snaps = []
    for with_call in (False, True):
        dev, _, _ = swept_multi(G, c, seed=22, reuse_stats=True)
        with dev:
            dev.set_noise(2.0 * c["W"])
            before = dev.sweep_kind()
            assert before[0] == REUSED
            if with_call:
                dev.in_message(c["X"], c["start"], c["Y"], c["wts"])
                dev.in_message(c["X"], c["start"], c["Y"], c["wts"], c["mu_v"], c["Sigma_v"])
                assert dev.sweep_kind() == before
            dev.sweep()
            assert dev.sweep_kind()[1] == REUSED
            snaps.append(_snapshot(dev))
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k


def raw(dev, X, start, Y, w, mu, Sig, outs=(True, True, True, True), n=None, n_nodes=None):
    """The C entry point itself: its status, no exception."""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    X = as_f64(X)
    start = np.ascontiguousarray(start, dtype=np.int64)
    n = len(X) if n is None else n
    n_nodes = len(start) - 1 if n_nodes is None else n_nodes
    D = dev.D
    bufs = [np.empty(max(n, 1)), np.empty(max(n_nodes, 1)), np.empty(max(n_nodes, 1) * D), np.empty(max(n_nodes, 1) * D * D)]
    y_cm = as_f64(np.asarray(Y, dtype=np.float64).reshape(-1, dev.d_out).T)
    S = None if Sig is None else as_f64(np.asarray(Sig).T)
    return dev._lib.sgp_in_message(dev._h, ptr(X), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes, ptr(y_cm),
                                   None if w is None else ptr(as_f64(w)), None if mu is None else ptr(as_f64(mu)), ptr(S),
                                   *[ptr(b) if keep else None for b, keep in zip(bufs, outs)])


def test_statuses(G):
    c = R.reference("a")
    X, st, Y, w, mu, Sig = c["X"], c["start"], c["Y"], c["wts"], c["mu_v"], c["Sigma_v"]
    with device_for(G, c) as dev:
        assert raw(dev, X, st, Y, w, mu, Sig) == 0
        for bad in ([1] + list(st[1:]), list(st[:-1]) + [st[-1] - 1], list(st[:-1]) + [st[-1] + 1], [0, 10, 5, 15, 20, 25, 30, 35],
                    [0, 5, 5, 15, 20, 25, 30, 35]):                        # not from 0, not to n (both ways), decreasing, an empty node
            assert raw(dev, X, bad, Y, w, mu, Sig) == ERR_ARG, bad
        for v in (-1e-3, np.nan, np.inf):
            wb = np.array(w)
            wb[7] = v
            assert raw(dev, X, st, Y, wb, mu, Sig) == ERR_ARG, v
        wb = np.array(w)
        wb[st[2]:st[3]] = 0.0                                             # a node whose weights sum to 0: no moments
        assert raw(dev, X, st, Y, wb, mu, Sig) == ERR_ARG
        wb[st[2]] = 0.25                                                  # (one positive weight beside zeros is fine)
        assert raw(dev, X, st, Y, wb, mu, Sig) == 0
        for missing in range(1, 4):                                       # weights without one of log_norm, mean, cov
            outs = [True] * 4
            outs[missing] = False
            assert raw(dev, X, st, Y, w, mu, Sig, outs=outs) == ERR_ARG
        assert raw(dev, X, st, Y, None, mu, Sig, outs=(True, False, False, False)) == 0
        assert raw(dev, X, st, Y, w, mu, None) == ERR_ARG and raw(dev, X, st, Y, w, None, Sig) == ERR_ARG
        assert raw(dev, X, st, Y, w, None, None) == ERR_ARG               # no sweep yet: no posterior in the handle
        assert raw(dev, X[:0], [0], Y[:0], w[:0], mu, Sig, n=0, n_nodes=0) == 0          # n = 0: nothing to do
        assert dev._lib.sgp_in_message(dev._h, None, 0, None, 0, None, None, None, None, None, None, None, None) == 0
        bad = np.array(Sig)
        bad[5, :] = bad[:, 5] = 0.0
        bad[5, 5] = -100.0
        with pytest.raises(G.PosDefException) as e:                       # S inherits the negative direction: its leading minor
            dev.in_message(X, st, Y, w, mu, bad)
        assert e.value.info == 6
        assert raw(dev, X, st, Y, w, mu, Sig) == 0                        # (and the handle goes on working)
    u = R.reference("c")
    with device_for(G, u, n_max=200) as dev:                              # an open device-paced training run (UniSGP only)
        rng = np.random.default_rng(23)
        Xt = rng.uniform(-1.8, 1.8, (200, 1))
        dev.set_prior_isotropic(50.0)
        dev.train_begin(Xt, np.sin(Xt[:, 0]), np.array([0.5, 1.0]), jitter=1e-6)
        assert raw(dev, u["X"], u["start"], u["Y"], u["wts"], u["mu_v"], u["Sigma_v"]) == ERR_ARG
        dev.train_end()
        dev.set_kernel(u["sigma2"], u["ell"], u["jitter"])
        assert raw(dev, u["X"], u["start"], u["Y"], u["wts"], u["mu_v"], u["Sigma_v"]) == 0


def test_marginal_in_batch_matches_the_rule_in_closures(G):
    """The node mirror over case (a)'s 7 nodes: one device call, against the host moments of the existing per-node closures
    (each its own device pass through sgp_w_stats), and prod_logpdf against its entry of the batch."""
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    from gaussianprocessnode_amd.unisgp import shifted_moments
    c = R.reference("a")
    st = c["start"]
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    lefts = [MvNormalMeanCovariance(c["means"][t], c["covs"][t]) for t in range(c["nodes"])]
    q_outs = [PointMass(y) for y in c["Y"]]
    q_v, q_w = MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(c["W"])
    theta = PointMass(np.concatenate([[c["sigma2"]], c["ell"]]))
    b0, b1, b2 = c["bounds"]
    try:
        batch = MS.marginal_in_batch(q_outs, lefts, q_v, q_w, theta, meta)
        worst = 0.0
        for t in range(c["nodes"]):
            closure = MS.rule_in(q_outs[t], q_v, q_w, theta, meta)
            pts, wts = srcubature().points_weights(lefts[t].m, lefts[t].S)
            lp = np.asarray(closure.logpdf(pts))
            assert np.all(np.abs(lp - c["lp"][st[t]:st[t + 1]]) <= c["tol"][st[t]:st[t + 1]])
            _, m, S = shifted_moments(pts, wts, lp)
            worst = max(worst, np.max(np.abs(batch[t].m - m)) / b1[t], np.max(np.abs(batch[t].S - S)) / b2[t])
            one = MS.prod_logpdf(lefts[t], closure)
            assert np.array_equal(one.m, batch[t].m) and np.array_equal(one.S, batch[t].S)
        print(f"marginal_in_batch vs rule_in closures: error / bound {worst:.3g}")
        assert worst <= 1.0
    finally:
        meta.engine.close()
        if getattr(meta, "_aux_engine", None) is not None:
            meta._aux_engine.close()


def test_predict_var_and_in_message_share_the_call_scratch_cleanly(G, monkeypatch):
    """predict_var, in_message, predict_var on ONE handle: the two calls lay the same call scratch out differently, every piece
    rounded up to 64 doubles, so at sizes that are no multiple of 64 (M = 40: Mp != M, Q = 80: Qp != Q, 150 points, 7 uneven
    nodes) an overlap of two pieces or stale data of the other call's layout would show.  Bitwise: predict_var before and after
    the in_message call, and in_message against a fresh handle."""
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")                         # 150 points = 2 full chunks and 22
    M, D, d_out, n = 40, 3, 2, 150
    rng = np.random.default_rng(24)
    c = dict(M=M, D=D, d_out=d_out, Xu=rng.uniform(-1.8, 1.8, (M, D)), sigma2=0.9, ell=np.array([1.1, 0.8, 1.3]), jitter=1e-6,
             family="se", W=np.array([[2.0, 0.3], [0.3, 1.5]]))
    sizes = [1, 40, 23, 2, 64, 7, 13]
    assert sum(sizes) == n
    start = np.concatenate([[0], np.cumsum(sizes)])
    X = rng.uniform(-1.8, 1.8, (n, D))
    w = rng.uniform(0.1, 1.0, n)
    Y = rng.normal(size=(len(sizes), d_out))
    mu = rng.normal(size=M * d_out)
    A = rng.normal(size=(M * d_out, M * d_out))
    Sig = A @ A.T / (M * d_out) + 0.1 * np.eye(M * d_out)
    with device_for(G, c) as dev:
        first = dev.predict_var(X, mu, Sig, noise=True)
        msg = dev.in_message(X, start, Y, w, mu, Sig)
        second = dev.predict_var(X, mu, Sig, noise=True)
    with device_for(G, c) as dev:
        fresh = dev.in_message(X, start, Y, w, mu, Sig)
    assert all(np.isfinite(a).all() for a in first + msg)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    for a, b in zip(msg, fresh):
        assert np.array_equal(a, b)
