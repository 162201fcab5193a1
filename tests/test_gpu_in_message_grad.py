"""sgp_in_message_grad on the device: the :in log-messages of many nodes with their analytic gradients and Hessians, against the
NumPy restatement of tests/in_message_grad_ref.py at its bounds (C_BOUND was settled on the CPU, never against the device), then
the shapes at which the kernels change path, chunking, the posterior rules, the sweep's state, every status, and
multisgp.rule_in_laplace_batch.

Every comparison prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import in_message_grad_ref as GR
from tests import in_message_ref as R
from tests.test_gpu_in_message import ERR_ARG, REUSED, _snapshot, device_for, swept_multi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_of(G, c, **kw):
    return device_for(G, dict(c, ell=c.get("ell_dev", c["ell"])), **kw)


def check(name, c, lp, grad, hess):
    r = GR.ratios(c, lp, grad, hess)
    print(f"case {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(np.isfinite(x).all() for x in (lp, grad, hess))
    for k, v in r.items():
        assert v <= 1.0, (k, v)
    assert np.array_equal(hess, hess.transpose(0, 2, 1))


@pytest.mark.parametrize("name", GR.REFERENCE_CASES)
def test_cases_match_the_reference(G, name):
    c = GR.reference(name)
    args = (c["X"], c["start"], c["Y"], c["mu_v"], c["Sigma_v"])
    with device_of(G, c) as dev:
        out = dev.in_message_grad(*args)
        again = dev.in_message_grad(*args)
        message = dev.in_message(c["X"], c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])
        no_hess = dev.in_message_grad(*args, hessian=False)
    check(name, c, *out)
    for a, b in zip(out, again):                                          # repeated calls agree bitwise
        assert np.array_equal(a, b)
    assert np.array_equal(out[0], message)                                # logpdf is sgp_in_message's, bitwise
    assert no_hess[2] is None and np.array_equal(no_hess[0], out[0]) and np.array_equal(no_hess[1], out[1])


@pytest.mark.parametrize("name", sorted(GR.GRAD_SHAPES))
def test_shapes_match_the_reference(G, name):
    c = GR.reference(name)
    with device_of(G, c) as dev:
        out = dev.in_message_grad(c["X"], c["start"], c["Y"], c["mu_v"], c["Sigma_v"])
        message = dev.in_message(c["X"], c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])
    check(name, c, *out)
    assert np.array_equal(out[0], message)


def test_chunked_call_is_bitwise_the_unchunked_one(G, monkeypatch):
    c = R.reference("a")
    rng = np.random.default_rng(30)
    sizes = [1, 64, 65, 20]                                              # nodes that fill, straddle and share 64-point chunks
    start = np.concatenate([[0], np.cumsum(sizes)])
    X = rng.uniform(-1.8, 1.8, (150, c["D"]))
    Y = rng.normal(size=(4, c["d_out"]))
    out = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)                # 150 points = 2 full chunks and 22
        with device_for(G, c) as dev:
            out[chunk] = dev.in_message_grad(X, start, Y, c["mu_v"], c["Sigma_v"])
    for a, b in zip(out[None], out["64"]):
        assert np.array_equal(a, b)
    cc = dict(R.make_case("a"), X=X, start=start, Y=Y, nodes=4)
    lp, grad, hess = GR.evaluate(cc, "cholesky")
    tg, th = GR.bounds(cc)
    cc.update(lp=lp, tol=R.vector_logpdf(cc, want_bound=True)["tol"], grad=grad, hess=hess, tol_grad=tg, tol_hess=th)
    check("a/chunked", cc, *out["64"])


def test_null_posterior_is_the_last_sweeps(G):
    c = R.reference("a")
    dev, _, _ = swept_multi(G, c, seed=31)
    args = (c["X"], c["start"], c["Y"])
    with dev:
        mu, Sig, Uv = dev.posterior()
        a = dev.in_message_grad(*args)
        b = dev.in_message_grad(*args, mu, Sig)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        dev.set_posterior(mu, Uv)
        with pytest.raises(G.SGPError):                                   # set_posterior gives no Sigma_v
            dev.in_message_grad(*args)
        dev.in_message_grad(*args, mu, Sig)                               # (the explicit one is fine)
        dev.sweep()
        dev.in_message_grad(*args)


def test_reused_sweep_and_theta_objective_are_untouched_by_the_call(G):
    c = R.reference("a")
    snaps, objectives = [], []
    for with_call in (False, True):
        dev, _, _ = swept_multi(G, c, seed=32, reuse_stats=True)
        with dev:
            dev.set_noise(2.0 * c["W"])
            before = dev.sweep_kind()
            assert before[0] == REUSED
            if with_call:
                dev.in_message_grad(c["X"], c["start"], c["Y"])
                dev.in_message_grad(c["X"], c["start"], c["Y"], c["mu_v"], c["Sigma_v"])
                assert dev.sweep_kind() == before
            dev.sweep()
            assert dev.sweep_kind()[1] == REUSED
            snaps.append(_snapshot(dev))
            if with_call:
                dev.in_message_grad(c["X"], c["start"], c["Y"])
            value, grad = dev.theta_objective(want_grad=True)
            objectives.append(np.concatenate([[value], np.ravel(grad)]))
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k
    assert np.array_equal(objectives[0], objectives[1])


def raw(dev, X, start, Y, mu, Sig, outs=(True, True, True), n=None, n_nodes=None):
    """The C entry point itself: its status, no exception."""
    from gaussianprocessnode_amd._lib import as_f64, ptr
    X = as_f64(X)
    start = np.ascontiguousarray(start, dtype=np.int64)
    n = len(X) if n is None else n
    n_nodes = len(start) - 1 if n_nodes is None else n_nodes
    D = dev.D
    bufs = [np.empty(max(n, 1)), np.empty(max(n, 1) * D), np.empty(max(n, 1) * D * D)]
    y_cm = as_f64(np.asarray(Y, dtype=np.float64).reshape(-1, dev.d_out).T)
    S = None if Sig is None else as_f64(np.asarray(Sig).T)
    return dev._lib.sgp_in_message_grad(dev._h, ptr(X), n, start.ctypes.data_as(C.POINTER(C.c_int64)), n_nodes, ptr(y_cm),
                                        None if mu is None else ptr(as_f64(mu)), ptr(S),
                                        *[ptr(b) if keep else None for b, keep in zip(bufs, outs)])


def test_statuses(G):
    c = R.reference("a")
    X, st, Y, mu, Sig = c["X"], c["start"], c["Y"], c["mu_v"], c["Sigma_v"]
    with device_for(G, c) as dev:
        assert raw(dev, X, st, Y, mu, Sig) == 0
        for bad in ([1] + list(st[1:]), list(st[:-1]) + [st[-1] - 1], list(st[:-1]) + [st[-1] + 1], [0, 10, 5, 15, 20, 25, 30, 35],
                    [0, 5, 5, 15, 20, 25, 30, 35]):                        # not from 0, not to n (both ways), decreasing, an empty node
            assert raw(dev, X, bad, Y, mu, Sig) == ERR_ARG, bad
        assert raw(dev, X, st, Y, mu, Sig, outs=(True, True, False)) == 0          # hess = NULL
        assert raw(dev, X, st, Y, mu, Sig, outs=(False, True, False)) == 0         # logpdf = NULL too
        assert raw(dev, X, st, Y, mu, Sig, outs=(True, False, True)) == ERR_ARG    # grad is required
        assert raw(dev, X, st, Y, mu, None) == ERR_ARG and raw(dev, X, st, Y, None, Sig) == ERR_ARG
        assert raw(dev, X, st, Y, None, None) == ERR_ARG                  # no sweep yet: no posterior in the handle
        assert raw(dev, X[:0], [0], Y[:0], mu, Sig, n=0, n_nodes=0) == 0  # n = 0: nothing to do
        assert dev._lib.sgp_in_message_grad(dev._h, None, 0, None, 0, None, None, None, None, None, None) == 0
        dev.set_kernel(c["sigma2"], c["ell"], c["jitter"], family="matern12")
        assert raw(dev, X, st, Y, mu, Sig) == ERR_ARG                     # a kink at every inducing input: no gradient
        dev.set_kernel(c["sigma2"], c["ell"], c["jitter"], family=c["family"])
        bad = np.array(Sig)
        bad[5, :] = bad[:, 5] = 0.0
        bad[5, 5] = -100.0
        with pytest.raises(G.PosDefException) as e:                       # S inherits the negative direction: its leading minor
            dev.in_message_grad(X, st, Y, mu, bad)
        assert e.value.info == 6
        assert raw(dev, X, st, Y, mu, Sig) == 0                           # (and the handle goes on working)
    u = R.reference("c")
    with device_for(G, u, n_max=200) as dev:                              # an open device-paced training run (UniSGP only)
        rng = np.random.default_rng(33)
        Xt = rng.uniform(-1.8, 1.8, (200, 1))
        dev.set_prior_isotropic(50.0)
        dev.train_begin(Xt, np.sin(Xt[:, 0]), np.array([0.5, 1.0]), jitter=1e-6)
        assert raw(dev, u["X"], u["start"], u["Y"], u["mu_v"], u["Sigma_v"]) == ERR_ARG
        dev.train_end()
        dev.set_kernel(u["sigma2"], u["ell"], u["jitter"])
        assert raw(dev, u["X"], u["start"], u["Y"], u["mu_v"], u["Sigma_v"]) == 0


@pytest.mark.parametrize("batch", ["case a", "pendulum"])
def test_rule_in_laplace_batch(G, batch, monkeypatch):
    """Not a comparison of two optimisers: at every converged node's m_z the CPU restatement's gradient is below the stop
    threshold plus tol_grad, W_z is the restatement's Hessian there within tol_hess, and f has not risen."""
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.device import SGPDevice
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    c = dict(R.make_case("a")) if batch == "case a" else GR.pendulum_batch()
    T = len(c["means"])
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    q_ins = [MvNormalMeanCovariance(c["means"][t], c["covs"][t]) for t in range(T)]
    q_outs = [PointMass(y) for y in c["Y"]]
    calls = [0]
    inner = SGPDevice.in_message_grad

    def counted(self, *a, **k):
        calls[0] += 1
        return inner(self, *a, **k)
    monkeypatch.setattr(SGPDevice, "in_message_grad", counted)
    try:
        marginals, records = MS.rule_in_laplace_batch(q_outs, q_ins, MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(c["W"]),
                                                      PointMass(np.concatenate([[c["sigma2"]], c["ell"]])), meta, iterations=20)
    finally:
        meta.engine.close()
    W_z = np.stack([m.W for m in marginals])
    m_z = np.stack([r["mode"] for r in records])                         # (W_z may be singular where the message is flat)
    assert all(np.array_equal(m.xi, m.W @ z) for m, z in zip(marginals, m_z))
    node = np.arange(T)
    lp, grad, hess = GR.evaluate(c, "cholesky", X=m_z, node=node)
    tg, th = GR.bounds(c, X=m_z, node=node)
    lp0 = GR.evaluate(c, "cholesky", X=c["means"], node=node)[0]
    tol = R.vector_logpdf(dict(c, X=m_z, start=np.arange(T + 1)), want_bound=True)["tol"]
    conv = np.array([r["converged"] for r in records])
    thr = np.array([r["threshold"] for r in records])
    g_ratio = GR.worst(np.abs(grad)[conv], (thr[:, None] + tg)[conv])
    h_ratio = GR.worst(np.abs(W_z + hess)[conv], th[conv])
    print(f"{batch}: {calls[0]} device calls, {int((~conv).sum())} of {T} unconverged, improper {sum(not r['proper'] for r in records)}, "
          f"gradient / (threshold + bound) {g_ratio:.3g}, W_z error / bound {h_ratio:.3g}")
    assert calls[0] <= 21
    assert np.mean(~conv) <= 0.05
    assert g_ratio <= 1.0 and h_ratio <= 1.0
    assert np.all((-lp <= -lp0 + 2 * tol)[conv])                          # f(m_z) <= f(mean(q_in)), both from the restatement
