"""sgp_sample_path on the device against the float64 reference of tests/sample_path_ref.py at its per-entry bound
(tests/test_sample_path_host.py holds the bound's constant to mpmath and shows that it sees the faults of sample_path_ref.FAULTS).

    tile0 .. tile9   M in {1, 5, 64, 65, 130}, ns in {1, 63, 64, 65, 300}, L in {1, 63, 64, 65, 200}, d_out n_samples in {1, 3, 64, 65,
                     130} through d_out 1..4, D in {1, 2, 8, 9, 32}, every family: each edge of k_path_eval's tiles (sample_path_ref.CASES)
    func, uni        the linear map column by column, the function property, the handle's own q(v), the state, the refusals
    large            ns d_out = 3 x 8192, beyond SGP_JOINT_MAX_ROWS

Every comparison prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import sample_path_ref as P

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


def path(dev, c, X=None, feat_w=None, eps_v=None):
    return dev.sample_path(c["X"] if X is None else X, c["omega"], c["phase"], c["feat_w"] if feat_w is None else feat_w,
                           c["eps_v"] if eps_v is None else eps_v, c["mu_v"], c["Sigma_v"])


def held(what, ratio):
    print(f"{what}: error / bound {ratio:.3g}")
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("name", P.group("tile"))
def test_tile_edges(G, name):
    c = P.reference(name)
    with device_for(G, c) as dev:
        f = path(dev, c)
        again = path(dev, c)
    assert f.shape == (len(c["X"]), c["d_out"], c["S"]) and np.isfinite(f).all()
    assert f.tobytes() == again.tobytes()
    held(f"case {name}", P.ratio(c, f))


def test_the_linear_map_column_by_column(G):
    """feat_w = 0, eps_v = e_q: mean + k_s' L_S[:, q]; eps_v = 0, feat_w = e_(l, i): mean + phi_l(x_s) - k_s' K^-1 Phi_u[:, l] on
    output i and the mean on the others; all zero: the predictive mean -- each to rounding, against the reference at those inputs."""
    c = P.reference("func")
    M, d_out, L, Q = c["M"], c["d_out"], c["L"], c["M"] * c["d_out"]
    X = c["X"][:70]
    qs = [0, 1, M - 1, M, Q - 1]
    ls = [(0, 0), (63, 1), (64, 0), (L - 1, 1)]
    with device_for(G, c) as dev:
        zero_w = np.zeros((L, d_out, len(qs)))
        e_q = np.zeros((Q, len(qs)))
        e_q[qs, np.arange(len(qs))] = 1.0
        f_eps = path(dev, c, X, zero_w, e_q)
        e_l = np.zeros((L, d_out, len(ls)))
        for j, (l, i) in enumerate(ls):
            e_l[l, i, j] = 1.0
        zero_e = np.zeros((Q, len(ls)))
        f_w = path(dev, c, X, e_l, zero_e)
        f_0 = path(dev, c, X, np.zeros((L, d_out, 1)), np.zeros((Q, 1)))
        mean = dev.predict(X, c["mu_v"])
    held("eps_v = e_q", P.ratio(c, f_eps, X, zero_w, e_q))
    held("feat_w = e_(l, i)", P.ratio(c, f_w, X, e_l, zero_e))
    held("all zero", P.ratio(c, f_0, X, np.zeros((L, d_out, 1)), np.zeros((Q, 1))))
    _, b0 = P.evaluate(c, X, np.zeros((L, d_out, 1)), np.zeros((Q, 1)), cond=c["cond"])
    held("all zero against sgp_predict", P.worst(np.abs(f_0[:, :, 0] - mean), b0[:, :, 0]))
    for j, (l, i) in enumerate(ls):                              # the outputs a unit feature weight does not touch: the mean
        for o in range(d_out):
            if o != i:
                held(f"feat_w = e_({l}, {i}), output {o}", P.worst(np.abs(f_w[:, o, j] - mean[:, o]), b0[:, o, 0]))


def test_a_sample_is_a_function_bitwise(G, monkeypatch):
    """A point's rows from a call over 300 points, from a call with that point alone, from calls under SGP_PREDICT_CHUNK = 64 and
    100 (read per handle), and from a call over other points in another order: bitwise the same."""
    c = P.reference("func")
    n = len(c["X"])
    alone = [0, 63, 64, 99, 100, 255, 256, n - 1]
    with device_for(G, c) as dev:
        full = path(dev, c)
        assert path(dev, c).tobytes() == full.tobytes()
        for s in alone:
            one = path(dev, c, c["X"][s:s + 1])
            assert one.shape == (1, c["d_out"], c["S"]) and one[0].tobytes() == full[s].tobytes(), s
        perm = np.random.default_rng(1).permutation(n)[:130]
        assert path(dev, c, c["X"][perm]).tobytes() == np.ascontiguousarray(full[perm]).tobytes()
    for chunk in ("64", "100"):
        monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        with device_for(G, c) as dev:
            assert path(dev, c).tobytes() == full.tobytes(), chunk
    held("case func", P.ratio(c, full))


LARGE_ROWS = sorted({0, 1, 8191} | {r for k in range(1, 8192 // 64) for r in (64 * k - 1, 64 * k)} | set(range(37, 8192, 251)))


def test_beyond_the_joint_calls_row_limit(G, monkeypatch):
    """ns d_out = 3 x 8192 in chunks of 1024: the first and last row of every chunk (and of every point block), and a stride."""
    c = P.reference("large")
    assert len(c["X"]) * c["d_out"] == 3 * G._lib.SGP_JOINT_MAX_ROWS
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "1024")
    with device_for(G, c) as dev:
        f = path(dev, c)
    assert f.shape == (8192, 3, c["S"]) and np.isfinite(f).all()
    assert {0, 1023, 1024, 7167, 7168, 8191} <= set(LARGE_ROWS)
    held("case large", P.ratio(c, f[LARGE_ROWS], rows=LARGE_ROWS))


def _swept(G, c, N=200, **kw):
    rng = np.random.default_rng(77)
    X = rng.uniform(-1.5, 1.5, (N, c["D"]))
    Y = rng.normal(size=(N, c["d_out"]))
    dev = G.SGPDevice(N, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    dev.set_data(X, Y[:, 0] if c["d_out"] == 1 else Y)
    dev.set_prior_isotropic(2.0)
    dev.sweep()
    return dev


@pytest.mark.parametrize("name", ["func", "uni"])
def test_the_handle_s_own_posterior(G, name):
    c = dict(P.reference(name))
    with _swept(G, c) as dev:
        mu, Sig, _ = dev.posterior()
        own = dev.sample_path(c["X"], c["omega"], c["phase"], c["feat_w"], c["eps_v"])
        given = dev.sample_path(c["X"], c["omega"], c["phase"], c["feat_w"], c["eps_v"], mu, Sig)
    assert own.tobytes() == given.tobytes()
    c.update(mu_v=np.asarray(mu).reshape(-1), Sigma_v=Sig)
    cond = (c["cond"][0], float(np.linalg.cond(Sig)))
    f, b = P.evaluate(c, cond=cond)
    held(f"own q(v) of {name}, cond(Sigma_v) {cond[1]:.3g}", P.worst(np.abs(own - f), b))


def _state(dev):
    mu, Sig, Uv = dev.posterior()
    return [mu, Sig, Uv, np.array(dev.sweep_kind()), *dev.stats(), np.array([dev.theta_objective()]).ravel()]


@pytest.mark.parametrize("reuse", [False, True])
def test_nothing_the_sweep_keeps_is_written(G, reuse):
    c = P.reference("uni")
    calls = []

    def run(with_call):
        with _swept(G, c, reuse_stats=reuse) as dev:
            dev.set_allreduce(lambda buf, count, stream: calls.append(count) or 0)
            dev.sweep()
            before = _state(dev)
            if with_call:
                n_calls = len(calls)
                dev.sample_path(c["X"], c["omega"], c["phase"], c["feat_w"], c["eps_v"])
                path(dev, c)
                assert len(calls) == n_calls                 # an installed hook is neither called nor a reason to refuse
                assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _state(dev)))
            dev.sweep()
            return before + _state(dev)

    plain, called = run(False), run(True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, called))


class Call:
    """The raw ABI with the case's valid arguments, any of them replaced by keyword; the outputs start as a pattern."""

    def __init__(self, dev, c):
        from gaussianprocessnode_amd._lib import as_f64, ptr
        self.dev, self.lib, self.ptr = dev, dev._lib, ptr
        self.a = dict(X=as_f64(c["X"]), ns=len(c["X"]), mu=as_f64(c["mu_v"]), Sig=as_f64(np.asarray(c["Sigma_v"]).T),
                      om=as_f64(c["omega"].T), ph=as_f64(c["phase"]), L=c["L"], w=as_f64(c["feat_w"].transpose(2, 1, 0)),
                      eps=as_f64(c["eps_v"].T), n=c["S"], flags=0)
        self.out = np.full((c["S"], c["d_out"], len(c["X"])), 7.25)
        self.info = (C.c_int64 * 2)(-5, -5)

    def run(self, **kw):
        a = {**self.a, "out": self.out, **kw}
        p = lambda v: None if v is None else self.ptr(v)
        return self.lib.sgp_sample_path(self.dev._h, p(a["X"]), a["ns"], p(a["mu"]), p(a["Sig"]), p(a["om"]), p(a["ph"]), a["L"],
                                        p(a["w"]), p(a["eps"]), a["n"], a["flags"], p(a["out"]), self.info)

    def refused(self, text, **kw):
        rc = self.run(**kw)
        msg = self.lib.sgp_last_error(self.dev._h).decode()
        assert rc == ERR_ARG and msg == f"sgp_sample_path: {text}", (rc, msg)
        assert (self.out == 7.25).all() and list(self.info) == [-5, -5]         # the outputs are untouched


def test_refusals_leave_the_outputs_untouched(G):
    c = P.reference("uni")
    rng = np.random.default_rng(5)
    N = 100
    X, y = rng.uniform(-1.5, 1.5, (N, c["D"])), rng.normal(size=N)
    with G.SGPDevice(N, c["M"], c["D"], 1) as dev:
        k = Call(dev, c)
        k.refused("set_inducing and set_kernel first")
        dev.set_inducing(c["Xu"])
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
        dev.set_noise(c["W"])
        for flags in (1, 2, -1):
            k.refused("unknown flags", flags=flags)
        k.refused("bad argument", ns=-1)
        k.refused("pass both mu_v and Sigma_v, or neither", mu=None)
        k.refused("pass both mu_v and Sigma_v, or neither", Sig=None)
        k.refused("no posterior in the handle and mu_v / Sigma_v are NULL", mu=None, Sig=None)
        k.refused("null Xstar or samples", X=None)
        k.refused("null Xstar or samples", out=None)
        for key in ("om", "ph", "w", "eps"):
            k.refused("null omega, phase, feat_w or eps_v", **{key: None})
        for L in (0, -1, G._lib.SGP_PATH_MAX_FEATURES + 1):
            k.refused("L must lie in 1 .. SGP_PATH_MAX_FEATURES (16384)", L=L)
        for n in (0, -3):
            k.refused("need n_samples >= 1", n=n)
        k.refused("d_out * n_samples exceeds SGP_PATH_MAX_COLUMNS (2097152)", n=G._lib.SGP_PATH_MAX_COLUMNS + 1)
        for key, text in (("X", "Xstar must be finite"), ("om", "omega and phase must be finite"),
                          ("ph", "omega and phase must be finite"), ("w", "feat_w and eps_v must be finite"),
                          ("eps", "feat_w and eps_v must be finite")):
            for bad_value in (np.nan, np.inf):
                bad = k.a[key].copy()
                bad.reshape(-1)[-1] = bad_value
                k.refused(text, **{key: bad})
        assert k.run(ns=0, X=None, out=None) == 0 and (k.out == 7.25).all()          # no points: nothing done
        dev.set_data(X, y)
        dev.set_prior_isotropic(5.0)
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
        dev.set_posterior(mu, Uv)
        k.refused("sgp_set_posterior gave no Sigma_v: pass mu_v and Sigma_v, or sweep first", mu=None, Sig=None)
        dev.sweep()
        dev.train_begin(X, y, np.zeros(1 + c["D"]))
        k.refused("a device-paced training run is open (sgp_train_end first)")
        dev.train_end()
        dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])     # (the run left its own kernel parameters)
        assert G._lib.load().sgp_sample_path(None, None, 1, None, None, None, None, 1, None, None, 1, 0, None, None) == ERR_ARG
        assert k.run() == 0 and list(k.info) == [0, 0] and not (k.out == 7.25).any()
        held("the raw call", P.ratio(c, k.out.transpose(2, 1, 0)))


def test_failed_factorisations_report_their_minor(G):
    c = P.reference("uni")
    with device_for(G, c) as dev:
        k = Call(dev, c)
        Sig = np.asarray(c["Sigma_v"]).copy()
        Sig[9, 9] = -1.0
        rc = k.run(Sig=np.ascontiguousarray(Sig.T))
        assert rc == 10 and dev._lib.sgp_last_error(dev._h).decode() == "Sigma_v is not positive definite"
        assert list(k.info) == [0, 10] and (k.out == 7.25).all()
        Xu = c["Xu"].copy()
        Xu[17] = Xu[5]
        dev.set_inducing(Xu)
        dev.set_kernel(c["sigma2"], c["ell_dev"], 0.0, family=c["family"])
        rc = k.run()
        assert 0 < rc <= c["M"] and dev._lib.sgp_last_error(dev._h).decode() == "K_uu (current kernel) is not positive definite"
        assert list(k.info) == [rc, 0] and (k.out == 7.25).all()


# ---- the Python layers ------------------------------------------------------------------------------------------------------------
def _gpssm(c):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=c["jitter"])
    return (meta, MvNormalMeanCovariance(c["mu_v"], c["Sigma_v"]), PointMass(c["W"]),
            PointMass(np.concatenate([[c["sigma2"]], c["ell"]])))


def test_sample_paths_is_one_device_call_from_the_seed(G):
    from gaussianprocessnode_amd import train
    c = P.reference("tile8")                                    # SE, D = 2, d_out = 1 ... through the MultiSGP engine
    meta, q_v, q_w, q_theta = _gpssm(c)
    try:
        smp = train.sample_paths(meta, c["X"], 4, np.random.default_rng(3), q_v=q_v, q_theta=q_theta, features=50)
        again = train.sample_paths(meta, c["X"], 4, np.random.default_rng(3), q_v=q_v, q_theta=q_theta, features=50)
        noisy = train.sample_paths(meta, c["X"], 4, np.random.default_rng(3), q_v=q_v, q_theta=q_theta, features=50, q_w=q_w,
                                   noise=True)
        rng = np.random.default_rng(3)
        omega, phase = train.path_features("se", c["D"], 50, rng)
        w, e = rng.standard_normal((50, 1, 4)), rng.standard_normal((c["M"], 4))
        direct = meta.engine.sample_path(c["X"], omega, phase, w, e, c["mu_v"], c["Sigma_v"])
        z = rng.standard_normal((4, len(c["X"]), 1))
    finally:
        meta.engine.close()
    assert smp.shape == (4, len(c["X"]), 1) and smp.tobytes() == again.tobytes()
    assert np.array_equal(smp, direct.transpose(2, 0, 1))
    assert np.allclose(noisy, smp + z / np.sqrt(c["W"][0, 0]), rtol=1e-13, atol=1e-15)


def test_rollout_draws_each_function_once(G):
    """Two paths fed the same state return the same next state for the same path index across two steps; the rollout without noise
    is reproducible from the seed and is the diagonal of the device call at every step."""
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    c = dict(P.reference("func"))                                # D = 3, d_out = 2: not a transition
    meta, q_v, q_w, q_theta = _gpssm(c)
    try:
        with pytest.raises(ValueError):
            train.rollout_gpssm_paths(PointMass(np.zeros(3)), 2, 4, np.random.default_rng(0), q_v=q_v, q_w=q_w, q_theta=q_theta, meta=meta)
    finally:
        meta.engine.close()
    t = P.make_case("func")
    t.update(P.R.make_shape_case(M=40, D=2, d_out=2, family="se", sizes=[4], seed=3400, jitter=P.PS.SHARP_JITTER))
    meta, q_v, q_w, q_theta = _gpssm(t)
    n_paths, steps, L = 5, 2, 30
    x0 = np.array([0.3, -0.4])
    try:
        kw = dict(q_v=q_v, q_w=q_w, q_theta=q_theta, meta=meta, features=L, noise=False)
        traj = train.rollout_gpssm_paths(PointMass(x0), steps, n_paths, np.random.default_rng(9), **kw)
        again = train.rollout_gpssm_paths(PointMass(x0), steps, n_paths, np.random.default_rng(9), **kw)
        spread = train.rollout_gpssm_paths(MvNormalMeanCovariance(x0, 0.01 * np.eye(2)), steps, n_paths, np.random.default_rng(9), **kw)
        noisy = train.rollout_gpssm_paths(PointMass(x0), steps, n_paths, np.random.default_rng(9), **dict(kw, noise=True))
        rng = np.random.default_rng(9)
        omega, phase = train.path_features("se", 2, L, rng)
        w, e = rng.standard_normal((L, 2, n_paths)), rng.standard_normal((80, n_paths))
        f = lambda X: meta.engine.sample_path(X, omega, phase, w, e, t["mu_v"], t["Sigma_v"])
        first = f(np.tile(x0, (n_paths, 1)))                     # every path at the same state
        second = f(traj[1])
    finally:
        meta.engine.close()
    assert traj.shape == (steps + 1, n_paths, 2) and traj.tobytes() == again.tobytes()
    assert np.array_equal(traj[0], np.tile(x0, (n_paths, 1)))
    for j in range(n_paths):
        # the state x0 fed at any position returns path j's next state; so does path j's own state one step on
        assert all(first[s, :, j].tobytes() == traj[1, j].tobytes() for s in range(n_paths))
        assert second[j, :, j].tobytes() == traj[2, j].tobytes()
    assert len({traj[1, j].tobytes() for j in range(n_paths)}) == n_paths            # the functions differ
    assert spread.shape == traj.shape and not np.array_equal(spread[0], traj[0])
    assert noisy.shape == traj.shape and not np.array_equal(noisy[1], traj[1])
