"""sgp_theta_descend on the device: `steps` AdaMax steps on the raw kernel parameters at a held q(v), paced by the device, for
UniSGP and MultiSGP handles -- against the host-paced loop on the same handle (set_kernel, theta_objective, train.AdaMax) and the
NumPy restatement of tests/theta_descend_ref.py, its first value against sgp_theta_objective, bitwise repeatability and
continuation through the optimiser state, the stop on a K_uu that is not positive definite, the state the call leaves, the
refusals, and `train.optimize_theta_multi(device_paced=True)`.

Shapes (tests/theta_descend_ref.py, SHAPES): one tile with one shared SE lengthscale (d_out 1, M 20); the pendulum (d_out 2, M 48
on the 8 x 6 grid, 60 nodes x 5 cubature points, jitter 1e-12, 100 steps); two padded tiles with ARD Matern-3/2 (d_out 4, D 5,
M 96); three tiles, Q = 390, one shared Matern-1/2 lengthscale (d_out 3, M 130); d_out 1 with point weights, ARD Matern-5/2,
M 130.  tests/test_theta_descend_host.py shows that the reference loop moves theta by more than 1e-3 relative in each."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from gaussianprocessnode_amd import train as TR
from oracle import sgp_oracle as O
from tests import theta_descend_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-6          # what test_pendulum_inner_loop_matches_the_numpy_gradient grants two implementations of this loop


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def open_handle(G, case, *, jitter=None, reuse=False, sweep=True):
    """A handle with the case's data, noise, prior and the kernel softplus(theta0), swept once unless told not to."""
    dev = G.SGPDevice(len(case["X"]), case["M"], case["D"], case["d_out"], reuse_stats=reuse)
    dev.set_inducing(case["Xu"])
    y = case["Y"] if case["d_out"] > 1 else case["Y"][:, 0]
    dev.set_data(case["X"], y, weights=case["omega"] if case["weighted"] else None,
                 n_nodes=case["n_nodes"] if case["n_nodes"] != len(case["X"]) else None)
    set_kernel(dev, case, case["theta0"], jitter)
    dev.set_prior_isotropic(50.0)
    dev.set_noise(case["W"], float(np.linalg.slogdet(case["W"])[1]))
    if sweep:
        dev.sweep()
    return dev


def set_kernel(dev, case, theta, jitter=None):
    p = O.softplus(np.asarray(theta, dtype=np.float64))
    dev.set_kernel(p[0], p[1:], case["jitter"] if jitter is None else jitter, family=case["family"])


def host_paced(dev, case, steps):
    """The loop as `train.optimize_theta_multi` paces it from the host: per step set_kernel, theta_objective, train.AdaMax."""
    theta = case["theta0"].copy()
    opt = TR.AdaMax(eta=case["eta"])
    values = np.empty(steps)
    for k in range(steps):
        set_kernel(dev, case, theta)
        values[k], g = dev.theta_objective(want_grad=True, n_ell=case["n_ell"])
        opt.update(theta, g * TR.sigmoid(theta))
    return theta, values, opt.get_state(theta)


@functools.lru_cache(maxsize=None)
def runs(name):
    """Per case, computed once and shared (arrays not to be written to): the device-paced call on a fresh handle, the host-paced
    loop on the SAME handle afterwards (the kernel set back to theta0 by its first step), and the NumPy loop at the handle's q(v)."""
    import gaussianprocessnode_amd as G
    case = R.get_case(name)
    with open_handle(G, case) as dev:
        mu, Sigma, _ = dev.posterior(want_uv=False)
        got = dev.theta_descend(case["theta0"], case["steps"], eta=case["eta"])
        host = host_paced(dev, case, case["steps"])
    ref = R.descend(case, mu, Sigma, case["theta0"], case["steps"], eta=case["eta"])
    return dict(got=got, host=host, ref=ref)


def same(a, b):
    """bitwise equality of two theta_descend results (theta, values, steps taken, state)"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2] and np.array_equal(a[3], b[3])


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_against_the_host_paced_loop_and_the_numpy_loop(G, name):
    case, r = R.get_case(name), runs(name)
    theta, values, taken, state = r["got"]
    assert taken == case["steps"] and np.all(np.isfinite(values))
    assert np.max(np.abs(theta - case["theta0"]) / np.abs(case["theta0"])) > 1e-3           # the loop went somewhere
    for other in ("host", "ref"):
        th_o, val_o, st_o = r[other]
        print(f"ERR {name} vs {other}: theta {np.max(np.abs(theta - th_o) / np.abs(th_o)):.3g}, "
              f"values {np.max(np.abs(values - val_o) / np.abs(val_o)):.3g}")
    for other in ("host", "ref"):
        th_o, val_o, st_o = r[other]
        np.testing.assert_allclose(theta, th_o, rtol=RTOL, err_msg=other)
        np.testing.assert_allclose(values, val_o, rtol=RTOL, err_msg=other)
    assert state[-2] == r["host"][2][-2] and state[-1] == r["host"][2][-1]                    # the powers: the same products


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_first_value_is_the_theta_objective_re_evaluated(G, name):
    case = R.get_case(name)
    with open_handle(G, case) as dev:
        set_kernel(dev, case, case["theta0"] + 0.05)
        dev.theta_objective(want_grad=True)                                                  # re-evaluated at another theta
        set_kernel(dev, case, case["theta0"])
        v_re = dev.theta_objective(want_grad=False)                                          # ... and at theta0, not the fresh path
    v0 = runs(name)["got"][1][0]
    assert abs(v0 - v_re) <= 1e-12 * abs(v_re), (v0, v_re)


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uni_m130_d3_ard_m52_weights", "d3_m130_d2_iso_m12"])
def test_two_identical_calls_agree_bitwise(G, name):
    case = R.get_case(name)
    with open_handle(G, case) as dev:
        again = dev.theta_descend(case["theta0"], case["steps"], eta=case["eta"])
    assert same(again, runs(name)["got"])


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uni_m20_d1_iso_se", "d4_m96_d5_ard_m32"])
def test_continuation_through_the_state_and_the_null_state(G, name):
    case = R.get_case(name)
    whole = runs(name)["got"]
    with open_handle(G, case) as dev:
        th4, v4, n4, st4 = dev.theta_descend(case["theta0"], 4, eta=case["eta"])
        th8, v8, n8, st8 = dev.theta_descend(th4, 4, eta=case["eta"], state=st4)
    assert same((th8, np.concatenate([v4, v8]), n4 + n8, st8), whole)
    # a NULL opt_state through the C ABI: zero moments, powers (beta1, beta2), no state returned
    with open_handle(G, case) as dev:
        th = case["theta0"].copy()
        values = np.empty(case["steps"])
        counts = (C.c_int64 * 2)()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = dev._lib.sgp_theta_descend(dev._h, dp(th), case["n_ell"], case["steps"], case["eta"], 0.9, 0.999, 1e-8, None, dp(values),
                                        counts)
    assert rc == 0 and counts[0] == case["steps"] and counts[1] == 0
    assert np.array_equal(th, whole[0]) and np.array_equal(values, whole[1])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def singular_case():
    """Four identical inducing inputs, jitter 0 and sigma2 = softplus(64) = 64 exactly: K_uu's second pivot is 64 - 64 * 64 / 64 = 0
    (the recipe of test_rejected_minibatches_leave_theta_alone_and_the_handle_usable: an info flag, not a fault)."""
    rng = np.random.default_rng(31)
    n, M, D = 120, 12, 2
    X = rng.uniform(-1.7, 1.7, (n, D))
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    Xu[1:4] = Xu[0]
    Y = np.sin(X @ rng.normal(size=(D, 1)))
    theta0 = np.array([64.0, *O.invsoftplus(np.array([0.9, 1.1]))])
    mu = rng.normal(size=M)
    L = rng.normal(size=(M, M)) / M
    Uv = np.linalg.cholesky(L @ L.T + 0.05 * np.eye(M) + np.outer(mu, mu)).T
    case = dict(name="singular", d_out=1, D=D, M=M, family="se", jitter=0.0, X=X, omega=np.ones(n), Y=Y, n_nodes=n, Xu=Xu,
                W=np.array([[20.0]]), theta0=theta0, n_ell=2, steps=8, eta=0.01, weighted=False)
    return case, mu, Uv


def test_stop_on_a_singular_kuu_leaves_theta_and_a_usable_handle(G):
    case, mu, Uv = singular_case()
    with open_handle(G, case, sweep=False) as dev:
        dev.set_posterior(mu, Uv)                                                            # q(v): no sweep at a singular K_uu
        with pytest.raises(np.linalg.LinAlgError, match="step 0") as exc:
            dev.theta_descend(case["theta0"], case["steps"], eta=case["eta"])
        e = exc.value
        assert e.minor > 0 and e.steps_taken == 0
        assert np.array_equal(e.theta, case["theta0"]) and np.all(np.isnan(e.values)) and len(e.values) == case["steps"]
        assert np.array_equal(e.state, np.concatenate([np.zeros(6), [0.9, 0.999]]))
        set_kernel(dev, case, case["theta0"], jitter=1e-6)
        after = dev.theta_descend(case["theta0"], case["steps"], eta=case["eta"])
    with open_handle(G, case, sweep=False, jitter=1e-6) as clean:
        clean.set_posterior(mu, Uv)
        want = clean.theta_descend(case["theta0"], case["steps"], eta=case["eta"])
    assert want[2] == case["steps"] and np.all(np.isfinite(want[1]))
    assert same(after, want)


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uni_m20_d1_iso_se", "pendulum"])
def test_state_after_the_call(G, name):
    case = R.get_case(name)
    steps = 8
    with open_handle(G, case, reuse=True) as dev:
        assert dev.sweep_kind()[0] != G._lib.SGP_SWEEP_FULL                                  # (a second sweep would reuse the statistics)
        before = dev.posterior()
        theta, _, taken, _ = dev.theta_descend(case["theta0"], steps, eta=case["eta"])
        assert dev.sweep_kind()[0] == G._lib.SGP_SWEEP_FULL
        after = dev.posterior()
        v, g = dev.theta_objective(want_grad=True, n_ell=case["n_ell"])
    assert taken == steps
    for a, b in zip(before, after):
        assert np.array_equal(a, b)                                                          # q(v) untouched
    with open_handle(G, case) as fresh:
        set_kernel(fresh, case, theta)
        v_f, g_f = fresh.theta_objective(want_grad=True, n_ell=case["n_ell"])
    assert abs(v - v_f) <= 1e-12 * abs(v_f), (v, v_f)
    np.testing.assert_allclose(g, g_f, rtol=1e-9, atol=1e-9 * np.abs(g_f).max())             # (the issue sets the value's bound only)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(G):
    uni, multi, wide = R.get_case("uni_m20_d1_iso_se"), R.get_case("pendulum"), R.get_case("d4_m96_d5_ard_m32")
    with open_handle(G, uni, sweep=False) as dev:
        with pytest.raises(G.SGPError, match="q\\(v\\)"):
            dev.theta_descend(uni["theta0"], 2)                                              # no sweep, no sgp_set_posterior
        dev.set_allreduce(lambda buf, count, stream: None)                                   # single rank: the sum is the identity
        dev.sweep()
        with pytest.raises(G.SGPError, match="hook"):
            dev.theta_descend(uni["theta0"], 2)                                              # data-sharded, d_out = 1
        dev.set_allreduce(None)
        dev.sweep()
        with pytest.raises(G.SGPError, match="steps"):
            dev.theta_descend(uni["theta0"], -1)
        bad = np.concatenate([np.zeros(4), [1.0, 0.999]])
        with pytest.raises(G.SGPError, match="powers"):
            dev.theta_descend(uni["theta0"], 2, state=bad)                                   # beta1^t = 1: no step was ever taken
        th, values, taken, state = dev.theta_descend(uni["theta0"], 0)                       # steps = 0: the input, unchanged
        assert np.array_equal(th, uni["theta0"]) and len(values) == 0 and taken == 0
        assert np.array_equal(state, np.concatenate([np.zeros(4), [0.9, 0.999]]))
        dev.train_begin(uni["X"], uni["Y"][:, 0], uni["theta0"], jitter=uni["jitter"])
        with pytest.raises(G.SGPError, match="training run"):
            dev.theta_descend(uni["theta0"], 2)                                              # an open sgp_train_* run
        dev.train_end()
    with open_handle(G, multi, sweep=False) as dev:
        dev.set_allreduce(lambda buf, count, stream: None)
        dev.sweep()
        with pytest.raises(G.SGPError, match="hook"):
            dev.theta_descend(multi["theta0"], 2)                                            # data-sharded, d_out = 2
    with open_handle(G, wide) as dev:
        with pytest.raises(G.SGPError, match="n_ell"):
            dev.theta_descend(wide["theta0"][:3], 2)                                         # n_ell = 2 with D = 5


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_optimize_theta_multi_device_paced_continues_one_optimiser(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.cubature import SphericalRadialCubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass, WishartFast
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    means, covs, Y = R.pendulum(60)
    Xu = R.pendulum_grid()
    M = len(Xu)
    meta = MultiSGPMeta(SphericalRadialCubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-12)
    theta0 = O.invsoftplus(np.array([1.0, 0.4, 1.0]))
    q_ins = [MvNormalMeanCovariance(m, P) for m, P in zip(means, covs)]
    q_w = WishartFast(100.0, np.eye(2))
    try:
        q_v = MS.sweep(meta, [PointMass(y) for y in Y], q_ins, q_w, PointMass(theta0),
                       MvNormalMeanCovariance(np.zeros(2 * M), 50.0 * np.eye(2 * M)))
        th_host = TR.optimize_theta_multi(theta0.copy(), Y, q_ins, q_v, q_w, meta, steps=100, optimizer=TR.AdaMax())
        opt = TR.AdaMax()
        th_dev = theta0.copy()
        for _ in range(2):
            out = TR.optimize_theta_multi(th_dev, Y, q_ins, q_v, q_w, meta, steps=50, optimizer=opt, device_paced=True)
            assert out is th_dev
    finally:
        if meta.engine is not None:
            meta.engine.close()
    assert not np.allclose(th_host, theta0)
    np.testing.assert_allclose(th_dev, th_host, rtol=RTOL)
    assert math.isclose(opt.get_state(th_dev)[-2], 0.9 ** 101, rel_tol=1e-13)                # 100 steps of ONE optimiser
