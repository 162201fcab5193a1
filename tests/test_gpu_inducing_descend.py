"""sgp_inducing_descend on the device: AdaMax on [theta | vec Xu] at a held q(v), paced by the device -- against the host-paced
`train.optimize_inducing` on the same handle, the NumPy loop (tests/inducing_descend_ref.py), `theta_objective_xu` for the first
value, repeatability and continuation, learn_theta=False, the stop, the state the call leaves, the refusals and
`train.optimize_inducing(device_paced=True)`.  Shapes: tests/inducing_descend_ref.py, POINT_SHAPES.

Bounds.  Against the host-paced loop (the same device gradients, NumPy's optimiser arithmetic): theta and the values to RTOL = 1e-6,
Xu to 1e-6 max|Xu|.  Against the NumPy loop: theta and the values to RTOL, Xu to XU_ATOL = 1e-2 steps eta absolute -- the two
gradient routes agree to rtol 1e-6 + atol 1e-9 max|grad| (tests/test_gpu_xu_grad.py), and u_i >= |g_i(0)| >= 1e-6 max|grad| (the
sign-flip condition, asserted on the CPU), so each update m / u is off by at most about 2e-3 eta; summed over the steps, with slack
for the drift of the trajectory.  The measured errors are printed and recorded in profiles/inducing_descend.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussianprocessnode_amd import train as TR
from tests import inducing_descend_ref as IR

pytestmark = pytest.mark.gpu

RTOL, STEPS, ETA = IR.RTOL, IR.STEPS, IR.ETA
KW = dict(eta=ETA, beta=IR.BETA, eps=IR.EPS)


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def qv(c):
    return c["mu"], np.linalg.cholesky(c["Rv"]).T


def open_handle(G, c, *, jitter=None, Xu=None, theta=None, reuse=False):
    """A handle with the case's data, noise, kernel softplus(theta0), inducing inputs and q(v) installed"""
    dev = G.SGPDevice(c["N"], c["M"], c["D"], c["d_out"], reuse_stats=reuse)
    dev.set_inducing(c["Xu"] if Xu is None else Xu)
    dev.set_data(c["X"], c["Y"] if c["d_out"] > 1 else c["Y"][:, 0], weights=c["om"] if c["weighted"] else None)
    p = IR.softplus(c["theta0"] if theta is None else theta)
    dev.set_kernel(float(p[0]), p[1:], c["jitter"] if jitter is None else jitter, family=c["family"])
    dev.set_prior_isotropic(50.0)
    dev.set_noise(c["W"], float(np.linalg.slogdet(c["W"])[1]))
    dev.set_posterior(*qv(c))
    return dev


@functools.lru_cache(maxsize=None)
def runs(name, learn_theta=True):
    """Per shape, once (arrays not to be written to): the device-paced call and, on the same handle, the host-paced loop"""
    import gaussianprocessnode_amd as G
    c = IR.case(name)
    with open_handle(G, c) as dev:
        got = dev.inducing_descend(c["theta0"], c["Xu"], STEPS, learn_theta=learn_theta, **KW)
        host = TR.optimize_inducing(c["theta0"], c["Xu"], dev, q_v=qv(c), steps=STEPS, optimizer=TR.AdaMax(**KW),
                                    learn_theta=learn_theta, jitter=c["jitter"])
    return got, host


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(IR.POINT_SHAPES))
def test_matches_the_host_paced_loop_and_the_numpy_loop(G, name):
    c = IR.case(name)
    (th, Z, vals, taken, state), (th_h, Z_h, vals_h) = runs(name)
    th_r, Z_r, vals_r, state_r = IR.reference(name)
    assert taken == STEPS and Z.shape == (c["M"], c["D"]) and state.size == 2 * (th.size + Z.size) + 2
    e_host = (np.abs(th / th_h - 1).max(), np.abs(vals / vals_h - 1).max(), np.abs(Z - Z_h).max() / np.abs(Z_h).max())
    e_ref = (np.abs(th / th_r - 1).max(), np.abs(vals / vals_r - 1).max(), np.abs(Z - Z_r).max())
    print(f"inducing_descend {name}: vs host-paced theta {e_host[0]:.2e} values {e_host[1]:.2e} Xu/max|Xu| {e_host[2]:.2e}; "
          f"vs NumPy theta {e_ref[0]:.2e} values {e_ref[1]:.2e} Xu abs {e_ref[2]:.2e} (bound {IR.XU_ATOL:.1e})")
    np.testing.assert_allclose(th, th_h, rtol=RTOL)
    np.testing.assert_allclose(vals, vals_h, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_h, rtol=0, atol=1e-6 * np.abs(Z_h).max())
    np.testing.assert_allclose(th, th_r, rtol=RTOL)
    np.testing.assert_allclose(vals, vals_r, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_r, rtol=0, atol=IR.XU_ATOL)
    P = th.size + Z.size
    np.testing.assert_allclose(state[2 * P:], state_r[2 * P:], rtol=1e-14)


@pytest.mark.parametrize("name", ["a", "d"])
def test_first_value_is_theta_objective_xu_at_the_same_state(G, name):
    """learn_theta=False leaves the kernel at softplus(theta0) as the device forms it; with Xu0 and q(v) put back, theta_objective_xu
    re-evaluates exactly what step 0 evaluated."""
    c = IR.case(name)
    with open_handle(G, c) as dev:
        _, _, vals, _, _ = dev.inducing_descend(c["theta0"], c["Xu"], 1, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"])
        dev.set_posterior(*qv(c))
        v, _, _ = dev.theta_objective_xu(want_grad=True)
    assert vals[0] == v and vals[0] == runs(name)[0][2][0] == runs(name, False)[0][2][0]


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_repeatable_and_continued_through_the_state(G, name):
    c = IR.case(name)
    one = runs(name)[0]
    k = 6
    with open_handle(G, c) as dev:
        again = dev.inducing_descend(c["theta0"], c["Xu"], STEPS, **KW)
        dev.set_posterior(*qv(c))
        th1, Z1, v1, n1, s1 = dev.inducing_descend(c["theta0"], c["Xu"], k, **KW)
        th2, Z2, v2, n2, s2 = dev.inducing_descend(th1, Z1, STEPS - k, state=s1, **KW)
    assert same(one, again)
    assert same(one, (th2, Z2, np.concatenate([v1, v2]), n1 + n2, s2))
    # a state from train.AdaMax: k host-paced steps, then the rest on the device
    opt = TR.AdaMax(**KW)
    x = np.concatenate([c["theta0"], c["Xu"].ravel()])
    nt = c["theta0"].size
    with open_handle(G, c) as dev:
        for _ in range(k):
            p = IR.softplus(x[:nt])
            dev.set_kernel(float(p[0]), p[1:], c["jitter"])
            dev.set_inducing(x[nt:].reshape(c["M"], c["D"]))
            dev.set_posterior(*qv(c))
            _, g, gx = dev.theta_objective_xu(want_grad=True)
            opt.update(x, np.concatenate([g * TR.sigmoid(x[:nt]), gx.ravel()]))
        th3, Z3, _, _, s3 = dev.inducing_descend(x[:nt], x[nt:].reshape(c["M"], c["D"]), STEPS - k, state=opt.get_state(x), **KW)
    np.testing.assert_allclose(th3, one[0], rtol=RTOL)
    np.testing.assert_allclose(Z3, one[1], rtol=0, atol=1e-6 * np.abs(one[1]).max())
    np.testing.assert_allclose(s3[-2:], one[4][-2:], rtol=1e-14)


@pytest.mark.parametrize("name", ["a", "b"])
def test_learn_theta_false_moves_xu_alone(G, name):
    c = IR.case(name)
    (th, Z, vals, taken, state), (th_h, Z_h, vals_h) = runs(name, False)
    assert np.array_equal(th, c["theta0"]) and taken == STEPS and state.size == 2 * Z.size + 2
    spread = c["Xu"].max() - c["Xu"].min()
    assert np.abs(Z - c["Xu"]).max() > 1e-3 * spread
    np.testing.assert_allclose(vals, vals_h, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_h, rtol=0, atol=1e-6 * np.abs(Z_h).max())
    _, Z_r, vals_r, _ = IR.reference(name, False)
    np.testing.assert_allclose(Z, Z_r, rtol=0, atol=IR.XU_ATOL)
    # the kernel stays what the device formed from theta0: a second call changes no bit of it
    with open_handle(G, c) as dev:
        dev.inducing_descend(c["theta0"], c["Xu"], 2, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"]); dev.set_posterior(*qv(c))
        v1, g1 = dev.theta_objective(want_grad=True)
        dev.inducing_descend(c["theta0"], c["Xu"], 3, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"]); dev.set_posterior(*qv(c))
        v2, g2 = dev.theta_objective(want_grad=True)
    assert v1 == v2 and np.array_equal(g1, g2)


def test_stop_on_two_identical_inducing_rows(G):
    """Identical inducing rows, jitter 0 and sigma2 = softplus(64) = 64 exactly: K_uu's second pivot is 64 - 64 * 64 / 64 = 0 (the recipe
    of tests/test_gpu_theta_descend.py: an info flag, not a fault)."""
    c = IR.case("a")
    Xu = c["Xu"].copy()
    Xu[1:4] = Xu[0]
    th0 = c["theta0"].copy()
    th0[0] = 64.0
    with open_handle(G, c, jitter=0.0, Xu=Xu, theta=th0) as dev:
        with pytest.raises(np.linalg.LinAlgError) as ei:
            dev.inducing_descend(th0, Xu, 5, **KW)
        e = ei.value
        assert e.minor > 0 and e.steps_taken == 0 and np.isnan(e.values).all() and len(e.values) == 5
        assert np.array_equal(e.theta, th0) and np.array_equal(e.Xu, Xu)
        assert np.array_equal(e.state, np.concatenate([np.zeros(2 * (th0.size + Xu.size)), IR.BETA]))
        th, Z = th0.copy(), Xu.copy()
        counts = (C.c_int64 * 2)()
        from gaussianprocessnode_amd._lib import ptr
        rc = dev._lib.sgp_inducing_descend(dev._h, ptr(th), th.size - 1, ptr(Z), 3, 4, ETA, 0.9, 0.999, 1e-8, None, None, counts)
        assert rc == e.minor and list(counts) == [0, e.minor]
        assert np.array_equal(th, th0) and np.array_equal(Z, Xu)


def test_state_afterwards(G):
    c = IR.case("d")
    with open_handle(G, c, reuse=True) as dev:
        dev.sweep()
        dev.sweep()
        assert dev.sweep_kind()[0] != 0                                     # the next sweep would reuse the statistics
        mu, Sig, Uv = dev.posterior()
        th, Z, vals, _, _ = dev.inducing_descend(c["theta0"], c["Xu"], STEPS, **KW)
        assert dev.sweep_kind()[0] == 0                                     # SGP_SWEEP_FULL
        v, g, gx = dev.theta_objective_xu(want_grad=True)                   # no set_posterior: q(v) is still the sweep's
        Xs = c["X"][:40]
        pred = dev.predict(Xs)
    with open_handle(G, c, Xu=Z, theta=th) as fresh:
        fresh.set_posterior(mu, Uv)
        v0, g0, gx0 = fresh.theta_objective_xu(want_grad=True)
        pred0 = fresh.predict(Xs, mu_v=mu)
    np.testing.assert_allclose(v, v0, rtol=RTOL)
    np.testing.assert_allclose(g, g0, rtol=RTOL, atol=1e-9 * np.abs(g0).max())
    np.testing.assert_allclose(gx, gx0, rtol=RTOL, atol=1e-9 * np.abs(gx0).max())
    np.testing.assert_allclose(pred, pred0, rtol=RTOL, atol=1e-9 * np.abs(pred0).max())
    assert np.abs(Z - c["Xu"]).max() > 1e-3


@pytest.mark.parametrize("op", ["theta_descend_3", "theta_descend_psi_3", "inducing_descend_3", "inducing_descend_psi_3"])
def test_all_four_descents_leave_the_handle_at_what_they_return(G, op):
    """The four descents share one teardown: after three steps of each, on a handle whose next sweep would have reused its statistics,
    that sweep is what tests/call_sequence_ref.py says for the call, and the next objective -- q(v) still the sweep's, no setter in
    between -- is that of a fresh handle given the returned theta and Xu, to the bound of test_state_afterwards (RTOL: the host's
    softplus is not the device's to the last bit).  Point pair: shape a; exact-Psi pair: shape e, its means as the resident points."""
    from tests import call_sequence_ref as CR
    psi, inducing = "psi" in op, op.startswith("inducing")
    c = IR.case("e" if psi else "a")
    X, Y = (c["mean"], c["Y"]) if psi else (c["X"], c["Y"][:, 0])
    gauss = (c["mean"], c["S"], c["Y"]) if psi else ()

    def handle(Xu, theta):
        dev = G.SGPDevice(len(X), c["M"], c["D"], c["d_out"], reuse_stats=True)
        dev.set_inducing(Xu)
        dev.set_data(X, Y)
        p = IR.softplus(theta)
        dev.set_kernel(float(p[0]), p[1:], c["jitter"], family=c["family"])
        dev.set_prior_isotropic(50.0)
        dev.set_noise(c["W"], float(np.linalg.slogdet(c["W"])[1]))
        return dev

    def objective(dev):
        return dev.theta_objective_psi(*gauss) if psi else dev.theta_objective()
    with handle(c["Xu"], c["theta0"]) as dev:
        dev.sweep()
        dev.sweep()
        assert dev.sweep_kind()[0] == CR.REUSED
        mu, _, Uv = dev.posterior()
        if inducing:
            call = functools.partial(dev.inducing_descend_psi, *gauss) if psi else dev.inducing_descend
            th, Z, vals, taken, _ = call(c["theta0"], c["Xu"], 3, **KW)
        else:
            call = functools.partial(dev.theta_descend_psi, *gauss) if psi else dev.theta_descend
            th, vals, taken, _ = call(c["theta0"], 3, **KW)
            Z = c["Xu"]
        assert taken == 3 and np.isfinite(vals).all()
        assert dev.sweep_kind()[0] == CR.MUTATORS[op].kind == CR.FULL
        v = objective(dev)
    with handle(Z, th) as fresh:
        fresh.set_posterior(mu, Uv)
        v0 = objective(fresh)
    print(f"{op}: next objective {v:.12e}, fresh handle {v0:.12e}, rel {abs(v / v0 - 1):.2e}")
    np.testing.assert_allclose(v, v0, rtol=RTOL)
    assert (np.abs(Z - c["Xu"]).max() > 1e-3) == inducing and np.abs(th - c["theta0"]).max() > 1e-3


def test_refusals(G):
    from gaussianprocessnode_amd._lib import ptr
    c = IR.case("a")
    th0, Z0 = c["theta0"], c["Xu"]

    def raw(dev, th=th0, Z=Z0, n_ell=None, flags=3, steps=3, eta=ETA, b1=0.9, b2=0.999, state=None):
        th = None if th is None else np.array(th, dtype=np.float64)
        Z = None if Z is None else np.array(Z, dtype=np.float64)
        rc = dev._lib.sgp_inducing_descend(dev._h, ptr(th), (len(th0) - 1) if n_ell is None else n_ell, ptr(Z), flags, steps, eta, b1, b2,
                                           1e-8, ptr(state), None, None)
        return rc, dev._lib.sgp_last_error(dev._h).decode(), th, Z
    with open_handle(G, c) as dev:
        for kw in (dict(Z=None), dict(th=None), dict(flags=1), dict(flags=0), dict(flags=7), dict(n_ell=3), dict(steps=-1),
                   dict(eta=0.0), dict(b1=1.0), dict(b2=-0.1), dict(Z=np.where(np.arange(Z0.size).reshape(Z0.shape) == 5, np.nan, Z0)),
                   dict(th=np.array([np.inf, 0.1])), dict(state=np.concatenate([np.zeros(2 * (2 + Z0.size)), [1.0, 0.5]]))):
            rc, msg, _, _ = raw(dev, **kw)
            assert rc == -1 and "sgp_inducing_descend" in msg, (kw, rc, msg)
        rc, _, th, Z = raw(dev, steps=0)
        assert rc == 0 and np.array_equal(th, th0) and np.array_equal(Z, Z0)
        v1 = dev.theta_objective()
        assert v1 == dev.theta_objective()                                  # steps = 0 changed nothing: still evaluable, same value
        dev.set_allreduce(lambda buf, count, stream: 0)
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "hook" in msg
    with G.SGPDevice(c["N"], c["M"], c["D"], 1) as dev:                     # no q(v), no data
        dev.set_inducing(Z0)
        dev.set_kernel(0.9, [0.7], 1e-8)
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "q(v)" in msg
    with G.SGPDevice(c["N"], c["M"], c["D"], 1) as dev:                     # q(v) installed, but no data
        dev.set_inducing(Z0)
        dev.set_kernel(0.9, [0.7], 1e-8)
        dev.set_noise(c["W"])
        dev.set_posterior(*qv(c))
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "data and kernel" in msg, msg
    with open_handle(G, c) as dev:                                          # the resident statistics are exact Psi-statistics
        S = np.tile(0.01 * np.eye(c["D"]), (c["N"], 1, 1))
        dev.sweep_local_psi(c["X"], S, c["Y"][:, 0])
        dev.sweep_finish()
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "exact Psi-statistics" in msg, msg
        rc, msg, _, _ = raw(dev, steps=0)
        assert rc == -1 and "exact Psi-statistics" in msg, msg              # steps = 0 sits behind every refusal
    with open_handle(G, c) as dev:                                          # an open training run
        dev.train_begin(c["X"], c["Y"][:, 0], th0)
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "training" in msg
        dev.train_end()


@pytest.mark.parametrize("learn_theta", [True, False])
def test_optimize_inducing_device_paced(G, learn_theta):
    c = IR.case("a")
    direct = runs("a", learn_theta)[0]
    opt = TR.AdaMax(**KW)
    with open_handle(G, c) as dev:
        th, Z, vals = TR.optimize_inducing(c["theta0"], c["Xu"], dev, q_v=qv(c), steps=STEPS, optimizer=opt, learn_theta=learn_theta,
                                           jitter=c["jitter"], device_paced=True)
        assert np.array_equal(th, direct[0]) and np.array_equal(Z, direct[1]) and np.array_equal(vals, direct[2])
        P = (th.size if learn_theta else 0) + Z.size
        assert np.array_equal(opt.get_named_state(TR.INDUCING_STATE, P), direct[4])
        # the engine ends AT the returned parameters, and the optimizer continues by name whatever arrays are passed
        th2, Z2, vals2 = TR.optimize_inducing(th.copy(), Z.copy(), dev, q_v=qv(c), steps=3, optimizer=opt, learn_theta=learn_theta,
                                              jitter=c["jitter"], device_paced=True)
    with open_handle(G, c) as dev:
        ref = dev.inducing_descend(c["theta0"], c["Xu"], STEPS + 3, learn_theta=learn_theta, **KW)
    np.testing.assert_allclose(Z2, ref[1], rtol=0, atol=1e-6 * np.abs(ref[1]).max())
    np.testing.assert_allclose(np.concatenate([vals, vals2]), ref[2], rtol=RTOL)
    assert np.array_equal(opt.get_named_state(TR.INDUCING_STATE, P)[-2:], ref[4][-2:])
