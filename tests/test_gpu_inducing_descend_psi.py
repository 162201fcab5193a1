"""sgp_inducing_descend_psi on the device: tests/test_gpu_inducing_descend.py for the objective over the exact Psi-statistics of
Gaussian inputs -- the host-paced `train.optimize_inducing(psi="exact")` on the same handle, the NumPy loop, the first value,
repeatability, continuation, a different SGP_PREDICT_CHUNK in a fresh child process, learn_theta=False, both stops, the state the
call leaves, the refusals and the driver.  Shapes: tests/inducing_descend_ref.py, PSI_SHAPES; bounds as in the point file."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gaussianprocessnode_amd import train as TR
from tests import inducing_descend_ref as IR
from tests import test_gpu_psi_theta as PT

pytestmark = pytest.mark.gpu

RTOL, STEPS, ETA = IR.RTOL, IR.STEPS, IR.ETA
KW = dict(eta=ETA, beta=IR.BETA, eps=IR.EPS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def qv(c):
    return c["mu"], np.linalg.cholesky(c["Rv"]).T


def inputs(c):
    return c["mean"], c["S"], c["Y"]


def open_handle(G, c, *, jitter=None, Xu=None, theta=None):
    dev = G.SGPDevice(max(8, c["T"]), c["M"], c["D"], d_out=c["d_out"])
    dev.set_inducing(c["Xu"] if Xu is None else Xu)
    p = IR.softplus(c["theta0"] if theta is None else theta)
    dev.set_kernel(float(p[0]), p[1:], c["jitter"] if jitter is None else jitter)
    dev.set_noise(c["W"])
    dev.set_posterior(*qv(c))
    return dev


@functools.lru_cache(maxsize=None)
def runs(name, learn_theta=True):
    import gaussianprocessnode_amd as G
    c = IR.case(name)
    with open_handle(G, c) as dev:
        got = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], STEPS, learn_theta=learn_theta, **KW)
        host = TR.optimize_inducing(c["theta0"], c["Xu"], dev, q_v=qv(c), steps=STEPS, optimizer=TR.AdaMax(**KW),
                                    learn_theta=learn_theta, jitter=c["jitter"], psi="exact", inputs=inputs(c))
    return got, host


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(IR.PSI_SHAPES))
def test_matches_the_host_paced_loop_and_the_numpy_loop(G, name):
    c = IR.case(name)
    (th, Z, vals, taken, state), (th_h, Z_h, vals_h) = runs(name)
    th_r, Z_r, vals_r, state_r = IR.reference(name)
    assert taken == STEPS and Z.shape == (c["M"], c["D"]) and state.size == 2 * (th.size + Z.size) + 2
    e_host = (np.abs(th / th_h - 1).max(), np.abs(vals / vals_h - 1).max(), np.abs(Z - Z_h).max() / np.abs(Z_h).max())
    e_ref = (np.abs(th / th_r - 1).max(), np.abs(vals / vals_r - 1).max(), np.abs(Z - Z_r).max())
    print(f"inducing_descend_psi {name}: vs host-paced theta {e_host[0]:.2e} values {e_host[1]:.2e} Xu/max|Xu| {e_host[2]:.2e}; "
          f"vs NumPy theta {e_ref[0]:.2e} values {e_ref[1]:.2e} Xu abs {e_ref[2]:.2e} (bound {IR.XU_ATOL:.1e})")
    np.testing.assert_allclose(th, th_h, rtol=RTOL)
    np.testing.assert_allclose(vals, vals_h, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_h, rtol=0, atol=1e-6 * np.abs(Z_h).max())
    np.testing.assert_allclose(th, th_r, rtol=RTOL)
    np.testing.assert_allclose(vals, vals_r, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_r, rtol=0, atol=IR.XU_ATOL)


@pytest.mark.parametrize("name", ["e", "g"])
def test_first_value_is_theta_objective_psi_xu_at_the_same_state(G, name):
    c = IR.case(name)
    with open_handle(G, c) as dev:
        _, _, vals, _, _ = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], 1, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"])
        dev.set_posterior(*qv(c))
        v, _, _ = dev.theta_objective_psi_xu(*inputs(c), want_grad=True)
    assert vals[0] == v and vals[0] == runs(name)[0][2][0] == runs(name, False)[0][2][0]


CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import gaussianprocessnode_amd as G
from tests import inducing_descend_ref as IR
from tests import test_gpu_inducing_descend_psi as T
c = IR.case({name!r})
with T.open_handle(G, c) as dev:
    th, Z, vals, taken, state = dev.inducing_descend_psi(*T.inputs(c), c["theta0"], c["Xu"], T.STEPS, **T.KW)
print(json.dumps([a.tobytes().hex() for a in (th, Z, vals, state)]))
"""


def test_repeatable_continued_and_independent_of_the_chunk(G):
    name = "f"
    c = IR.case(name)
    one = runs(name)[0]
    k = 6
    with open_handle(G, c) as dev:
        again = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], STEPS, **KW)
        th1, Z1, v1, n1, s1 = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], k, **KW)
        th2, Z2, v2, n2, s2 = dev.inducing_descend_psi(*inputs(c), th1, Z1, STEPS - k, state=s1, **KW)
    assert same(one, again)
    assert same(one, (th2, Z2, np.concatenate([v1, v2]), n1 + n2, s2))
    env = dict(os.environ, SGP_PREDICT_CHUNK="64")
    out = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, name=name)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for h, a in zip(got, (one[0], one[1], one[2], one[4])):
        assert bytes.fromhex(h) == a.tobytes()
    # a state from train.AdaMax continues to RTOL
    opt = TR.AdaMax(**KW)
    with open_handle(G, c) as dev:
        thk, Zk, _ = TR.optimize_inducing(c["theta0"], c["Xu"], dev, q_v=qv(c), steps=k, optimizer=opt, jitter=c["jitter"], psi="exact",
                                          inputs=inputs(c), device_paced=True)
        nt = thk.size
        x = np.concatenate([thk, Zk.ravel()])
        opt.set_state(x, opt.get_named_state(TR.INDUCING_STATE, x.size))
        for _ in range(2):                                                  # two host-paced updates of the same joint vector
            p = IR.softplus(x[:nt])
            dev.set_kernel(float(p[0]), p[1:], c["jitter"])
            dev.set_inducing(x[nt:].reshape(c["M"], c["D"]))
            dev.set_posterior(*qv(c))
            _, g, gx = dev.theta_objective_psi_xu(*inputs(c), want_grad=True)
            opt.update(x, np.concatenate([g * TR.sigmoid(x[:nt]), gx.ravel()]))
        th3, Z3, _, _, _ = dev.inducing_descend_psi(*inputs(c), x[:nt], x[nt:].reshape(c["M"], c["D"]), STEPS - k - 2,
                                                    state=opt.get_state(x), **KW)
    np.testing.assert_allclose(th3, one[0], rtol=RTOL)
    np.testing.assert_allclose(Z3, one[1], rtol=0, atol=1e-6 * np.abs(one[1]).max())


def test_learn_theta_false_moves_xu_alone(G):
    name = "e"
    c = IR.case(name)
    (th, Z, vals, taken, state), (th_h, Z_h, vals_h) = runs(name, False)
    assert np.array_equal(th, c["theta0"]) and taken == STEPS and state.size == 2 * Z.size + 2
    assert np.abs(Z - c["Xu"]).max() > 1e-3 * (c["Xu"].max() - c["Xu"].min())
    np.testing.assert_allclose(vals, vals_h, rtol=RTOL)
    np.testing.assert_allclose(Z, Z_h, rtol=0, atol=1e-6 * np.abs(Z_h).max())
    np.testing.assert_allclose(Z, IR.reference(name, False)[1], rtol=0, atol=IR.XU_ATOL)
    with open_handle(G, c) as dev:
        dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], 2, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"]); dev.set_posterior(*qv(c))
        v1, g1 = dev.theta_objective_psi(*inputs(c), want_grad=True)
        dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], 3, learn_theta=False, **KW)
        dev.set_inducing(c["Xu"]); dev.set_posterior(*qv(c))
        v2, g2 = dev.theta_objective_psi(*inputs(c), want_grad=True)
    assert v1 == v2 and np.array_equal(g1, g2)


def test_stops(G):
    """K_uu: identical inducing rows, jitter 0, sigma2 = softplus(64) = 64 exactly (second pivot 64 - 64 * 64 / 64 = 0).  A node: an
    indefinite covariance."""
    c = IR.case("e")
    Xu = c["Xu"].copy()
    Xu[1:4] = Xu[0]
    th0 = c["theta0"].copy()
    th0[0] = 64.0
    zero_state = np.concatenate([np.zeros(2 * (th0.size + Xu.size)), IR.BETA])
    with open_handle(G, c, jitter=0.0, Xu=Xu, theta=th0) as dev:
        with pytest.raises(np.linalg.LinAlgError) as ei:
            dev.inducing_descend_psi(*inputs(c), th0, Xu, 4, **KW)
        e = ei.value
        assert e.minor > 0 and e.node == 0 and e.steps_taken == 0 and np.isnan(e.values).all()
        assert np.array_equal(e.theta, th0) and np.array_equal(e.Xu, Xu) and np.array_equal(e.state, zero_state)
    S = c["S"].copy()
    S[5] = -np.eye(c["D"])
    with open_handle(G, c) as dev:
        with pytest.raises(G.PosDefException) as ei:
            dev.inducing_descend_psi(c["mean"], S, c["Y"], c["theta0"], c["Xu"], 4, **KW)
        e = ei.value
        assert e.info == 6 and e.node == 6 and e.minor == 0 and e.steps_taken == 0 and np.isnan(e.values).all()
        assert np.array_equal(e.theta, c["theta0"]) and np.array_equal(e.Xu, c["Xu"])
        assert np.array_equal(e.state, np.concatenate([np.zeros(2 * (c["theta0"].size + c["Xu"].size)), IR.BETA]))


def test_state_afterwards(G):
    """After an exact sweep: the call writes none of the resident statistics and leaves q(v) and sweep_kind as they were (FULL: the
    inducing inputs moved, the next sweep forms everything again); predict uses Xu_out."""
    c = IR.case("e")
    with open_handle(G, c) as dev:
        dev.set_prior_isotropic(50.0)
        dev.sweep_local_psi(*inputs(c))
        dev.sweep_finish()
        mu, Sig, Uv = dev.posterior()
        before = (dev.sweep_kind(), dev.stats(), (mu, Sig, Uv))
        th, Z, vals, _, _ = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], STEPS, **KW)
        after = (dev.sweep_kind(), dev.stats(), dev.posterior())
        assert before[0] == after[0] and after[0][0] == 0
        for a, b in zip(before[1] + before[2], after[1] + after[2]):
            assert np.array_equal(a, b)
        v, g, gx = dev.theta_objective_psi_xu(*inputs(c), want_grad=True)   # no set_posterior: q(v) is still the sweep's
        pred = dev.predict(c["mean"][:20])
    with open_handle(G, c, Xu=Z, theta=th) as fresh:
        fresh.set_posterior(mu, Uv)
        v0, g0, gx0 = fresh.theta_objective_psi_xu(*inputs(c), want_grad=True)
        pred0 = fresh.predict(c["mean"][:20], mu_v=mu)
    np.testing.assert_allclose(v, v0, rtol=RTOL)
    np.testing.assert_allclose(g, g0, rtol=RTOL, atol=1e-9 * np.abs(g0).max())
    np.testing.assert_allclose(gx, gx0, rtol=RTOL, atol=1e-9 * np.abs(gx0).max())
    np.testing.assert_allclose(pred, pred0, rtol=RTOL, atol=1e-9 * np.abs(pred0).max())


def test_resident_reusable_statistics_are_withdrawn(G):
    """A handle with resident data whose next sweep would reuse its statistics: after the call the inducing inputs have moved, so the
    next sweep is FULL -- and it gives what a fresh handle at (theta_out, Xu_out) gives."""
    c = IR.case("e")
    X, y = c["mean"], c["Y"]

    def handle(Xu, theta):
        dev = G.SGPDevice(c["T"], c["M"], c["D"], d_out=c["d_out"], reuse_stats=True)
        dev.set_inducing(Xu)
        dev.set_data(X, y)
        p = IR.softplus(theta)
        dev.set_kernel(float(p[0]), p[1:], c["jitter"])
        dev.set_prior_isotropic(50.0)
        dev.set_noise(c["W"], float(np.linalg.slogdet(c["W"])[1]))
        return dev
    with handle(c["Xu"], c["theta0"]) as dev:
        dev.sweep()
        dev.sweep()
        assert dev.sweep_kind()[0] != 0                                     # the next sweep would reuse the statistics
        # learn_theta=False: the kernel VALUES may not move at all, so nothing but the call's own bookkeeping withdraws the statistics
        th, Z, _, _, _ = dev.inducing_descend_psi(*inputs(c), c["theta0"], c["Xu"], 3, learn_theta=False, **KW)
        p = IR.softplus(c["theta0"])
        dev.set_kernel(float(p[0]), p[1:], c["jitter"])                     # the values of the statistics' record again
        assert dev.sweep_kind()[0] == 0                                     # SGP_SWEEP_FULL
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
    with handle(Z, c["theta0"]) as fresh:
        fresh.sweep()
        mu0, Sig0, _ = fresh.posterior(want_uv=False)
    np.testing.assert_allclose(mu, mu0, rtol=RTOL, atol=1e-9 * np.abs(mu0).max())
    np.testing.assert_allclose(Sig, Sig0, rtol=RTOL, atol=1e-9 * np.abs(Sig0).max())


def test_refusals(G):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = IR.case("e")
    th0, Z0 = c["theta0"], c["Xu"]
    m, S, y = as_f64(c["mean"]), as_f64(c["S"]), as_f64(c["Y"].T)

    def raw(dev, th=th0, Z=Z0, n_ell=None, flags=3, steps=3, eta=ETA, b1=0.9, b2=0.999, state=None, mean=m, cov=S, T=None):
        th = None if th is None else np.array(th, dtype=np.float64)
        Z = None if Z is None else np.array(Z, dtype=np.float64)
        rc = dev._lib.sgp_inducing_descend_psi(dev._h, ptr(mean), ptr(cov), ptr(y), c["T"] if T is None else T, ptr(th),
                                               (len(th0) - 1) if n_ell is None else n_ell, ptr(Z), flags, steps, eta, b1, b2, 1e-8,
                                               ptr(state), None, None)
        return rc, dev._lib.sgp_last_error(dev._h).decode(), th, Z
    bad_mean = m.copy()
    bad_mean[3, 0] = np.nan
    with open_handle(G, c) as dev:
        for kw in (dict(Z=None), dict(th=None), dict(flags=1), dict(flags=0), dict(flags=8 | 2), dict(n_ell=3), dict(n_ell=0),
                   dict(steps=-1), dict(eta=-1.0), dict(b1=1.0), dict(b2=1.5), dict(Z=np.full_like(Z0, np.inf)),
                   dict(th=np.full_like(th0, np.nan)), dict(state=np.concatenate([np.zeros(2 * (th0.size + Z0.size)), [0.9, 0.0]])),
                   dict(mean=None), dict(mean=bad_mean), dict(T=0)):
            rc, msg, _, _ = raw(dev, **kw)
            assert rc == -1 and "sgp_inducing_descend_psi" in msg, (kw, rc, msg)
        rc, _, th, Z = raw(dev, steps=0)
        assert rc == 0 and np.array_equal(th, th0) and np.array_equal(Z, Z0)
        rc, msg, _, _ = raw(dev, steps=0, mean=None)
        assert rc == -1 and "sgp_inducing_descend_psi" in msg               # steps = 0 sits behind every refusal
        dev.set_allreduce(lambda buf, count, stream: 0)
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "hook" in msg
    with G.SGPDevice(max(8, c["T"]), c["M"], c["D"], d_out=c["d_out"]) as dev:          # no q(v)
        dev.set_inducing(Z0)
        dev.set_kernel(0.9, IR.softplus(th0[1:]), 1e-8)
        dev.set_noise(c["W"])
        rc, msg, _, _ = raw(dev)
        assert rc == -1 and "q(v)" in msg
    with open_handle(G, c) as dev:                                          # another family
        dev.set_kernel_family("matern32")
        rc, msg, _, _ = raw(dev)
        assert rc == -1


@pytest.mark.parametrize("learn_theta", [True, False])
def test_optimize_inducing_device_paced(G, learn_theta):
    c = IR.case("g")
    direct = runs("g", learn_theta)[0]
    opt = TR.AdaMax(**KW)
    with open_handle(G, c) as dev:
        th, Z, vals = TR.optimize_inducing(c["theta0"], c["Xu"], dev, q_v=qv(c), steps=STEPS, optimizer=opt, learn_theta=learn_theta,
                                           jitter=c["jitter"], psi="exact", inputs=inputs(c), device_paced=True)
    assert np.array_equal(th, direct[0]) and np.array_equal(Z, direct[1]) and np.array_equal(vals, direct[2])
    assert np.array_equal(opt.get_named_state(TR.INDUCING_STATE, (th.size if learn_theta else 0) + Z.size), direct[4])
