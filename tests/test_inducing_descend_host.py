"""The inducing-input descent without a GPU: the NumPy loop (tests/inducing_descend_ref.py) against `train.optimize_inducing`'s host
loop driven by a test double that serves the restatement's gradients; that every shape moves; the sign-flip condition at step 0; the
injected faults against the GPU tests' bounds; `optimize_inducing(device_paced=True)` over a test double; and the entry points'
boundary (declared, exported, bound)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaussianprocessnode_amd import train as TR
from tests import inducing_descend_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RestatementEngine:
    """What `optimize_inducing` drives, on the restatement (host-paced), and `inducing_descend[_psi]` as the NumPy loop
    (device-paced), recording the calls."""

    def __init__(self, c):
        self.c, self.calls, self.qv = c, [], None

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.p = np.concatenate([[sigma2], np.asarray(ell, dtype=np.float64)])
        self.calls.append("kernel")

    def set_inducing(self, Xu):
        self.Xu, self.qv = np.array(Xu, dtype=np.float64), None
        self.calls.append("inducing")

    def set_posterior(self, mu_v, Uv):
        self.qv = (mu_v, Uv)
        self.calls.append("posterior")

    def theta_objective_xu(self, want_grad=False):
        assert self.qv is not None
        self.calls.append("objective")
        return IR.value_and_grads(self.c, self.p, self.Xu)

    def theta_objective_psi_xu(self, mean, cov, y_mean, want_grad=False):
        return self.theta_objective_xu()

    def inducing_descend(self, theta, Xu, steps, *, learn_theta=True, eta, beta, eps, state):
        assert self.qv is not None and (eta, tuple(beta), eps) == (IR.ETA, IR.BETA, IR.EPS)
        self.calls.append("descend")
        nt = len(theta) if learn_theta else 0
        th, Z, vals, st = IR.loop(self.c, steps, learn_theta, state=state, x0=np.concatenate([np.ravel(theta)[:nt], np.ravel(Xu)]))
        return th, Z, vals, steps, st

    def inducing_descend_psi(self, mean, cov, y_mean, theta, Xu, steps, **kw):
        return self.inducing_descend(theta, Xu, steps, **kw)


def drive(c, learn_theta, **kw):
    eng = RestatementEngine(c)
    opt = TR.AdaMax(eta=IR.ETA, beta=IR.BETA, eps=IR.EPS)
    extra = dict(psi="exact", inputs=(c["mean"], c["S"], c["Y"])) if c["psi"] else {}
    out = TR.optimize_inducing(c["theta0"], c["Xu"], eng, q_v=(c["mu"], np.linalg.cholesky(c["Rv"]).T), steps=IR.STEPS, optimizer=opt,
                               learn_theta=learn_theta, jitter=c["jitter"], **extra, **kw)
    return out, eng, opt


@pytest.mark.parametrize("learn_theta", [True, False])
@pytest.mark.parametrize("name", sorted(IR.SHAPES))
def test_the_numpy_loop_is_optimize_inducing(name, learn_theta):
    c = IR.case(name)
    (th, Z, vals), eng, _ = drive(c, learn_theta)
    th_r, Z_r, vals_r, _ = IR.reference(name, learn_theta)
    assert eng.calls.count("objective") == IR.STEPS
    np.testing.assert_allclose(th, th_r, rtol=1e-13)
    np.testing.assert_allclose(Z, Z_r, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(vals, vals_r, rtol=1e-13)


@pytest.mark.parametrize("name", sorted(IR.SHAPES))
def test_every_shape_moves_and_meets_the_sign_flip_condition(name):
    c = IR.case(name)
    assert c["cond"] < 1e6, c["cond"]
    margin = IR.sign_margin(c)
    th, Z, vals, _ = IR.reference(name)
    spread = c["Xu"].max() - c["Xu"].min()
    moved_xu = np.abs(Z - c["Xu"]).max() / spread
    moved_th = np.abs(th - c["theta0"]).max()
    print(f"{name}: cond(K_uu) {c['cond']:.2e}; min|g_i(0)| / max|grad| {margin:.2e}; Xu moved {moved_xu:.2e} of its spread, "
          f"theta {moved_th:.2e}; f {vals[0]:.6g} -> {vals[-1]:.6g}")
    assert margin >= IR.SIGN_MARGIN
    assert moved_xu > 1e-3 and moved_th > 1e-3
    if name == "b":
        assert c["nranges"] >= 2 and c["range_len"] >= 2


@pytest.mark.parametrize("fault,name", [(f, n) for f, names in IR.FAULTS.items() for n in names])
def test_injected_faults_miss_the_bounds_tenfold(fault, name):
    """The GPU tests' bounds -- theta and values to RTOL, Xu to XU_ATOL -- against a loop with one mistake: at least one of them is
    missed by 10 x or more."""
    c = IR.case(name)
    th_r, Z_r, vals_r, _ = IR.reference(name)
    th, Z, vals, _ = IR.loop(c, fault=fault)
    miss = max(np.abs(th / th_r - 1).max() / IR.RTOL, np.abs(vals / vals_r - 1).max() / IR.RTOL, np.abs(Z - Z_r).max() / IR.XU_ATOL)
    print(f"{fault} {name}: worst error / bound {miss:.3g}")
    assert miss >= 10.0


@pytest.mark.parametrize("name", ["a", "e"])
@pytest.mark.parametrize("learn_theta", [True, False])
def test_device_paced_driver_installs_once_and_carries_the_state(name, learn_theta):
    c = IR.case(name)
    (th, Z, vals), eng, opt = drive(c, learn_theta, device_paced=True)
    assert eng.calls == ["kernel", "inducing", "posterior", "descend"]
    th_r, Z_r, vals_r, state_r = IR.reference(name, learn_theta)
    assert np.array_equal(th, th_r) and np.array_equal(Z, Z_r) and np.array_equal(vals, vals_r)
    P = (th.size if learn_theta else 0) + Z.size
    assert np.array_equal(opt.get_named_state(TR.INDUCING_STATE, P), state_r)
    # the optimizer carries the joint state by name: copies of the returned arrays continue it; 15 + 5 steps are 20
    extra = dict(psi="exact", inputs=(c["mean"], c["S"], c["Y"])) if c["psi"] else {}
    th2, Z2, _ = TR.optimize_inducing(th.copy(), Z.copy(), eng, q_v=(c["mu"], np.linalg.cholesky(c["Rv"]).T), steps=5, optimizer=opt,
                                      learn_theta=learn_theta, jitter=c["jitter"], device_paced=True, **extra)
    th20, Z20, _, state20 = IR.loop(c, IR.STEPS + 5, learn_theta)
    assert np.array_equal(Z2, Z20) and np.array_equal(th2, th20) and np.array_equal(opt.get_named_state(TR.INDUCING_STATE, P), state20)
    # host-paced updates of a joint array continue it through set_state, and hand it back through set_named_state
    x = np.concatenate([th2 if learn_theta else [], Z2.ravel()])
    opt.set_state(x, opt.get_named_state(TR.INDUCING_STATE, P))
    _, g = IR.joint_gradient(c, x, learn_theta)
    opt.update(x, g)
    th21, Z21, _, state21 = IR.loop(c, IR.STEPS + 6, learn_theta)
    np.testing.assert_allclose(x[x.size - Z21.size:].reshape(Z21.shape), Z21, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(opt.get_state(x), state21, rtol=1e-13, atol=1e-300)
    with pytest.raises(ValueError):                                         # a kept state of another size is never taken silently
        opt.get_named_state(TR.INDUCING_STATE, P + 1)


def test_the_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import SGPDevice, _build, _lib
    blob = open(_build.build(), "rb").read()
    for name, nargs in (("sgp_inducing_descend", 13), ("sgp_inducing_descend_psi", 17)):
        assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int
    assert (_lib.SGP_DESCEND_THETA, _lib.SGP_DESCEND_XU) == (1, 2) and "SGP_DESCEND_THETA = 1, SGP_DESCEND_XU = 2" in txt
    for kernel in (b"k_inducing_step", b"k_inducing_step_psi", b"k_inducing_step_xu"):
        assert kernel in blob, kernel
    jl = open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    assert "sgp_inducing_descend" in jl and "sgp_inducing_descend_psi" in jl
    assert callable(SGPDevice.inducing_descend) and callable(SGPDevice.inducing_descend_psi)
