"""The reference of the predictive-derivative tests without a GPU (tests/predict_grad_ref.py): its three routes against each other
in units of the bound (the measurement C_BOUND rests on), its derivatives against central differences of its own mean, covariance
and joint covariance, the Matern-3/2 limit on an inducing input, the transposed cross block the dense case must reject, the
linearised rollout against a plain loop, and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import predict_grad_ref as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD_MARGIN = 4.0                       # C_BOUND leaves this factor above the worst float64 route's distance from longdouble
FD_CASES = ["dense", "coincident_se", "coincident_matern32", "coincident_matern52", "rollout_matern52"]


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_declares_the_call():
    from gaussianprocessnode_amd import _build, _lib
    from tests import call_sequence_ref as CR
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    api = open(os.path.join(ROOT, "gaussianprocessnode_amd", "csrc", "sgp_api.hip")).read()
    assert re.search(r"^int\s+sgp_predict_grad\s*\(sgp_handle\* h, const double\* Xstar", txt, re.M)
    assert re.search(r'extern "C" int sgp_predict_grad\(', api)
    assert "sgp_predict_grad" in _lib.EXPORTS and b"sgp_predict_grad" in open(_build.build(), "rb").read()
    assert CR.ENTRY_POINTS["sgp_predict_grad"] == CR.READER
    assert ":sgp_predict_grad" in open(os.path.join(ROOT, "julia", "SGPHip.jl")).read()
    lib = _lib.load()
    assert len(lib.sgp_predict_grad.argtypes) == 11
    assert lib.sgp_predict_grad(None, None, 1, None, None, 0, None, None, None, None, None) == -1      # SGP_ERR_ARG without a device


def test_the_binding_rejects_wrong_shapes_before_the_device():
    from gaussianprocessnode_amd.device import SGPDevice

    class Lib:
        calls = 0

        @staticmethod
        def sgp_predict_grad(*a):
            Lib.calls += 1
            return 0
    M, D, o = 5, 3, 2
    dev = object.__new__(SGPDevice)
    dev._lib, dev._h, dev.M, dev.D, dev.d_out, dev.Q = Lib, C.c_void_p(), M, D, o, M * o
    X, mu, Sig = np.zeros((4, D)), np.zeros(M * o), np.eye(M * o)
    for bad in (np.zeros((4, D + 1)), np.zeros(D), np.zeros((2, 2, D))):
        with pytest.raises(ValueError):
            dev.predict_grad(bad, mu, Sig)
    with pytest.raises(ValueError):
        dev.predict_grad(X, mu[:-1], Sig)
    with pytest.raises(ValueError):
        dev.predict_grad(X, mu, Sig[:-1, :-1])
    with pytest.raises(ValueError):
        dev.predict_grad(X, mu, None)
    assert Lib.calls == 0
    mean, jac, var, vg, jc = dev.predict_grad(X, mu, Sig, jac_cov=True)
    assert Lib.calls == 1
    assert mean.shape == (4, o) and jac.shape == (4, o, D) and var.shape == (4, o, o) and vg.shape == (4, o, o, D)
    assert jc.shape == (4, o * D, o * D)
    out = dev.predict_grad(X, mu, Sig, var=False, var_grad=False)
    assert out[2] is None and out[3] is None and out[4] is None
    dev.D, dev.d_out, dev.Q = 1, 1, M
    assert dev.predict_grad(np.zeros(7), np.zeros(M), np.eye(M))[1].shape == (7, 1, 1)


def test_the_grid_covers_the_issue_s_values():
    ks = [PG.CASES[n] for n in PG.GRID + PG.CORNERS]
    assert {k["family"] for k in ks} == set(PG.FAMILIES) and {k["iso"] for k in ks} == {False, True}
    assert {k["d_out"] for k in ks} == {1, 2, 4} and {k["D"] for k in ks} == set(PG.DIMS)
    assert {k["M"] for k in ks} == set(PG.SIZES) and {k["ns"] for k in ks} == set(PG.COUNTS)
    for fam in PG.FAMILIES:
        sub = [k for k in ks if k["family"] == fam]
        assert {(k["iso"], k["d_out"]) for k in sub} == {(i, o) for i in (False, True) for o in (1, 2, 4)}


# ---- the constant --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PG.SPREAD_CASES)
def test_the_float64_routes_against_longdouble(name):
    c = PG.get_case(name)
    one = PG.bounds(c, cst=1.0)
    exact = PG.evaluate(c, route="longdouble")
    worst = 0.0
    for route in ("inverse", "cholesky"):
        r = PG.ratios(exact, one, PG.evaluate(c, route=route))
        print(f"case {name}: route {route} against longdouble, error / (bound at C = 1) " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst = max(worst, max(r.values()))
    assert SPREAD_MARGIN * worst <= PG.C_BOUND, (name, worst)


# ---- the derivatives are derivatives ---------------------------------------------------------------------------------------------------
def _shift(X, d, h):
    Y = X.copy()
    Y[:, d] += h
    return Y


@pytest.mark.parametrize("name", FD_CASES)
def test_jac_and_var_grad_against_central_differences(name):
    c = PG.get_case(name)
    X = c["X"][2:] if name.startswith("coincident") else c["X"]          # (the Matern-3/2 third derivative jumps on an inducing input)
    ref, h = PG.evaluate(c, X), 1e-5
    for d in range(c["D"]):
        up, dn = PG.evaluate(c, _shift(X, d, h)), PG.evaluate(c, _shift(X, d, -h))
        fd_mean, fd_var = (up["mean"] - dn["mean"]) / (2 * h), (up["var"] - dn["var"]) / (2 * h)
        # central differences: h^2 / 6 f''' + eps |f| / h; both below 1e-6 of the output's scale at h = 1e-5
        for fd, an in ((fd_mean, ref["jac"][:, :, d]), (fd_var, ref["var_grad"][:, :, :, d])):
            assert np.max(np.abs(fd - an)) <= 1e-6 * max(1.0, np.max(np.abs(an))), (name, d)
    assert np.array_equal(ref["var_grad"], ref["var_grad"].transpose(0, 2, 1, 3)) or np.allclose(
        ref["var_grad"], ref["var_grad"].transpose(0, 2, 1, 3), rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", FD_CASES)
def test_jac_cov_against_the_mixed_second_difference_of_the_joint_covariance(name):
    c = PG.get_case(name)
    X = c["X"][2:] if name.startswith("coincident") else c["X"]
    D, o, h = c["D"], c["d_out"], 1e-4
    jc = PG.evaluate(c, X)["jac_cov"].reshape(len(X), o, D, o, D)
    scale = np.max(np.abs(jc))
    for d in range(D):
        for e in range(D):
            fd = (PG.joint_cov(c, _shift(X, d, h), _shift(X, e, h)) - PG.joint_cov(c, _shift(X, d, h), _shift(X, e, -h)) -
                  PG.joint_cov(c, _shift(X, d, -h), _shift(X, e, h)) + PG.joint_cov(c, _shift(X, d, -h), _shift(X, e, -h))) / (4 * h * h)
            # truncation O(h) for Matern-3/2 (|r|^3 in k(x, x')), O(h^2) otherwise; rounding eps |cov| / h^2 ~ 1e-8
            assert np.max(np.abs(fd - jc[:, :, d, :, e])) <= 2e-3 * scale, (name, d, e)
    full = PG.evaluate(c, X)["jac_cov"]
    assert np.allclose(full, full.transpose(0, 2, 1), rtol=0, atol=1e-13 * scale)


def test_the_matern32_limit_on_an_inducing_input():
    c = PG.get_case("coincident_matern32")
    on = PG.evaluate(c, c["X"][:1])
    k, J, s = PG.panel(c, c["X"][:1])
    assert s[0, 0] == 0.0 and np.all(J[0, 0] == 0.0) and k[0, 0] == c["sigma2"]
    assert all(np.isfinite(v).all() for v in on.values())
    # continuous through the kink of |r|^3: a point 1e-7 away agrees to the first derivative's Lipschitz constant times 1e-7
    near = PG.evaluate(c, c["X"][:1] + 1e-7 / np.sqrt(c["D"]))
    for key in ("jac", "var_grad", "jac_cov"):
        assert np.max(np.abs(on[key] - near[key])) <= 1e-5 * max(1.0, np.max(np.abs(on[key]))), key
    for fam in PG.FAMILIES:
        cf = PG.get_case(f"coincident_{fam}")
        assert PG.C_FAM[fam] == -2.0 * float(PG.g01(fam, np.float64(0.0))[1])
        assert PG.worst(0.0, PG.bounds(cf)["jac_cov"]) == 0.0 and np.isfinite(PG.bounds(cf)["jac_cov"]).all()


def test_a_transposed_cross_block_falls_outside_the_bound():
    c = PG.reference("dense")
    M = c["M"]
    cross = c["Sigma_v"][:M, M:]
    assert np.max(np.abs(cross - cross.T)) > 0.1 * np.max(np.abs(cross))
    bad = PG.evaluate(c, transpose_cross=True)
    D = c["D"]
    off = (slice(None), slice(0, D), slice(D, 2 * D))
    ratio = PG.worst(np.abs(bad["jac_cov"][off] - c["ref"]["jac_cov"][off]), c["tol"]["jac_cov"][off])
    print(f"case dense: the restatement with Sigma^(ij) transposed, off-diagonal jac_cov blocks, error / bound {ratio:.3g}")
    assert ratio > 1e3
    # ... and the (0, 1) block of jac_cov is then the transpose of the right one
    assert np.allclose(bad["jac_cov"][off], c["ref"]["jac_cov"][off].transpose(0, 2, 1), rtol=1e-12, atol=0)


# ---- the linearised rollout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rollout_se", "rollout_matern52"])
def test_the_linearised_rollout_against_a_plain_loop(name):
    from gaussianprocessnode_amd.train import linearize_step
    c = PG.get_case(name)
    m0, S0 = rollout_start(c)
    want_m, want_S = PG.linearize_rollout(c, m0, S0, 3, noise=True)
    m, S = m0.copy(), S0.copy()
    Winv = np.linalg.inv(c["W"])
    for k in range(3):
        r = PG.evaluate(c, m)
        var = r["var"] + Winv                                 # (the device's var is exactly symmetric; the restatement's to rounding)
        m, S = linearize_step(r["mean"], r["jac"], 0.5 * (var + var.transpose(0, 2, 1)), S)
        assert np.array_equal(S, S.transpose(0, 2, 1))
        assert np.allclose(m, want_m[k], rtol=1e-13, atol=1e-15) and np.allclose(S, want_S[k], rtol=1e-12, atol=1e-15)
    # S = 0: one step returns the predictive mean and covariance themselves
    r = PG.evaluate(c, m0)
    m1, S1 = linearize_step(r["mean"], r["jac"], r["var"], np.zeros_like(S0))
    assert np.array_equal(m1, r["mean"]) and np.array_equal(S1, r["var"])


def rollout_start(c):
    """two Gaussians about the case's two points"""
    rng = np.random.default_rng(77)
    D = c["D"]
    L = 0.1 * rng.normal(size=(2, D, D))
    return np.array(c["X"], dtype=np.float64), L @ L.transpose(0, 2, 1) + 0.01 * np.eye(D)
