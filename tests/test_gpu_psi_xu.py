"""sgp_theta_objective_psi_xu on the device: grad_xu against the NumPy restatement (tests/psi_xu_ref.py) at the smallest shapes at
which each part of k_psi_xu_prep / k_psi1_xu_accumulate / k_psi2_xu_accumulate / k_psi_xu_finish can go wrong -- see CASES -- value
and theta gradient bitwise against sgp_theta_objective_psi, determinism, the point route as an independent device cross-check, the
state the call leaves, its refusals and `train.optimize_inducing(psi="exact")`.

Bounds: the project's for the same objective -- value and theta gradient bitwise equal to theta_objective_psi(want_grad=True) on the
same handle (tests/test_gpu_xu_grad.py), grad_xu rtol 1e-6 with atol 1e-9 max|grad| against the restatement
(tests/test_gpu_psi_theta.py).  The inputs are tests/test_gpu_psi_theta.problem's, with its SCALES: cond(K_uu) stays below 1e5.  The
measured errors are printed and recorded in profiles/psi_xu.txt.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import psi_theta_ref as TR
from tests import psi_xu_ref as XR
from tests import test_gpu_psi_theta as PT
from tests.xu_grad_ref import analytic_grad_xu as point_grad_xu

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9
SIGMA2 = PT.SIGMA2

# name: what it exercises.  The specs are tests/test_gpu_psi_theta.CASES' where the name is there, (d_out, M, D, T, shared, cov, jitter).
SHARED = ["smallest_M",             # (1, 1, 2, 65): only the diagonal entry, the (z - z') and K_uu terms vanish
          "single_node",            # (2, 48, 2, 1)
          "one_tile_T63",           # (2, 48, 2, 63): one diagonal tile, one range
          "one_tile_T65",           # (2, 48, 2, 65): the first shape with a second 8-node range
          "one_tile_T300",          # (2, 48, 2, 300): 38 ranges
          "padded_second_tile",     # (1, 65, 1, 63), shared ell: the first off-diagonal tile, which feeds rows of two tile rows; D = 1
          "six_tiles",              # (2, 130, 2, 65): a row sums three tiles plus column parts from later tile rows
          "shared_ell_D5",          # (4, 65, 5, 65), shared ell, d_out = 4
          "D32",                    # (1, 65, 32, 63)
          "cov_null", "cov_zero", "cov_rank1"]      # (3, 65, 5, 65)
OWN = {"D8": (3, 65, 8, 65, False, "full", 1e-8),  # both sides of the DCAP 8 / 32 switch
       "D9": (3, 65, 9, 65, False, "full", 1e-8)}
CASES = SHARED + sorted(OWN)


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs (tests/test_gpu_psi_theta's, shared with it where the case is its own) and the restatement's grad_xu, once."""
    c = dict(PT.case(name) if name in PT.CASES else PT.problem(name, OWN[name], 700 + sorted(OWN).index(name)))
    cond = np.linalg.cond(TR._common(SIGMA2, c["ell"], c["Xu"], c["Rv"], c["mu"], c["W"], c["jitter"])[5] + c["jitter"] * np.eye(c["M"]))
    assert cond < 1e5, f"the test's inputs leave K_uu ill-conditioned ({cond:.1e}): it would compare rounding"
    c["gxu"] = XR.analytic_grad_xu(SIGMA2, c["ell"], c["mean"], c["S"], c["Y"], c["Rv"], c["mu"], c["W"], c["Xu"], c["jitter"])
    return c


def error(g, ref):
    return float(np.max(np.abs(g - ref) / (RTOL * np.abs(ref) + ATOL * np.max(np.abs(ref)))))


def assert_close(label, g, ref):
    e = error(g, ref)
    print(f"theta_objective_psi_xu {label}: grad_xu error / bound {e:.3g}; max |err| / max|grad| "
          f"{float(np.max(np.abs(g - ref)) / np.max(np.abs(ref))):.3g}")
    assert g.shape == ref.shape
    assert e <= 1.0, (g, ref)


@pytest.mark.parametrize("name", CASES)
def test_grad_xu_matches_the_restatement_and_the_rest_is_bitwise(G, name):
    c = case(name)
    with PT.device(G, c) as dev:
        f0, g0 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        f, g, gxu = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"], want_grad=True)
        f2, g2, gxu2 = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"], want_grad=True)
        f3, gxu3 = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"])
    assert f == f0 and np.array_equal(g, g0)                      # value and theta gradient: the objective's own, bitwise
    assert f2 == f and f3 == f and np.array_equal(g2, g)
    assert np.array_equal(gxu2, gxu) and np.array_equal(gxu3, gxu)   # a second identical call agrees bitwise
    assert gxu.shape == (c["M"], c["D"])
    assert_close(name, gxu, c["gxu"])


@pytest.mark.parametrize("name", ["one_tile_T65", "one_tile_T300", "six_tiles"])
def test_the_chunk_size_changes_no_bit(G, name, monkeypatch):
    c = case(name)
    with PT.device(G, c) as dev:
        f, g, gxu = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"], want_grad=True)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")
    with PT.device(G, c) as dev:
        f64, g64, gxu64 = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"], want_grad=True)
    assert f == f64 and np.array_equal(g, g64) and np.array_equal(gxu, gxu64)


def test_null_covariance_matches_the_point_route_on_the_means(G):
    """Two independent device routes: closed-form statistics at S = 0 against K_uf of the means as resident data."""
    c = case("cov_null")
    with PT.device(G, c) as dev:
        f, gxu = dev.theta_objective_psi_xu(c["mean"], None, c["Y"])
    with PT.device(G, c, posterior=False) as dev:
        dev.set_data(c["mean"], c["Y"])
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)
        f0, gxu0 = dev.theta_objective_xu()
    assert abs(f - f0) <= PT.VALUE_RTOL * abs(f0)
    assert_close("cov=NULL against sgp_theta_objective_xu on the means", gxu, gxu0)
    ref = point_grad_xu(SIGMA2, c["ell"], c["mean"], np.ones(c["T"]), c["Y"], c["Rv"], c["mu"], c["W"], c["Xu"], c["jitter"], "se")
    assert_close("cov=NULL against the point restatement", gxu, ref)


def test_works_after_an_exact_sweep_and_changes_nothing_the_sweep_keeps(G):
    c = case("one_tile_T65")
    with PT.device(G, c, posterior=False) as dev:
        dev.set_prior_isotropic(50.0)
        dev.sweep_local_psi(c["mean"], c["S"], c["Y"])
        dev.sweep_finish()
        mu, Sig, Uv = dev.posterior()
        before = (dev.sweep_kind(), dev.stats(), (mu, Sig, Uv))
        f, g, gxu = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"], want_grad=True)
        after = (dev.sweep_kind(), dev.stats(), dev.posterior())
        assert before[0] == after[0]
        for a, b in zip(before[1] + before[2], after[1] + after[2]):
            assert np.array_equal(a, b)
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective()
        assert "exact Psi-statistics" in str(ei.value)
        Rv = Sig + np.outer(mu, mu)
        ref = XR.analytic_grad_xu(SIGMA2, c["ell"], c["mean"], c["S"], c["Y"], Rv, mu, c["W"], c["Xu"], c["jitter"])
        assert_close("after sweep_local_psi + sweep_finish", gxu, ref)


def raw_call(dev, c, S, grad_xu, n_nodes=None):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    v, info = C.c_double(), (C.c_int64 * 2)()
    m, Sb, y = as_f64(c["mean"]), None if S is None else as_f64(S), as_f64(c["Y"].T)
    rc = dev._lib.sgp_theta_objective_psi_xu(dev._h, ptr(m), ptr(Sb), ptr(y), c["T"] if n_nodes is None else n_nodes,
                                             C.cast(C.byref(v), C.POINTER(C.c_double)), None, ptr(grad_xu), info)
    return rc, list(info), dev._lib.sgp_last_error(dev._h).decode()


def test_refusals(G):
    c = case("one_tile_T63")
    mean, S, Y = c["mean"], c["S"], c["Y"]

    def refused(dev, text, *args):
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective_psi_xu(*(args or (mean, S, Y)))
        assert "status -1" in str(ei.value) and text in str(ei.value), str(ei.value)
        assert "sgp_theta_objective_psi_xu: " in str(ei.value), str(ei.value)

    with G.SGPDevice(64, c["M"], c["D"], d_out=c["d_out"]) as dev:
        PT.install(dev, c, posterior=False)
        refused(dev, "q(v)")
        PT.install(dev, c)
        rc, _, msg = raw_call(dev, c, S, None)
        assert rc == -1 and msg.startswith("sgp_theta_objective_psi_xu: ") and "grad_xu" in msg, (rc, msg)
        nan_mean, inf_cov, nan_y = mean.copy(), S.copy(), Y.copy()
        nan_mean[3, 0], inf_cov[2, 0, 0], nan_y[5, 1] = np.nan, np.inf, np.nan
        refused(dev, "mean must be finite", nan_mean, S, Y)
        refused(dev, "cov must be finite", mean, inf_cov, Y)
        refused(dev, "y_mean must be finite", mean, S, nan_y)
        refused(dev, "n_nodes must be >= 1", mean[:0], S[:0], Y[:0])
        dev.set_kernel_family("matern32")
        refused(dev, "SGP_KERNEL_SE only")
        dev.set_kernel_family("se")
        dev.set_allreduce(lambda buf, count, stream: 0)
        refused(dev, "all-reduce hook")
        dev.set_allreduce(None)
        _, gxu = dev.theta_objective_psi_xu(mean, S, Y)
        assert_close("after the refusals", gxu, c["gxu"])
    c1 = case("padded_second_tile")
    with PT.device(G, c1) as dev:
        dev.train_begin(c1["mean"], c1["Y"][:, 0], np.zeros(2))
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective_psi_xu(c1["mean"], c1["S"], c1["Y"])
        assert "status -1" in str(ei.value) and "a device-paced training run is open" in str(ei.value)
        dev.train_end()


def test_an_indefinite_covariance_reports_its_node_and_writes_nothing(G):
    c = case("one_tile_T65")
    bad = c["S"].copy()
    bad[40] = -10.0
    bad[7] = -10.0
    with PT.device(G, c) as dev:
        with pytest.raises(G.PosDefException) as ei:
            dev.theta_objective_psi_xu(c["mean"], bad, c["Y"], want_grad=True)
        assert ei.value.info == 8 and "node 7" in str(ei.value)
        buf = np.full((c["M"], c["D"]), -7.25)
        rc, info, _ = raw_call(dev, c, bad, buf)
        assert rc == 8 and info == [0, 8]
        assert np.all(buf == -7.25)                                # a failed call leaves grad_xu unwritten
        _, gxu = dev.theta_objective_psi_xu(c["mean"], c["S"], c["Y"])  # the handle is as good as before
    assert_close("after an indefinite node", gxu, c["gxu"])


@pytest.mark.parametrize("learn_theta", [False, True], ids=["Xu", "theta_Xu"])
def test_optimize_inducing_exact_follows_the_host_loop(G, learn_theta):
    from gaussianprocessnode_amd import train
    from gaussianprocessnode_amd.meta import softplus
    from oracle import sgp_oracle as O
    c = case("one_tile_T65")
    M, D, steps = c["M"], c["D"], 5
    theta0 = O.invsoftplus(np.concatenate([[SIGMA2], c["ell"]]))
    Uv = np.linalg.cholesky(c["Rv"]).T
    with PT.device(G, c) as dev:
        th, Z, vals = train.optimize_inducing(theta0, c["Xu"], dev, q_v=(c["mu"], Uv), steps=steps, learn_theta=learn_theta,
                                              jitter=c["jitter"], optimizer=train.AdaMax(eta=1e-3), psi="exact",
                                              inputs=(c["mean"], c["S"], c["Y"]))
    nt = theta0.size if learn_theta else 0

    def grad(x):
        t = x[:nt] if learn_theta else theta0
        p = softplus(t)
        a = (p[0], p[1:], c["mean"], c["S"], c["Y"], c["Rv"], c["mu"], c["W"], x[nt:].reshape(M, D), c["jitter"])
        g = TR.analytic_grad(*a, n_ell=D) / (1.0 + np.exp(-t))
        return TR.objective(*a), np.concatenate([g[:nt], XR.analytic_grad_xu(*a).ravel()])
    x, values = XR.adamax(np.concatenate([theta0[:nt], c["Xu"].ravel()]), grad, steps, eta=1e-3)
    print(f"optimize_inducing(psi='exact') learn_theta={learn_theta}: values rel {np.max(np.abs(vals - values) / np.abs(values)):.3g}, "
          f"Xu rel {np.max(np.abs(Z - x[nt:].reshape(M, D)) / np.abs(x[nt:].reshape(M, D))):.3g}")
    np.testing.assert_allclose(vals, values, rtol=1e-6)
    np.testing.assert_allclose(Z, x[nt:].reshape(M, D), rtol=1e-6)
    np.testing.assert_allclose(th, x[:nt] if learn_theta else theta0, rtol=1e-6)
    assert not np.allclose(Z, c["Xu"])


def test_optimize_inducing_default_route_is_unchanged(G):
    """The new keywords at their defaults change no bit of what the call without them returns."""
    from gaussianprocessnode_amd import train
    from oracle import sgp_oracle as O
    c = case("one_tile_T65")
    theta0 = O.invsoftplus(np.concatenate([[SIGMA2], c["ell"]]))
    Uv = np.linalg.cholesky(c["Rv"]).T
    out = []
    for kw in (dict(), dict(psi="cubature", inputs=None)):
        with PT.device(G, c, posterior=False) as dev:
            dev.set_data(c["mean"], c["Y"])
            out.append(train.optimize_inducing(theta0, c["Xu"], dev, q_v=(c["mu"], Uv), steps=3, jitter=c["jitter"], **kw))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    with PT.device(G, c) as dev:
        with pytest.raises(ValueError):
            train.optimize_inducing(theta0, c["Xu"], dev, q_v=(c["mu"], Uv), steps=1, psi="exact")
        dev.set_kernel_family("matern32")
        with pytest.raises(ValueError):
            train.optimize_inducing(theta0, c["Xu"], dev, q_v=(c["mu"], Uv), steps=1, psi="exact", inputs=(c["mean"], c["S"], c["Y"]))
