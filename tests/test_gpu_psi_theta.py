"""sgp_theta_objective_psi against the NumPy restatement (tests/psi_theta_ref.py) at the smallest shapes at which each part can go
wrong -- see CASES -- and its determinism, state and refusal contracts.

Bounds: value rel 1e-8, gradient rtol 1e-6 with atol 1e-9 max|g|: what tests/test_gpu_multi_theta.py sets for the same objective over
cubature points against NumPy.  The measured errors are printed and recorded in profiles/psi_theta.txt.
"""
import functools

import numpy as np
import pytest

from tests import psi_stats_ref as PR
from tests import psi_theta_ref as R
from tests import theta_descend_ref as DR

pytestmark = pytest.mark.gpu

VALUE_RTOL, GRAD_RTOL, GRAD_ATOL = 1e-8, 1e-6, 1e-9
SIGMA2 = 0.9

# name: (d_out, M, D, T, shared lengthscale, cov, jitter)
CASES = {
    "smallest_M": (1, 1, 2, 65, False, "full", 1e-8),
    "single_node": (2, 48, 2, 1, False, "full", 1e-8),
    "one_tile_T63": (2, 48, 2, 63, False, "full", 1e-8),
    "one_tile_T65": (2, 48, 2, 65, False, "full", 1e-8),
    "one_tile_T65_jitter1e-12": (2, 48, 2, 65, False, "full", 1e-12),
    "one_tile_T300": (2, 48, 2, 300, False, "full", 1e-8),
    "padded_second_tile": (1, 65, 1, 63, True, "full", 1e-8),
    "shared_ell_D5": (4, 65, 5, 65, True, "full", 1e-8),
    "six_tiles": (2, 130, 2, 65, False, "full", 1e-8),
    "D32": (1, 65, 32, 63, False, "full", 1e-8),
    "cov_null": (3, 65, 5, 65, False, "null", 1e-8),
    "cov_zero": (3, 65, 5, 65, False, "zero", 1e-8),
    "cov_rank1": (3, 65, 5, 65, False, "rank1", 1e-8),
}


# (M, D): lengthscale over sqrt(D) where the default would leave K_uu ill conditioned (it stays below 1e5)
SCALES = {(65, 1): 0.06, (130, 2): 0.2, (64, 2): 0.3}


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    return problem(name, CASES[name], 500 + sorted(CASES).index(name))


def problem(name, spec, seed):
    """The inputs of a case and the reference's value and gradient (computed once; arrays not to be written to).  q(v) is one VMP
    update from an isotropic prior over the exact statistics, so that the terms of the objective have their usual sizes."""
    d_out, M, D, T, shared, cov, jitter = spec
    rng = np.random.default_rng(seed)
    if (M, D) == (48, 2):
        Xu, ell, lo, hi = DR.pendulum_grid(), np.array([0.4, 1.0]), np.array([-1.3, -3.7]), np.array([1.3, 3.7])
    else:
        Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
        scale = SCALES.get((M, D), 0.45) * np.sqrt(D)
        ell = np.full(D, scale) if shared else scale * np.linspace(0.9, 1.1, D)
        lo, hi = np.full(D, -1.7), np.full(D, 1.7)
    mean = rng.uniform(lo, hi, (T, D))
    if cov == "full":
        A = rng.normal(size=(T, D, D)) * 0.3 * ell.mean() / np.sqrt(D)
        S = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    elif cov == "rank1":
        a = rng.normal(size=(T, D, 1)) * 0.3 * ell.mean()
        S = a @ a.transpose(0, 2, 1)
    elif cov == "zero":
        S = np.zeros((T, D, D))
    else:
        S = None
    Y = np.sin(mean @ rng.normal(size=(D, d_out)) / np.sqrt(D) * 2.0) + 0.05 * rng.normal(size=(T, d_out))
    A = rng.normal(size=(d_out, d_out))
    W = 20.0 * (A @ A.T / d_out + np.eye(d_out))
    psi1, psi2 = PR.psi_stats(Xu, SIGMA2, ell, mean, S)
    Sig = np.linalg.inv(np.kron(W, psi2) + np.eye(d_out * M) / 50.0)
    Sig = 0.5 * (Sig + Sig.T)
    mu = Sig @ ((psi1.T @ Y) @ W.T).T.ravel()
    Rv = Sig + np.outer(mu, mu)
    n_ell = 1 if shared else D
    ell_arg = ell[:1] if shared else ell
    f = R.objective(SIGMA2, ell_arg, mean, S, Y, Rv, mu, W, Xu, jitter)
    g = R.analytic_grad(SIGMA2, ell_arg, mean, S, Y, Rv, mu, W, Xu, jitter, n_ell=n_ell)
    return dict(name=name, d_out=d_out, M=M, D=D, T=T, n_ell=n_ell, ell=ell_arg, mean=mean, S=S, Y=Y, W=W, Xu=Xu, mu=mu, Rv=Rv,
                jitter=jitter, f=f, g=g)


def install(dev, c, posterior=True):
    dev.set_inducing(c["Xu"])
    dev.set_kernel(SIGMA2, c["ell"], c["jitter"])
    dev.set_noise(c["W"])
    if posterior:
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)


def device(G, c, posterior=True):
    dev = G.SGPDevice(max(8, c["T"]), c["M"], c["D"], d_out=c["d_out"])
    install(dev, c, posterior)
    return dev


def errors(f, g, f_ref, g_ref):
    ef = abs(f - f_ref) / abs(f_ref)
    eg = float(np.max(np.abs(g - g_ref) / (GRAD_RTOL * np.abs(g_ref) + GRAD_ATOL * np.max(np.abs(g_ref)))))
    return ef, eg


def assert_close(label, f, g, f_ref, g_ref):
    ef, eg = errors(f, g, f_ref, g_ref)
    print(f"theta_objective_psi {label}: value rel {ef:.3g} (bound {VALUE_RTOL:g}); gradient error / bound {eg:.3g}; "
          f"max rel grad {float(np.max(np.abs(g - g_ref) / np.max(np.abs(g_ref)))):.3g}")
    assert ef <= VALUE_RTOL, (f, f_ref)
    assert eg <= 1.0, (g, g_ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_value_and_gradient_match_the_restatement(G, name):
    c = case(name)
    with device(G, c) as dev:
        f, g = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        f2, g2 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        f3 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"])
    assert g.shape == (1 + c["n_ell"],)
    assert f == f2 == f3 and np.array_equal(g, g2)               # two calls agree bitwise
    assert_close(name, f, g, c["f"], c["g"])


@pytest.mark.parametrize("name", ["one_tile_T65", "one_tile_T300", "six_tiles"])
def test_the_chunk_size_changes_no_bit(G, name, monkeypatch):
    c = case(name)
    with device(G, c) as dev:
        f, g = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")
    with device(G, c) as dev:
        f64, g64 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
    assert f == f64 and np.array_equal(g, g64)


def test_null_covariance_matches_the_point_objective_on_the_means(G):
    c = case("cov_null")
    with device(G, c) as dev:
        f, g = dev.theta_objective_psi(c["mean"], None, c["Y"], want_grad=True)
    with device(G, c, posterior=False) as dev:
        dev.set_data(c["mean"], c["Y"])
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)
        f0, g0 = dev.theta_objective(want_grad=True)
    assert_close("cov=NULL against sgp_theta_objective on the means", f, g, f0, g0)


def test_works_after_an_exact_sweep_and_changes_nothing_the_sweep_keeps(G):
    c = case("one_tile_T65")
    with device(G, c, posterior=False) as dev:
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective_psi(c["mean"], c["S"], c["Y"])
        assert "status -1" in str(ei.value) and "q(v)" in str(ei.value)
        dev.set_prior_isotropic(50.0)
        dev.sweep_local_psi(c["mean"], c["S"], c["Y"])
        dev.sweep_finish()
        mu, Sig, Uv = dev.posterior()
        before = (dev.sweep_kind(), dev.stats(), (mu, Sig, Uv))
        f, g = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        after = (dev.sweep_kind(), dev.stats(), dev.posterior())
        assert before[0] == after[0]
        for a, b in zip(before[1] + before[2], after[1] + after[2]):
            assert np.array_equal(a, b)
        with pytest.raises(G.SGPError) as ei:                      # the refusal tests/test_gpu_psi_sweep.py pins is still there
            dev.theta_objective()
        assert "exact Psi-statistics" in str(ei.value)
        Rv = Sig + np.outer(mu, mu)
        args = (c["mean"], c["S"], c["Y"], Rv, mu, c["W"], c["Xu"], c["jitter"])
        assert_close("after sweep_local_psi + sweep_finish", f, g, R.objective(SIGMA2, c["ell"], *args),
                     R.analytic_grad(SIGMA2, c["ell"], *args))
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)  # a later set_posterior is honoured
        f, g = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        assert_close("set_posterior after the sweep", f, g, c["f"], c["g"])


def test_refusals(G):
    c = case("one_tile_T63")
    mean, S, Y = c["mean"], c["S"], c["Y"]

    def refused(dev, text, *args):
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective_psi(*(args or (mean, S, Y)))
        assert "status -1" in str(ei.value) and text in str(ei.value), str(ei.value)

    with G.SGPDevice(64, c["M"], c["D"], d_out=c["d_out"]) as dev:
        refused(dev, "set_inducing and set_kernel first")
        dev.set_inducing(c["Xu"])
        refused(dev, "set_inducing and set_kernel first")
        install(dev, c, posterior=False)
        refused(dev, "q(v)")
        install(dev, c)
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
        dev.theta_objective_psi(mean, S, Y)
    c1 = case("padded_second_tile")
    with device(G, c1) as dev:
        dev.train_begin(c1["mean"], c1["Y"][:, 0], np.zeros(2))
        with pytest.raises(G.SGPError) as ei:
            dev.theta_objective_psi(c1["mean"], c1["S"], c1["Y"])
        assert "status -1" in str(ei.value) and "a device-paced training run is open" in str(ei.value)
        dev.train_end()


def test_an_indefinite_covariance_reports_its_node(G):
    import ctypes as C
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = case("one_tile_T65")
    bad = c["S"].copy()
    bad[40] = -10.0
    bad[7] = -10.0
    with device(G, c) as dev:
        with pytest.raises(G.PosDefException) as ei:
            dev.theta_objective_psi(c["mean"], bad, c["Y"], want_grad=True)
        assert ei.value.info == 8 and "node 7" in str(ei.value)
        v, info = C.c_double(), (C.c_int64 * 2)()
        m, Sb, y = as_f64(c["mean"]), as_f64(bad), as_f64(c["Y"].T)
        rc = dev._lib.sgp_theta_objective_psi(dev._h, ptr(m), ptr(Sb), ptr(y), c["T"], C.cast(C.byref(v), C.POINTER(C.c_double)),
                                              None, info)
        assert rc == 8 and list(info) == [0, 8]
        f = dev.theta_objective_psi(c["mean"], c["S"], c["Y"])     # the handle is as good as before
    assert abs(f - c["f"]) <= VALUE_RTOL * abs(c["f"])
