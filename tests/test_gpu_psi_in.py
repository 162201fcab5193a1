"""sgp_psi_in_grad against the NumPy restatement (tests/psi_in_ref.py) at the smallest shapes at which each part can go wrong -- see
CASES -- with its determinism, state and refusal contracts, and the q(x) update built on it (multisgp.marginal_in_exact_batch,
train.vmp_gpssm(in_psi="exact")).

Bounds: those tests/test_gpu_psi_theta.py sets for this objective family -- value rel 1e-8 (per node), gradient rtol 1e-6 with atol
1e-9 max|g|, per node over the stacked (gamma, Gamma).  The measured errors are printed.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import psi_in_ref as R
from tests import psi_stats_ref as PR
from tests import theta_descend_ref as DR

pytestmark = pytest.mark.gpu

VALUE_RTOL, GRAD_RTOL, GRAD_ATOL = 1e-8, 1e-6, 1e-9
SIGMA2 = 0.9

# name: (d_out, M, D, T, shared lengthscale, cov)
CASES = {
    "smallest_M": (1, 1, 2, 65, False, "full"),
    "single_node": (2, 48, 2, 1, False, "full"),
    "one_tile_T63": (2, 48, 2, 63, False, "full"),
    "one_tile_T65": (2, 48, 2, 65, False, "full"),
    "one_tile_T300": (2, 48, 2, 300, False, "full"),
    "node_block_T257": (2, 48, 2, 257, False, "full"),
    "padded_second_tile_D1": (1, 65, 1, 63, True, "full"),
    "shared_ell_D5": (4, 65, 5, 65, True, "full"),
    "six_tiles": (2, 130, 2, 65, False, "full"),
    "D8": (1, 65, 8, 63, False, "full"),
    "cov_null": (3, 65, 5, 65, False, "null"),
    "cov_zero": (3, 65, 5, 65, False, "zero"),
    "cov_rank1": (3, 65, 5, 65, False, "rank1"),
}
JITTER = 1e-8


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


# (M, D): lengthscale over sqrt(D) where the default would leave K_uu ill conditioned (it stays below 1e5)
SCALES = {(65, 1): 0.06, (130, 2): 0.2, (64, 2): 0.3, (128, 2): 0.15, (17, 1): 0.2}


@functools.lru_cache(maxsize=None)
def case(name):
    return problem(name, CASES[name], 900 + sorted(CASES).index(name))


def problem(name, spec, seed, subset=None):
    """The inputs of a case and the reference's U, gamma, Gamma (computed once; arrays not to be written to), built as
    tests/test_gpu_psi_theta.py builds its cases: q(v) is one VMP update from an isotropic prior over the exact statistics.
    subset: the nodes q(v) is fitted to and the reference is evaluated at (an index array; default: all of them)."""
    d_out, M, D, T, shared, cov = spec
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
    sel = slice(None) if subset is None else subset
    S_sel = None if S is None else S[sel]
    psi1, psi2 = PR.psi_stats(Xu, SIGMA2, ell, mean[sel], S_sel)
    Sig = np.linalg.inv(np.kron(W, psi2) + np.eye(d_out * M) / 50.0)
    Sig = 0.5 * (Sig + Sig.T)
    mu = Sig @ ((psi1.T @ Y[sel]) @ W.T).T.ravel()
    Rv = Sig + np.outer(mu, mu)
    ell_arg = ell[:1] if shared else ell
    U, gamma, Gamma = R.evaluate(SIGMA2, ell_arg, mean[sel], S_sel, Y[sel], Rv, mu, W, Xu, JITTER)
    return dict(name=name, d_out=d_out, M=M, D=D, T=T, ell=ell_arg, mean=mean, S=S, Y=Y, W=W, Xu=Xu, mu=mu, Sig=Sig, Rv=Rv, jitter=JITTER,
                U=U, gamma=gamma, Gamma=Gamma)


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


def errors(U, gamma, Gamma, U_ref, gamma_ref, Gamma_ref):
    eu = float(np.max(np.abs(U - U_ref) / np.abs(U_ref)))
    g, g_ref = R.stacked(gamma, Gamma), R.stacked(gamma_ref, Gamma_ref)
    eg = float(np.max(np.abs(g - g_ref) / (GRAD_RTOL * np.abs(g_ref) + GRAD_ATOL * np.max(np.abs(g_ref), axis=1, keepdims=True))))
    return eu, eg


def assert_close(label, got, ref):
    eu, eg = errors(*got, *ref)
    print(f"psi_in_grad {label}: value rel {eu:.3g} (bound {VALUE_RTOL:g}); gradient error / bound {eg:.3g}")
    assert eu <= VALUE_RTOL
    assert eg <= 1.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_energy_and_derivatives_match_the_restatement(G, name):
    c = case(name)
    with device(G, c) as dev:
        U, gamma, Gamma = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
        U2, gamma2, Gamma2 = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
        none_U, gamma3, none_G = dev.psi_in_grad(c["mean"], c["S"], c["Y"], want_energy=False, want_cov=False)
    assert U.shape == (c["T"],) and gamma.shape == (c["T"], c["D"]) and Gamma.shape == (c["T"], c["D"], c["D"])
    assert np.array_equal(Gamma, Gamma.transpose(0, 2, 1))                       # exactly symmetric
    assert np.array_equal(U, U2) and np.array_equal(gamma, gamma2) and np.array_equal(Gamma, Gamma2)    # two calls agree bitwise
    assert none_U is None and none_G is None and np.array_equal(gamma, gamma3)
    assert_close(name, (U, gamma, Gamma), (c["U"], c["gamma"], c["Gamma"]))


@pytest.mark.parametrize("name", ["one_tile_T65", "one_tile_T300", "node_block_T257", "six_tiles"])
def test_the_chunk_size_changes_no_bit(G, name, monkeypatch):
    c = case(name)
    with device(G, c) as dev:
        a = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")
    with device(G, c) as dev:
        b = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["one_tile_T300", "shared_ell_D5", "cov_null"])
def test_the_energies_sum_to_the_theta_objective(G, name):
    c = case(name)
    with device(G, c) as dev:
        U, _, _ = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
        f = dev.theta_objective_psi(c["mean"], c["S"], c["Y"])
    total = U.sum() + 0.5 * np.trace(c["W"]) * SIGMA2 * c["T"]
    print(f"psi_in_grad {name}: sum of energies against theta_objective_psi rel {abs(total - f) / abs(f):.3g}")
    assert abs(total - f) <= 1e-8 * abs(f)


@pytest.mark.parametrize("name", ["cov_null", "one_tile_T65"])
def test_single_points_reproduce_in_message_grad(G, name):
    """S = 0: U = -logpdf - 1/2 tr(W) sigma2, gamma = -grad, Gamma = -1/2 hess of sgp_in_message_grad at the point m_t"""
    c = case(name)
    with device(G, c) as dev:
        got = dev.psi_in_grad(c["mean"], None, c["Y"])
        lp, grad, hess = dev.in_message_grad(c["mean"], np.arange(c["T"] + 1), c["Y"], c["mu"], c["Sig"])
    assert_close(f"{name}, cov = NULL against sgp_in_message_grad", got,
                 (-lp - 0.5 * np.trace(c["W"]) * SIGMA2, -grad, -0.5 * hess))


def test_an_indefinite_covariance_reports_its_node(G):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = case("one_tile_T65")
    bad = c["S"].copy()
    bad[40] = -10.0
    bad[7] = -10.0
    with device(G, c) as dev:
        with pytest.raises(G.PosDefException) as ei:
            dev.psi_in_grad(c["mean"], bad, c["Y"])
        assert ei.value.info == 8 and "node 7" in str(ei.value)
        info = (C.c_int64 * 2)()
        m, Sb, y, g = as_f64(c["mean"]), as_f64(bad), as_f64(c["Y"].T), np.empty((c["T"], c["D"]))
        rc = dev._lib.sgp_psi_in_grad(dev._h, ptr(m), ptr(Sb), ptr(y), c["T"], None, ptr(g), None, info)
        assert rc == 8 and list(info) == [0, 8]
        got = dev.psi_in_grad(c["mean"], c["S"], c["Y"])            # the handle is as good as before
    assert_close("after an indefinite node", got, (c["U"], c["gamma"], c["Gamma"]))


def test_refusals(G):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = case("one_tile_T63")
    mean, S, Y = c["mean"], c["S"], c["Y"]

    def refused(dev, text, *args):
        with pytest.raises(G.SGPError) as ei:
            dev.psi_in_grad(*(args or (mean, S, Y)))
        assert "status -1" in str(ei.value) and "sgp_psi_in_grad" in str(ei.value) and text in str(ei.value), str(ei.value)

    with G.SGPDevice(64, c["M"], c["D"], d_out=c["d_out"]) as dev:
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
        m, Sc, y = as_f64(mean), as_f64(S), as_f64(Y.T)
        rc = dev._lib.sgp_psi_in_grad(dev._h, ptr(m), ptr(Sc), ptr(y), c["T"], None, None, None, None)
        assert rc == -1 and b"grad_mean must not be NULL" in dev._lib.sgp_last_error(dev._h)
        dev.set_kernel_family("matern32")
        refused(dev, "SGP_KERNEL_SE only")
        dev.set_kernel_family("se")
        dev.set_allreduce(lambda buf, count, stream: 0)
        refused(dev, "all-reduce hook")
        dev.set_allreduce(None)
        dev.psi_in_grad(mean, S, Y)
    c1 = case("padded_second_tile_D1")
    with device(G, c1) as dev:
        dev.train_begin(c1["mean"], c1["Y"][:, 0], np.zeros(2))
        with pytest.raises(G.SGPError) as ei:
            dev.psi_in_grad(c1["mean"], c1["S"], c1["Y"])
        assert "status -1" in str(ei.value) and "a device-paced training run is open" in str(ei.value)
        dev.train_end()
    rng = np.random.default_rng(9)
    with G.SGPDevice(8, 4, 9) as dev:                              # D = 9: the per-node sums are sized for D <= 8
        dev.set_inducing(rng.normal(size=(4, 9)))
        dev.set_kernel(SIGMA2, np.full(9, 2.0), 1e-8)
        dev.set_noise([[2.0]])
        dev.set_posterior(np.zeros(4), np.eye(4))
        with pytest.raises(G.SGPError) as ei:
            dev.psi_in_grad(rng.normal(size=(3, 9)), None, np.zeros((3, 1)))
        assert "status -1" in str(ei.value) and "D > 8" in str(ei.value)


def test_changes_nothing_the_sweep_keeps(G):
    c = case("one_tile_T65")
    with device(G, c, posterior=False) as dev:
        dev.set_prior_isotropic(50.0)
        dev.sweep_local_psi(c["mean"], c["S"], c["Y"])
        dev.sweep_finish()
        mu, Sig, Uv = dev.posterior()
        before = (dev.sweep_kind(), dev.stats(), (mu, Sig, Uv))
        got = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
        after = (dev.sweep_kind(), dev.stats(), dev.posterior())
        assert before[0] == after[0]
        for a, b in zip(before[1] + before[2], after[1] + after[2]):
            assert np.array_equal(a, b)
        with pytest.raises(G.SGPError) as ei:                      # the refusal tests/test_gpu_psi_sweep.py pins is still there
            dev.theta_objective()
        assert "exact Psi-statistics" in str(ei.value)
        Rv = Sig + np.outer(mu, mu)
        assert_close("after sweep_local_psi + sweep_finish", got,
                     R.evaluate(SIGMA2, c["ell"], c["mean"], c["S"], c["Y"], Rv, mu, c["W"], c["Xu"], c["jitter"]))


# ---- the q(x) update on top of it ----
def gpssm_problem(T=12, M=10):
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    rng = np.random.default_rng(12)
    d = 2
    Xu = rng.uniform(-2.0, 2.0, (M, d))
    y = np.cumsum(0.3 * rng.normal(size=(T, d)), axis=0)
    meta = MultiSGPMeta(srcubature(), Xu, None, None, None, None, SEARDKernel(softplus_params=True), jitter=1e-8)
    kw = dict(P=0.1 * np.eye(d), x0_prior=(np.zeros(d), 0.5 * np.eye(d)))
    return np.log(np.expm1(np.ones(3))), y, meta, kw


def flat(res):
    q_x, q_v, q_w, fe = res
    return [np.concatenate([np.ravel(q.m) for q in q_x] + [np.ravel(q.S) for q in q_x]), np.ravel(q_v.m), np.ravel(q_v.S),
            np.ravel(q_w.invS), np.asarray(fe)]


def test_in_psi_cubature_is_bitwise_the_default(G):
    from gaussianprocessnode_amd.train import vmp_gpssm
    runs = {}
    for name, extra in (("default", {}), ("cubature", {"in_psi": "cubature"})):
        theta, y, meta, kw = gpssm_problem()
        try:
            runs[name] = flat(vmp_gpssm(theta, y, meta, iterations=2, free_energy=True, **kw, **extra))
        finally:
            if meta.engine is not None:
                meta.engine.close()
    for a, b in zip(runs["default"], runs["cubature"]):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        theta, y, meta, kw = gpssm_problem()
        vmp_gpssm(theta, y, meta, iterations=1, in_psi="other", **kw)


@pytest.mark.parametrize("psi", ["cubature", "exact"])
def test_in_psi_exact_runs_and_no_node_s_free_energy_rises(G, psi, monkeypatch):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.train import vmp_gpssm
    records = []
    inner = MS.marginal_in_exact_batch

    def recording(*args, **kwargs):
        marginals, rec = inner(*args, **kwargs)
        records.append(rec)
        return marginals, rec
    monkeypatch.setattr(MS, "marginal_in_exact_batch", recording)
    theta, y, meta, kw = gpssm_problem(T=20, M=16)
    try:
        q_x, q_v, q_w, fe = vmp_gpssm(theta, y, meta, iterations=2, free_energy=True, psi=psi, in_psi="exact", **kw)
    finally:
        if meta.engine is not None:
            meta.engine.close()
    assert len(records) == 2 and len(q_x) == 21 and np.all(np.isfinite(fe))
    for q in q_x:
        np.linalg.cholesky(q.S)                                     # every covariance is positive definite
    for rec in records:
        assert rec["before"].shape == (20,) and np.all(np.isfinite(rec["after"]))
        assert np.all(rec["after"] <= rec["before"])
    print(f"vmp_gpssm(psi={psi!r}, in_psi='exact'): free energies {fe}; steps taken " +
          ", ".join(f"{int(np.sum(r['rho'] > 0))}/20 (smallest rho {r['rho'].min():.3g})" for r in records))
