"""The upper half of the size range a handle accepts (d_out * M <= 4032: up to 63 tile columns in the K_uu and the Lambda chain)
against the oracle: the sgp_create edge, UniSGP sweeps at M = 2049 / 3001 / 4032 on both sides of the SYRK gate and in every
sweep order, MultiSGP at the limit for every d_out (and a ragged Q = 4000 whose output blocks straddle tiles) with every prior
form, the other entry points at the limit, the stand-alone potrf / potri up to n = 4500, and the status codes at size.

Fixtures and bounds are those of test_envelope_host.py, which also shows, on the CPU, that the bounds see a dropped late
update, a mis-mapped Kronecker block and a lost log-det slot."""
import math

import numpy as np
import pytest
from scipy.linalg import cholesky, lapack, solve_triangular

from oracle import sgp_oracle as O
from tests import multi_theta_ref as R
from tests.test_envelope_host import (EPS, LIMIT, MULTI_DIN, MULTI_ELL, MULTI_JIT, MULTI_RAGGED, MULTI_S2, UNI_D, UNI_ELL,
                                      UNI_JIT, UNI_PRIOR, UNI_S2, UNI_W, multi_reference, relF, uni_inputs, uni_reference)
from tests.test_envelope_host import spd_cond
from tests.test_gpu_parity import kuu_tol, post_tol
from tests.test_gpu_reuse_stats import assert_bitwise, snapshot
from tests.test_gpu_xu_grad import COND_MAX
from tests.xu_grad_coverage import geometry as xu_geometry
from tests.xu_grad_ref import analytic_grad_xu

pytestmark = pytest.mark.gpu

FULL, TARGETS, REUSED = 0, 1, 2


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


# ------------------------------------------------------------------------------------------------
# 1. the create edge
@pytest.mark.parametrize("d_out", [1, 2, 3, 4])
def test_create_accepts_the_limit_and_refuses_one_more(G, d_out):
    m = LIMIT // d_out
    with G.SGPDevice(16, m, 2, d_out) as dev:
        assert dev.Q == m * d_out <= LIMIT
    with pytest.raises(G.SGPError) as e:
        G.SGPDevice(16, m + 1, 2, d_out)
    assert "status -1" in str(e.value) and "limited to 4032" in str(e.value)


# ------------------------------------------------------------------------------------------------
# 2. UniSGP sweeps across the upper range
def uni_device(G, N, M, keep_kuf=False, reuse_stats=False, y=None):
    X, Xu, y0 = uni_inputs(N, M)
    dev = G.SGPDevice(N, M, UNI_D, keep_kuf=keep_kuf, reuse_stats=reuse_stats)
    dev.set_inducing(Xu)
    dev.set_data(X, y0 if y is None else y)
    dev.set_kernel(UNI_S2, np.full(UNI_D, UNI_ELL), UNI_JIT)
    dev.set_prior_isotropic(UNI_PRIOR)
    dev.set_noise([[UNI_W]])
    return dev


def check_uni(r, N, Psi2, B, KuuL, post, sc):
    """The sweep's outputs against the oracle at the bounds of test_gpu_parity; returns the error / bound ratios."""
    ref = r["ref"]
    mu, Sig, Uv = post
    ratios = {}
    ratios["Psi2"] = relF(Psi2, ref.stats.Psi2) / 1e-13
    ratios["B"] = relF(B, ref.stats.b) / 1e-13
    ratios["KuuL"] = relF(KuuL, ref.KuuL) / kuu_tol(r["cond_K"])
    tol = post_tol(r["cond_L"])
    for k, a, b in (("mu", mu, ref.mu_v), ("Sigma", Sig, ref.Sigma_v), ("Uv", Uv, ref.Uv)):
        ratios[k] = relF(a, b) / tol
    tol_I1 = 50 * EPS * r["cond_K"] * ref.stats.s_kk + 1e-12
    ratios["sum_I1"] = abs(sc.sum_I1 - ref.sum_I1) / tol_I1
    ratios["sum_I2"] = abs(sc.sum_I2 - ref.sum_I2) / (max(1e-7, tol) * abs(ref.sum_I2))
    ratios["energy"] = abs(sc.energy - ref.energy) / (max(1e-7, tol) * abs(ref.energy) + 0.5 * UNI_W * tol_I1)
    ratios["logdet_kuu"] = abs(sc.logdet_kuu - r["logdet_K"]) / r["tol_ldK"]
    ratios["logdet_lambda"] = abs(sc.logdet_lambda - r["logdet_L"]) / r["tol_ldL"]
    assert sc.info_kuu == 0 and sc.info_lambda == 0
    assert np.allclose(np.tril(Uv, -1), 0.0)
    bad = {k: v for k, v in ratios.items() if not v < 1.0}
    assert not bad, (N, bad)
    return ratios


# M = 2049: the first tile past 32; 3001: ragged, mid-range; 4032: the limit.  N = 4 / 5 at M = 4032 (2016 lower tiles) and
# N = 8 / 9 at M = 3001 (1128) sit on either side of the SYRK gate (points x lower tiles >= 10 000: k_syrk_direct, below it
# k_syrk_stream)
UNI_CASES = [(3000, 2049), (2500, 3001), (3000, 4032), (4, 4032), (5, 4032), (8, 3001), (9, 3001)]


@pytest.mark.parametrize("N,M", UNI_CASES)
def test_unisgp_sweep_at_the_limit(G, N, M):
    r = uni_reference(N, M)
    with uni_device(G, N, M) as dev:
        dev.sweep()
        Psi2, B, sc_data = dev.stats()
        KuuL = dev.kuu_chol()
        post = dev.posterior()
        sc = dev.scalars()
    assert sc_data[2] == N
    ratios = check_uni(r, N, Psi2, B, KuuL, post, sc)
    print(f"N={N} M={M} worst error / bound:", {k: f"{v:.2g}" for k, v in ratios.items()})


@pytest.mark.parametrize("overlap,cols", [("0", None), ("1", None), ("1", "40"), ("1", "9,47")])
def test_unisgp_sweep_orders_at_the_limit(G, overlap, cols, monkeypatch):
    """M = 4032 in the plain order, the overlapped order the planner picks, and groupings cut beyond tile column 32."""
    N, M, T = 3000, 4032, 63
    monkeypatch.setenv("SGP_OVERLAP", overlap)
    if cols:
        monkeypatch.setenv("SGP_OVERLAP_COLS", cols)
    r = uni_reference(N, M)
    with uni_device(G, N, M) as dev:
        plan = dev.overlap_plan()
        outs = []
        for _ in range(2):
            dev.sweep()
            Psi2, B, _ = dev.stats()
            outs.append((Psi2, B, dev.kuu_chol(), dev.posterior(), dev.scalars()))
    if overlap == "0":
        assert plan == []
    else:
        assert len(plan) >= 2 and plan[0]["col_begin"] == 0 and plan[-1]["col_end"] == T and plan[0]["masked"] == 0
        assert all(g["masked"] == 1 for g in plan[1:]) and sum(g["tiles"] for g in plan) == T * (T + 1) // 2
        assert all(a["col_end"] == b["col_begin"] for a, b in zip(plan, plan[1:]))
        assert all(g["form_step"] == g["col_begin"] for g in plan)
        if cols:
            assert [g["col_end"] for g in plan[:-1]] == [int(c) for c in cols.split(",")]
    ratios = check_uni(r, N, *outs[-1])
    for a, b in zip(outs[0][3], outs[-1][3]):                  # run-to-run bitwise identical
        assert np.array_equal(a, b)
    print(f"order {overlap} cols {cols} plan {[(g['col_begin'], g['col_end']) for g in plan]} worst error / bound:",
          {k: f"{v:.2g}" for k, v in ratios.items()})


# ------------------------------------------------------------------------------------------------
# 3. MultiSGP at the limit: (d_out, M, T nodes, prior form, Gaussian q_out)
MULTI_CASES = [(2, 2016, 500, "isotropic", True), (3, 1344, 450, "precision", False), (4, 1008, 420, "meancov", True),
               (4, 1000) + MULTI_RAGGED]


def multi_device(G, m, d_out, M, gauss_out):
    f = m["f"]
    T, S = f["pts"].shape[:2]
    dev = G.SGPDevice(T * S, M, MULTI_DIN, d_out=d_out)
    dev.set_inducing(f["Xu"])
    dev.set_data(f["pts"].reshape(T * S, MULTI_DIN), np.repeat(f["Y"], S, axis=0), None, f["wts"].reshape(-1), n_nodes=T)
    if gauss_out:
        dev.set_output_cov_sum(f["Sig_y"].sum(axis=0))
    dev.set_kernel(MULTI_S2, np.full(MULTI_DIN, MULTI_ELL), MULTI_JIT)
    kind, *args = m["dev_prior"]
    if kind == "isotropic":
        dev.set_prior_isotropic(*args)
    elif kind == "precision":
        dev.set_prior_precision(*args)
    else:
        dev.set_prior_meancov(*args)
    dev.set_noise(f["W"], f["E_logdetW"])
    return dev


@pytest.mark.parametrize("d_out,M,T,prior,gauss_out", MULTI_CASES)
def test_multisgp_sweep_at_the_limit(G, d_out, M, T, prior, gauss_out):
    m = multi_reference(d_out, M, T, prior, gauss_out)
    f, ms = m["f"], m["ms"]
    with multi_device(G, m, d_out, M, gauss_out) as dev:
        dev.sweep()
        Psi2, B, sc_data = dev.stats()
        mu, Sig, Uv = dev.posterior()
        Sw = dev.wishart_invscale()
        sc = dev.scalars()
        dev.carry_posterior()
        dev.sweep()
        mu2, Sig2, _ = dev.posterior(want_uv=False)
        sc2 = dev.scalars()
    ratios = {}
    ratios["Psi2"] = relF(Psi2, ms.Psi2) / 1e-12
    ratios["B"] = relF(B, ms.B) / 1e-12
    assert sc_data[2] == T and math.isclose(sc_data[1], T, rel_tol=1e-12)
    tol = post_tol(m["cond_L"])
    ratios["mu"] = relF(mu, m["mu"]) / tol
    ratios["Sigma"] = relF(Sig, m["Sig"]) / tol
    ratios["UvUv"] = relF(Uv.T @ Uv, m["Sig"] + np.outer(m["mu"], m["mu"])) / tol
    assert np.allclose(np.tril(Uv, -1), 0.0)
    # the diagonal of S and the energy carry sum I1 = s_kk - tr(Kuu^-1 Psi2), which cancels: cond(Kuu) eps s_kk
    tol_I1 = 50 * EPS * m["cond_K"] * MULTI_S2 * T
    ratios["wishart"] = np.abs(Sw - m["S_w"]).max() / (max(1e-7, tol) * np.abs(m["S_w"]).max() + tol_I1)
    ratios["energy"] = abs(sc.energy - m["energy"]) / (max(1e-7, tol) * abs(m["energy"]) + 0.5 * np.trace(f["W"]) * tol_I1)
    ratios["logdet_kuu"] = abs(sc.logdet_kuu - m["logdet_K"]) / m["tol_ldK"]
    ratios["logdet_lambda"] = abs(sc.logdet_lambda - m["logdet_L"]) / m["tol_ldL"]
    # after carry_posterior, the same data once more: Lambda0 + 2 W (x) Psi2
    tol2 = post_tol(m["cond_L2"])
    ratios["mu carried"] = relF(mu2, m["mu2"]) / tol2
    ratios["Sigma carried"] = relF(Sig2, m["Sig2"]) / tol2
    ratios["logdet_lambda carried"] = abs(sc2.logdet_lambda - m["logdet_L2"]) / m["tol_ldL"]
    assert sc.info_kuu == 0 and sc.info_lambda == 0 and sc2.info_lambda == 0
    bad = {k: v for k, v in ratios.items() if not v < 1.0}
    assert not bad, bad
    print(f"d_out={d_out} M={M} {prior} worst error / bound:", {k: f"{v:.2g}" for k, v in ratios.items()})


# ------------------------------------------------------------------------------------------------
# 4. other entry points at the limit
def test_w_stats_at_the_limit(G):
    """k_quadform_fused at M = 4032 (63 tile rows of K_uf) against the oracle's per-point quantities."""
    N, M = 3000, 4032
    r = uni_reference(N, M)
    X, Xu, y = uni_inputs(N, M)
    ell = np.full(UNI_D, UNI_ELL)
    with uni_device(G, N, M, keep_kuf=True) as dev:
        dev.sweep()
        mu, _, Uv = dev.posterior()
        I1, I2 = dev.w_stats()
    rI1, rI2 = O.w_stats_perpoint(Xu, X, y, None, UNI_S2, ell, r["ref"].KuuL, mu, Uv)
    tol_I1 = 50 * EPS * r["cond_K"] * UNI_S2 + 1e-12
    scale_I2 = float(np.max(y * y + np.sum((Uv @ O.kernelmatrix(UNI_S2, ell, Xu, X)) ** 2, axis=0)))
    tol_I2 = post_tol(r["cond_L"]) * scale_I2
    e1, e2 = np.abs(I1 - rI1).max() / tol_I1, np.abs(I2 - rI2).max() / tol_I2
    assert e1 < 1 and e2 < 1, (e1, e2)
    print(f"w_stats worst error / bound: I1 {e1:.2g} I2 {e2:.2g}")


def predict_reference(Xu, Xs, s2, ell, KuuL, mu_v, Sigma_v, cond_K, cond_S, d_out):
    """test_gpu_predict_var.reference with the condition numbers passed in (no SVD of a 4032 x 4032 matrix)."""
    M = Xu.shape[0]
    Ks = O.kernelmatrix(s2, ell, Xu, Xs)
    A = solve_triangular(KuuL, Ks, lower=True)
    qff = s2 - np.sum(A * A, axis=0)
    mean = np.stack([Ks.T @ mu_v[o * M:(o + 1) * M] for o in range(d_out)], axis=1)
    forms = np.empty((Xs.shape[0], d_out, d_out))
    for i in range(d_out):
        for j in range(d_out):
            forms[:, i, j] = np.sum(Ks * (Sigma_v[i * M:(i + 1) * M, j * M:(j + 1) * M] @ Ks), axis=0)
    C = forms + qff[:, None, None] * np.eye(d_out)[None]
    diag = np.sqrt(np.abs(np.einsum("sii->si", forms)))
    tol = 50 * EPS * (cond_K * s2 * np.eye(d_out)[None] + cond_S * diag[:, :, None] * diag[:, None, :])
    return mean, C, tol


@pytest.mark.parametrize("d_out", [1, 2])
def test_predict_and_predict_var_at_the_limit(G, d_out, monkeypatch):
    """M = 4032 and (d_out, M) = (2, 2016), 2345 test points in chunks of 1000 (and in the default chunking), with and
    without the noise term."""
    ns = 2345
    Xs = np.random.default_rng(d_out).uniform(-2.0, 2.0, (ns, UNI_D if d_out == 1 else MULTI_DIN))
    out = {}
    for chunk in (None, "1000"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        if d_out == 1:
            r = uni_reference(3000, 4032)
            dev = uni_device(G, 3000, 4032)
            Xu, s2, ell, KuuL, Winv = uni_inputs(3000, 4032)[1], UNI_S2, np.full(UNI_D, UNI_ELL), r["ref"].KuuL, np.eye(1) / UNI_W
            cond_K, cond_S = r["cond_K"], r["cond_L"]
        else:
            m = multi_reference(*MULTI_CASES[0])
            dev = multi_device(G, m, 2, 2016, MULTI_CASES[0][4])
            Xu, s2, ell, KuuL = m["f"]["Xu"], MULTI_S2, np.full(MULTI_DIN, MULTI_ELL), cholesky(m["Kuu"], lower=True)
            Winv, cond_K, cond_S = np.linalg.inv(m["f"]["W"]), m["cond_K"], m["cond_L"]
        with dev:
            dev.sweep()
            mu, Sig, _ = dev.posterior(want_uv=False)
            pm = dev.predict(Xs)
            mv, var = dev.predict_var(Xs)
            mv_n, var_n = dev.predict_var(Xs, noise=True)
        assert np.array_equal(pm, mv) and np.array_equal(mv, mv_n)
        out[chunk] = (mv, var, var_n)
    assert all(np.array_equal(a, b) for a, b in zip(out[None], out["1000"]))
    m_ref, C_ref, tol = predict_reference(Xu, Xs, s2, ell, KuuL, mu, Sig, cond_K, cond_S, d_out)
    C = var.reshape(ns, d_out, d_out)
    C_n = var_n.reshape(ns, d_out, d_out)
    mv = mv.reshape(ns, d_out)
    e_var = (np.abs(C - C_ref) / tol).max()
    e_mean = np.abs(mv - m_ref).max() / (1e-9 * np.abs(m_ref).max())
    assert e_var < 1 and e_mean < 1, (e_var, e_mean)
    assert np.array_equal(C, C.transpose(0, 2, 1)) and np.array_equal(C_n, C_n.transpose(0, 2, 1))
    # the noise flag adds W^-1: one rounding of the sum, plus W^-1's own (the device inverts the d_out x d_out W itself)
    d = np.abs(C_n - (C + Winv[None]))
    assert np.all(d <= 2 * np.spacing(np.abs(C_n) + np.abs(Winv)[None]) + 4 * EPS * np.abs(Winv).max()), d.max()
    print(f"predict_var d_out={d_out} worst error / bound: var {e_var:.2g} mean {e_mean:.2g}")


def test_unisgp_theta_objective_at_the_limit(G):
    """Value and analytic gradient at M = 4032 against the oracle objective and its central differences (isotropic
    lengthscale: two parameters)."""
    N, M = 3000, 4032
    X, Xu, y = uni_inputs(N, M)
    p0 = np.array([1.05 * UNI_S2, 1.1 * UNI_ELL])                  # the optimiser's next theta
    with uni_device(G, N, M) as dev:
        dev.set_kernel(UNI_S2, [UNI_ELL], UNI_JIT)
        dev.sweep()
        mu0, _, Uv0 = dev.posterior()
        dev.set_kernel(p0[0], p0[1:], UNI_JIT)
        val, grad = dev.theta_objective(want_grad=True, n_ell=1)
        xu_val, xu_grad, gxu = dev.theta_objective_xu(want_grad=True)

        def f_dev(p):
            dev.set_kernel(p[0], p[1:], UNI_JIT)
            return dev.theta_objective(want_grad=False, n_ell=1)
        g_dev = np.array([(f_dev(p0 + 1e-5 * e) - f_dev(p0 - 1e-5 * e)) / 2e-5 for e in np.eye(2)])
    f = lambda p: O.theta_objective(Xu, X, y, p[0], np.full(UNI_D, p[1]), mu0, Uv0, UNI_W, jitter=UNI_JIT)
    ref = f(p0)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(2)])
    assert math.isclose(val, ref, rel_tol=1e-8), (val, ref)
    np.testing.assert_allclose(grad, g_dev, rtol=5e-5, atol=1e-6 * np.abs(g_dev).max())
    np.testing.assert_allclose(grad, g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())
    print(f"theta M=4032: value rel err {abs(val - ref) / abs(ref):.2g}, gradient rel err "
          f"{np.abs(grad - g_ref).max() / np.abs(g_ref).max():.2g}")
    # the gradient in the inducing inputs behind it: T = 63, four ranges of 12, 12, 12 and 11 point blocks
    assert xu_geometry(N, M)[:5] == (63, 47, 12, 4, 11)
    assert xu_val == val and np.array_equal(xu_grad, grad) and gxu.shape == (M, UNI_D) and np.all(np.isfinite(gxu))
    cond = spd_cond(O.kernelmatrix(p0[0], np.full(UNI_D, p0[1]), Xu) + UNI_JIT * np.eye(M))
    assert cond < COND_MAX, cond                                   # so the bound of tests/test_gpu_xu_grad.py holds here as well
    x_ref = analytic_grad_xu(p0[0], p0[1:], X, np.ones(N), y, Uv0.T @ Uv0, mu0, [[UNI_W]], Xu, UNI_JIT)
    print(f"theta_objective_xu M=4032: cond(K_uu) {cond:.3g}, grad_xu error / bound = "
          f"{(np.abs(gxu - x_ref) / (1e-6 * np.abs(x_ref) + 1e-9 * np.abs(x_ref).max())).max():.3g}")
    np.testing.assert_allclose(gxu, x_ref, rtol=1e-6, atol=1e-9 * np.abs(x_ref).max())


def test_multisgp_theta_objective_at_the_limit(G):
    """(d_out, M) = (4, 1008): value and gradient against tests/multi_theta_ref.py's summed form and its analytic gradient."""
    d_out, M, T, prior, gauss_out = MULTI_CASES[2]
    m = multi_reference(d_out, M, T, prior, gauss_out)
    f = m["f"]
    S = f["pts"].shape[1]
    X, om, Yp = f["pts"].reshape(-1, MULTI_DIN), f["wts"].reshape(-1), np.repeat(f["Y"], S, axis=0)
    p0 = np.concatenate([[1.05 * MULTI_S2], MULTI_ELL * np.linspace(0.9, 1.1, MULTI_DIN)])
    with multi_device(G, m, d_out, M, gauss_out) as dev:
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        dev.set_kernel(p0[0], p0[1:], MULTI_JIT)
        val, grad = dev.theta_objective(want_grad=True)
        xu_val, xu_grad, gxu = dev.theta_objective_xu(want_grad=True)
    Rv = Sig + np.outer(mu, mu)
    fo = lambda p: R.batched_objective(p[0], p[1:], X, om, Yp, Rv, mu, f["W"], f["Xu"], MULTI_JIT)
    ref = fo(p0)
    g_an = R.analytic_grad(p0[0], p0[1:], X, om, Yp, Rv, mu, f["W"], f["Xu"], MULTI_JIT)
    g_fd = np.array([(fo(p0 + 1e-6 * e) - fo(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + MULTI_DIN)])
    assert math.isclose(val, ref, rel_tol=1e-8), (val, ref)
    np.testing.assert_allclose(grad, g_an, rtol=1e-6, atol=1e-9 * np.abs(g_an).max())
    np.testing.assert_allclose(grad, g_fd, rtol=5e-5, atol=1e-6 * np.abs(g_fd).max())
    print(f"theta (4, 1008): value rel err {abs(val - ref) / abs(ref):.2g}, gradient rel err "
          f"{np.abs(grad - g_an).max() / np.abs(g_an).max():.2g}")
    # the gradient in the inducing inputs behind it: T = 16 with four outputs, 15 ranges of 4 point blocks
    assert xu_geometry(len(X), M)[:5] == (16, 60, 4, 15, 4)
    assert xu_val == val and np.array_equal(xu_grad, grad) and gxu.shape == (M, MULTI_DIN) and np.all(np.isfinite(gxu))
    x_ref = analytic_grad_xu(p0[0], p0[1:], X, om, Yp, Rv, mu, f["W"], f["Xu"], MULTI_JIT)
    print(f"theta_objective_xu (4, 1008): grad_xu error / bound = "
          f"{(np.abs(gxu - x_ref) / (1e-6 * np.abs(x_ref) + 1e-9 * np.abs(x_ref).max())).max():.3g}")
    np.testing.assert_allclose(gxu, x_ref, rtol=1e-6, atol=1e-9 * np.abs(x_ref).max())


def test_reused_and_targets_sweeps_at_the_limit(G):
    """SGP_FLAG_REUSE_STATS at M = 4032: a REUSED sweep (new noise) and a TARGETS sweep (new targets) are bitwise full sweeps."""
    N, M = 3000, 4032
    y2 = np.cos(uni_inputs(N, M)[0][:, 0])
    with uni_device(G, N, M, keep_kuf=True, reuse_stats=True) as a, uni_device(G, N, M, keep_kuf=True) as b:
        for dev in (a, b):
            dev.sweep()
        assert_bitwise(snapshot(a), snapshot(b), "first sweep")
        for name, step, kind in (("set_noise", lambda d: d.set_noise([[2.0 * UNI_W]]), REUSED),
                                 ("set_targets", lambda d: d.set_targets(y2), TARGETS)):
            for dev in (a, b):
                step(dev)
            assert a.sweep_kind()[0] == kind and b.sweep_kind()[0] == FULL, name
            for dev in (a, b):
                dev.sweep()
            assert a.sweep_kind()[1] == kind, name
            assert_bitwise(snapshot(a), snapshot(b), f"after {name}")


# ------------------------------------------------------------------------------------------------
# 5. the stand-alone building blocks
def spd_with_condition(n, cond, seed):
    """Q diag(ev) Q^T with log-spaced eigenvalues 1 .. 1 / cond: a random SPD matrix of known condition number."""
    rng = np.random.default_rng(seed)
    Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.geomspace(1.0, 1.0 / cond, n)
    A = (Qm * ev) @ Qm.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("n", [1000, 2047, 2048, 2049, 4031, 4032, 4096, 4097, 4500])
def test_potrf_potri_up_to_and_past_the_limit(G, n):
    """n > 4096 (65 and more factorisation steps) needs scratch for one log-det slot per step: sized by n since the fix."""
    cond = 100.0
    A = spd_with_condition(n, cond, seed=n)
    L = G.potrf(A)
    assert np.array_equal(np.triu(L, 1), np.zeros((n, n)))
    np.testing.assert_allclose(L, np.linalg.cholesky(A), rtol=1e-10, atol=1e-12)
    back = np.linalg.norm(L @ L.T - A) / np.linalg.norm(A)             # reference-free backward error
    assert back <= n * EPS, (back, n * EPS)
    Ai = G.potri(A)
    assert relF(Ai, np.linalg.inv(A)) < 1e-11
    np.testing.assert_allclose(Ai, Ai.T, rtol=0, atol=1e-13 * np.abs(Ai).max())
    resid = np.linalg.norm(A @ Ai - np.eye(n))                         # |A X - I|_F <= sqrt(n) c n eps cond(A)
    assert resid <= n ** 1.5 * EPS * cond, (resid, n ** 1.5 * EPS * cond)
    print(f"n={n}: backward error / bound {back / (n * EPS):.2g}, residual / bound {resid / (n ** 1.5 * EPS * cond):.2g}")


def test_potrf_reports_a_failing_minor_in_the_last_tile(G):
    n = 4032
    A = np.eye(n)
    A[4000, 4000] = -1.0
    with pytest.raises(G.PosDefException) as e:
        G.potrf(A)
    assert e.value.info == 4001


# ------------------------------------------------------------------------------------------------
# 6. status codes at size
def test_negative_noise_at_the_limit_is_reported(G):
    N, M = 3000, 4032
    with uni_device(G, N, M) as dev:
        dev.set_noise([[-UNI_W]], 0.0)                              # negative precision: Lambda indefinite
        dev.sweep()
        with pytest.raises(G.PosDefException) as e:
            dev.posterior()
    assert 1 <= e.value.info <= M


def test_indefinite_prior_covariance_at_size_is_reported(G):
    """(d_out, M) = (4, 1008): a Sigma0 whose leading minor 3501 is indefinite -- set_prior_meancov raises with LAPACK's index."""
    d_out, M = 4, 1008
    Q = d_out * M
    rng = np.random.default_rng(3)
    A = rng.normal(size=(Q, 64))
    S0 = A @ A.T / 64 + 0.5 * np.eye(Q)
    S0[3500, 3500] = -1.0
    want = lapack.dpotrf(S0, lower=1)[1]
    assert want == 3501
    with G.SGPDevice(64, M, 2, d_out) as dev:
        dev.set_inducing(np.random.default_rng(4).uniform(-1, 1, (M, 2)))
        dev.set_kernel(1.0, [1.0, 1.0], 1e-6)
        with pytest.raises(G.PosDefException) as e:
            dev.set_prior_meancov(np.zeros(Q), S0)
    assert e.value.info == want
