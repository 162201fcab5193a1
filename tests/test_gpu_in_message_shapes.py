"""sgp_in_message on the device at the shapes its first tests leave out (tests/in_message_ref.SHAPE_CASES): input dimensions
5..32 with ARD and isotropic lengthscales and nodes of up to four lane rounds, every kernel family with 1..4 outputs and points
on and ~1e-9 off inducing inputs, M and Q that are no multiple of the tile, 1001 small nodes, the d_out * M = 4032 limit, the
last sweep's q(v) of a UniSGP and a MultiSGP handle, sgp_predict_var on the same handle, and weights of 0.

Every comparison is with the NumPy reference of tests/in_message_ref.py at its bound model (per point tol_p, per node 2 tau,
4 tau r, 8 tau r^2 plus 1e-13 relative, plus the derived mean-rounding term), prints its worst error / bound ratio before it
asserts, is made twice with the two calls agreeing bitwise, and asserts every covariance block exactly symmetric."""
import numpy as np
import pytest

from tests import in_message_ref as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_for(G, c, n_max=64, **kw):
    dev = G.SGPDevice(n_max, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    return dev


def call(dev, c, qv=True):
    return dev.in_message(c["X"], c["start"], c["Y"], c["wts"], *((c["mu_v"], c["Sigma_v"]) if qv else ()))


def check(name, c, out):
    ratios = R.worst_ratios(c, *out)
    print(f"case {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(np.isfinite(x).all() for x in out)
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    assert np.array_equal(out[3], out[3].transpose(0, 2, 1))


def twice(name, dev, c, qv=True):
    out, again = call(dev, c, qv), call(dev, c, qv)
    for a, b in zip(out, again):
        assert np.array_equal(a, b)
    check(name, c, out)
    return out


def run_case(G, name):
    c = R.shape_reference(name)
    with device_for(G, c) as dev:
        return twice(name, dev, c)


@pytest.mark.parametrize("kern", ["ard", "iso"])
@pytest.mark.parametrize("D", R.DIMS)
def test_dimensions(G, D, kern):
    """M = 70, d_out = 2, nodes of 1, 64, 65, 129, 200 and 3 points: k_predict<0>, k_gram_uf<8> / <MAXD> without targets, the
    moment loops up to MAXD, four lane rounds."""
    run_case(G, f"dim{D}" + ("iso" if kern == "iso" else ""))


@pytest.mark.parametrize("d_out", [1, 2, 3, 4])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_families_and_outputs(G, family, d_out):
    """D = 9, M = 65; node 1 holds five inducing inputs (r = 0) and five points ~1e-9 from inducing inputs."""
    run_case(G, f"{family}x{d_out}")


@pytest.mark.parametrize("d_out", [3, 4])
@pytest.mark.parametrize("M", [1, 63, 64, 129])
def test_ragged_m_and_q(G, M, d_out):
    """M != M_p and Q != Q_p (M = 64: M = M_p, Q = Q_p), output blocks of Sigma_v straddling 64-tiles."""
    run_case(G, f"ragged{M}x{d_out}")


def test_many_small_nodes(G, monkeypatch):
    """1001 nodes of 1, 2, 3, 1, .. points: 251 workgroups of k_in_moments, the last with one node; the default chunk and 64-point
    chunks (32 of them) agree bitwise."""
    c = R.shape_reference("many")
    out = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        with device_for(G, c) as dev:
            out[chunk] = twice(f"many/chunk {chunk or 'default'}", dev, c)
    for a, b in zip(out[None], out["64"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["limit1", "limit4"])
def test_size_limit(G, name):
    """d_out = 1, M = 4032 (S and K_uu of 63 tile columns) and d_out = 4, M = 1008 (a 4032^2 Sigma_v read in 16 blocks per
    entry).  Then a Sigma_v whose entry j = M - 30 (output 0) is -100 on the diagonal and 0 beside it: S keeps its leading minor
    j positive definite and fails at j + 1, which the call returns; the handle then serves the first call again, bitwise."""
    c = R.shape_reference(name)
    j = c["M"] - 30
    with device_for(G, c) as dev:
        out = twice(name, dev, c)
        bad = np.array(c["Sigma_v"])
        bad[j, :] = bad[:, j] = 0.0
        bad[j, j] = -100.0
        with pytest.raises(G.PosDefException) as e:
            dev.in_message(c["X"], c["start"], c["Y"], c["wts"], c["mu_v"], bad)
        assert e.value.info == j + 1
        for a, b in zip(out, call(dev, c)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("d_out", [1, 3])
def test_null_posterior_after_a_sweep(G, d_out):
    """N = 300, M = 70, D = 3, a UniSGP (d_out = 1) and a MultiSGP handle: q(v) read in place from the last sweep is, bitwise,
    dev.posterior()'s passed explicitly, matches the reference evaluated at that posterior, and the calls leave sweep_kind()
    as it was."""
    c = R.make_shape_case(70, 3, d_out, "se", [5, 70, 1], seed=700 + d_out)
    rng = np.random.default_rng(710 + d_out)
    N = 300
    Xd = rng.uniform(-1.745, 1.745, (N, 3))
    yd = np.stack([np.sin(Xd.sum(axis=1) + o) for o in range(d_out)], axis=1) + 0.1 * rng.normal(size=(N, d_out))
    with device_for(G, c, n_max=N) as dev:
        dev.set_data(Xd, yd[:, 0] if d_out == 1 else yd)
        dev.set_prior_isotropic(50.0)
        dev.sweep()
        kind = dev.sweep_kind()
        mu, Sig, _ = dev.posterior(want_uv=False)
        ref = R.finish_shape(dict(c, mu_v=mu, Sigma_v=Sig))
        print(f"d_out {d_out}: cond(S) of the swept posterior {ref['cond_S']:.3g}")
        null = twice(f"swept d_out {d_out} / null", dev, ref, qv=False)
        explicit = twice(f"swept d_out {d_out} / explicit", dev, ref)
        for a, b in zip(null, explicit):
            assert np.array_equal(a, b)
        assert dev.sweep_kind() == kind


@pytest.mark.parametrize("family", ["se", "matern52"])
@pytest.mark.parametrize("d_out", [1, 3])
@pytest.mark.parametrize("D", [3, 16])
def test_logpdf_is_predict_vars_mean_and_covariance(G, D, d_out, family):
    """No oracle: with m, C_f of sgp_predict_var (no noise flag) on the same handle, points and explicit q(v),
        logpdf_p = -1/2 tr(W C_f,p) + y_t' W m_p - 1/2 m_p' W m_p
    (tr(W C_f) = tr(W) (sigma2 - |L_K^-1 k|^2) + sum_ij W_ij k' Sigma_v^(ij) k, and m' W m supplies the mu mu' part of S).
    Bound: tol_p for the left side; on the right, to first order in the errors dC, dm of predict_var,
        |d| <= 1/2 sum_ij |W_ij| |dC_ij| + sum_d |((y_t - m_p)' W)_d| |dm_d|,
    with |dC_ij| <= the error model of tests/test_gpu_predict_var.reference and |dm_d| <= 50 eps |k|' |mu^(d)|, a dot product's
    rounding as in tol_p's last term (dm' W dm is of second order, ~1e-26).  Fails if either call reads a stale mirror, a
    wrong factor or the other call's scratch."""
    from tests.test_gpu_predict_var import reference as predict_reference
    c = R.finish_shape(R.make_shape_case(70, D, d_out, family, [5, 70, 1], seed=800 + 10 * D + d_out))
    X, W, M = c["X"], c["W"], c["M"]
    n = len(X)
    with device_for(G, c) as dev:
        m, C = dev.predict_var(X, c["mu_v"], c["Sigma_v"])
        lp = dev.in_message(X, c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])
        m2, C2 = dev.predict_var(X, c["mu_v"], c["Sigma_v"])
        lp2 = dev.in_message(X, c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])
    assert np.array_equal(m, m2) and np.array_equal(C, C2) and np.array_equal(lp, lp2)
    with R.oracle_family(family):
        _, _, tolC = predict_reference(c["Xu"], X, c["sigma2"], c["ell"], c["jitter"], c["mu_v"], c["Sigma_v"], d_out)
    m, C, tolC = m.reshape(n, d_out), C.reshape(n, d_out, d_out), tolC.reshape(n, d_out, d_out)
    assert np.array_equal(C, C.transpose(0, 2, 1))
    node = np.repeat(np.arange(c["nodes"]), np.diff(c["start"]))
    y = c["Y"][node]                                                        # (n, d_out)
    rhs = -0.5 * np.einsum("ij,pji->p", W, C) + np.einsum("pi,ij,pj->p", y, W, m) - 0.5 * np.einsum("pi,ij,pj->p", m, W, m)
    K = R.kernel_of(c)(c["sigma2"], c["ell"], c["Xu"], X)                   # M x n
    dm = 50 * EPS * np.abs(K).T @ np.abs(c["mu_v"].reshape(d_out, M).T)     # (n, d_out)
    bound = c["tol"] + 0.5 * np.einsum("ij,pij->p", np.abs(W), tolC) + np.sum(np.abs((y - m) @ W) * dm, axis=1)
    ratio = float(np.max(np.abs(lp - rhs) / bound))
    print(f"D {D} d_out {d_out} {family}: logpdf vs predict_var's identity, error / bound {ratio:.3g}; "
          f"logpdf vs the reference {float(np.max(np.abs(lp - c['lp']) / c['tol'])):.3g}")
    assert np.isfinite(lp).all() and ratio <= 1.0


@pytest.mark.parametrize("kind", ["some_zero", "top_zero_near", "top_zero_far"])
def test_zero_weights_take_no_part(G, kind):
    """Weights of exactly 0; a node whose largest logpdf lies on a zero-weight point, 300 and 850 above its positively weighted
    points (the second underflowed every term of the earlier kernel's sums: log_norm -inf, mean and cov NaN)."""
    run_case(G, "w_" + kind)


def test_a_node_of_zero_weights_is_refused(G):
    c = R.shape_reference("w_some_zero")
    w = np.array(c["wts"])
    w[c["start"][1]:c["start"][2]] = 0.0
    with device_for(G, c) as dev:
        with pytest.raises(G.SGPError, match="sum to 0"):
            dev.in_message(c["X"], c["start"], c["Y"], w, c["mu_v"], c["Sigma_v"])
        lp = dev.in_message(c["X"], c["start"], c["Y"], None, c["mu_v"], c["Sigma_v"])     # (without weights: no moments asked)
        out = twice("w_some_zero after the refusal", dev, c)
        assert np.array_equal(lp, out[0])
