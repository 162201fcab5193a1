"""Batched :in messages without a GPU: the fixtures of tests/in_message_ref.py keep the numbers they were chosen for, the checks
the GPU file makes would catch the faults a kernel of this shape can have, `SGPDevice.in_message` packs its arguments the way
the C ABI states them, and the node mirrors' fallback logic does what the reference's products do."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaussianprocessnode_amd import multisgp as MS
from gaussianprocessnode_amd import unisgp as U
from gaussianprocessnode_amd.cubature import ghcubature, srcubature
from gaussianprocessnode_amd.device import SGPDevice
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, NormalMeanVariance, PointMass
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel, UniSGPMeta
from oracle import sgp_oracle as O
from tests import in_message_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(R.CASES)


# ------------------------------------------------------------------------------------------------
# 1. the ABI
def test_in_message_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    assert re.search(r"int\s+sgp_in_message\s*\(", txt)
    assert re.search(r"#define\s+SGP_ABI_VERSION\s+1\b", txt)
    from gaussianprocessnode_amd import _build, _lib
    assert "sgp_in_message" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "sgp_in_message")
    assert b"sgp_in_message" in open(_build.build(), "rb").read()


# ------------------------------------------------------------------------------------------------
# 2. the fixtures keep their numbers
def test_fixture_shapes():
    shapes = {n: (R.reference(n)["M"], R.reference(n)["D"], R.reference(n)["d_out"], R.reference(n)["nodes"],
                  len(R.reference(n)["X"]) // R.reference(n)["nodes"]) for n in ALL}
    assert shapes == {"a": (48, 2, 2, 7, 5), "b": (129, 3, 3, 5, 7), "c": (70, 1, 1, 4, 21), "d": (200, 5, 4, 3, 11),
                      "e": (48, 2, 2, 7, 5), "f": (48, 2, 2, 7, 5)}
    a, e = R.reference("a"), R.reference("e")
    assert (a["sigma2"], a["jitter"]) == (e["sigma2"], e["jitter"]) and np.array_equal(a["ell"], e["ell"])
    assert R.reference("c")["jitter"] == 1e-6 and R.reference("f")["family"] == "matern32"


@pytest.mark.parametrize("name", ALL)
def test_fixture_numbers_do_not_drift(name):
    c = R.reference(name)
    print(f"case {name}: cond(K_uu) {c['cond_kuu']:.3e} cond(S) {c['cond_S']:.1f} max tol/|logpdf| {(c['tol'] / np.abs(c['lp'])).max():.2e} "
          f"logpdf in [{c['lp'].min():.1f}, {c['lp'].max():.1f}]")
    assert 4e5 <= c["cond_kuu"] <= 8e7
    assert 150 <= c["cond_S"] <= 550
    assert np.all(c["tol"] <= 5e-5 * np.abs(c["lp"]))
    unshifted = R.node_moments(c["X"], c["wts"], c["start"], c["lp"], shifted=False)
    finite = all(np.all(np.isfinite(u)) for u in unshifted)
    if name == "e":
        assert c["lp"].max() > R.LOG_DBL_MAX and not finite             # the reference's exp overflows: NaN moments
        assert all(np.all(np.isfinite(c[k])) for k in ("log_norm", "mean", "cov"))
    else:
        assert finite
        # where nothing overflows the shift changes nothing beyond rounding
        for u, k, b in zip(unshifted, ("log_norm", "mean", "cov"), c["bounds"]):
            assert np.all(np.abs(u - c[k]).reshape(len(b), -1).max(axis=1) <= b), k


# ------------------------------------------------------------------------------------------------
# 3. the checks see the faults
def _ratio(err, bound):
    err = np.where(np.isfinite(err), err, np.inf)
    return float(np.max(err / bound))


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("fault", ["zero_y", "drop_tile"])
def test_logpdf_check_sees_a_faulty_closure(name, fault):
    c = R.reference(name)
    lp_bad, _, _ = R.logpdf_and_bound(R.make_case(name), fault=fault)
    gap = _ratio(np.abs(lp_bad - c["lp"]), c["tol"])
    print(f"case {name} fault {fault}: moves logpdf by {gap:.3g} x its bound")
    assert gap >= 100


def test_moment_checks_see_the_unshifted_exp_in_case_e():
    c = R.reference("e")
    bad = R.node_moments(c["X"], c["wts"], c["start"], c["lp"], shifted=False)
    for u, k, b in zip(bad, ("log_norm", "mean", "cov"), c["bounds"]):
        gap = _ratio(np.abs(u - c[k]).reshape(len(b), -1).max(axis=1), b)
        print(f"case e unshifted exp: moves {k} by {gap:.3g} x its bound")
        assert gap >= 100


def test_moment_checks_see_moments_about_the_old_mean():
    """cov taken about the left message's mean instead of the new one (a fault the per-node kernel could have)."""
    c = R.reference("a")
    X, w, st = c["X"], c["wts"], c["start"]
    worst = 0.0
    for t in range(c["nodes"]):
        sl = slice(st[t], st[t + 1])
        g = w[sl] * np.exp(c["lp"][sl] - c["lp"][sl].max())
        d = X[sl] - c["means"][t]
        bad = (d * g[:, None]).T @ d / g.sum()
        worst = max(worst, np.abs(bad - c["cov"][t]).max() / c["bounds"][2][t])
    assert worst >= 100


# ------------------------------------------------------------------------------------------------
# 4. SGPDevice.in_message: packing and layout, through a recording library
class RecordingLib:
    def __init__(self):
        self.calls = []

    def sgp_in_message(self, h, X, n, node_start, n_nodes, y_mean, weights, mu_v, Sigma_v, logpdf, log_norm, mean, cov):
        def arr(p, count):
            return None if p is None else np.ctypeslib.as_array(p, shape=(count,)).copy()
        D, d_out, Q = self.D, self.d_out, self.Q
        self.calls.append(dict(n=n, n_nodes=n_nodes, X=arr(X, n * D), start=np.ctypeslib.as_array(node_start, shape=(n_nodes + 1,)).copy(),
                               y=arr(y_mean, n_nodes * d_out), w=arr(weights, n), mu=arr(mu_v, Q), S=arr(Sigma_v, Q * Q),
                               outs=(logpdf is not None, log_norm is not None, mean is not None, cov is not None)))
        np.ctypeslib.as_array(logpdf, shape=(n,))[:] = np.arange(n)
        if weights is not None:
            np.ctypeslib.as_array(log_norm, shape=(n_nodes,))[:] = 100 + np.arange(n_nodes)
            np.ctypeslib.as_array(mean, shape=(n_nodes * D,))[:] = np.arange(n_nodes * D)                 # D x n_nodes column-major
            np.ctypeslib.as_array(cov, shape=(n_nodes * D * D,))[:] = np.arange(n_nodes * D * D)
        return 0


def bare_device(D, d_out, M):
    dev = object.__new__(SGPDevice)
    dev._lib = RecordingLib()
    dev._lib.D, dev._lib.d_out, dev._lib.Q = D, d_out, M * d_out
    dev._h = C.c_void_p(1)
    dev.D, dev.d_out, dev.M, dev.Q = D, d_out, M, M * d_out
    dev._check = lambda rc, what: None
    return dev


def test_device_in_message_packs_the_abi_layout():
    D, d_out, M = 3, 2, 4
    dev = bare_device(D, d_out, M)
    rng = np.random.default_rng(0)
    X = rng.normal(size=(6, D))
    Y = rng.normal(size=(2, d_out))
    w = rng.uniform(size=6)
    mu = rng.normal(size=M * d_out)
    Sig = rng.normal(size=(M * d_out, M * d_out))
    lp, log_norm, mean, cov = dev.in_message(np.asfortranarray(X), [0, 4, 6], Y, w, mu, Sig)
    call = dev._lib.calls[-1]
    assert (call["n"], call["n_nodes"]) == (6, 2) and call["start"].dtype == np.int64 and list(call["start"]) == [0, 4, 6]
    assert np.array_equal(call["X"], X.ravel())                          # D x n column-major: one point after another
    assert np.array_equal(call["y"], Y.T.ravel())                        # n_nodes x d_out column-major
    assert np.array_equal(call["w"], w) and np.array_equal(call["mu"], mu)
    assert np.array_equal(call["S"], Sig.T.ravel())                      # Q x Q column-major
    assert call["outs"] == (True, True, True, True)
    assert np.array_equal(lp, np.arange(6)) and np.array_equal(log_norm, [100, 101])
    assert np.array_equal(mean, np.arange(2 * D).reshape(2, D))          # node t: entries t D .. of the D x n_nodes output
    assert np.array_equal(cov, np.arange(2 * D * D).reshape(2, D, D))
    # without weights: logpdf alone, no moment outputs passed; the handle's own q(v)
    out = dev.in_message(X, [0, 4, 6], Y)
    call = dev._lib.calls[-1]
    assert isinstance(out, np.ndarray) and out.shape == (6,)
    assert call["w"] is None and call["mu"] is None and call["S"] is None and call["outs"] == (True, False, False, False)
    with pytest.raises(ValueError):
        dev.in_message(X, [0, 4, 6], Y, w, mu, None)
    with pytest.raises(ValueError):
        dev.in_message(X, [0, 4, 6], Y[:1], w)                            # one row of y per node


# ------------------------------------------------------------------------------------------------
# 5. the node mirrors: one engine call, the reference's NaN fallback
class Engine:
    """The SGPDevice interface `marginal_in_batch` uses; closure values are a known function of the point."""

    def __init__(self, d_out, logpdf_of):
        self.n_max, self.d_out, self.logpdf_of, self.calls, self.noise = 10 ** 6, d_out, logpdf_of, [], None

    def set_inducing(self, Xu):
        pass

    def set_kernel(self, sigma2, ell, jitter=0.0, family="se"):
        self.kernel = (sigma2, np.asarray(ell), jitter, family)

    def set_noise(self, W, E_log_w=None):
        self.noise = np.atleast_2d(np.asarray(W, dtype=np.float64))

    def close(self):
        pass

    def in_message(self, X, node_start, y_mean, weights=None, mu_v=None, Sigma_v=None):
        X, st = np.asarray(X), np.asarray(node_start)
        self.calls.append(dict(X=X, start=st, y=np.asarray(y_mean), w=weights, mu_v=mu_v, Sigma_v=Sigma_v))
        lp = np.concatenate([self.logpdf_of(t, X[st[t]:st[t + 1]]) for t in range(len(st) - 1)])
        mom = R.node_moments(X, np.asarray(weights), st, lp)
        return (lp,) + mom


def test_multi_marginal_in_batch_is_one_call_with_the_reference_fallback():
    D, d_out, T = 2, 2, 4
    shift = np.array([0.0, 800.0, -2000.0, 3.0])                          # node 1 overflows exp, node 2 underflows everywhere

    def logpdf_of(t, x):
        return shift[t] - 0.5 * np.sum((x - 0.3) ** 2, axis=1)
    meta = MultiSGPMeta(None, np.zeros((5, D)), None, None, None, None, SEARDKernel(), jitter=1e-7)
    meta.engine = Engine(d_out, logpdf_of)
    rng = np.random.default_rng(1)
    lefts = [MvNormalMeanCovariance(rng.normal(size=D), 0.1 * np.eye(D) + 0.02) for _ in range(T)]
    q_outs = [PointMass(rng.normal(size=d_out)) for _ in range(T)]
    q_v = MvNormalMeanCovariance(np.arange(10.0), np.eye(10))
    Wbar = np.array([[2.0, 0.3], [0.3, 1.5]])
    theta = PointMass(np.array([0.7, 1.1, 1.3]))
    out = MS.marginal_in_batch(q_outs, lefts, q_v, PointMass(Wbar), theta, meta)
    assert len(meta.engine.calls) == 1
    call = meta.engine.calls[0]
    pw = [srcubature().points_weights(*q.mean_cov()) for q in lefts]
    assert np.array_equal(call["X"], np.concatenate([p for p, _ in pw])) and np.array_equal(call["w"], np.concatenate([w for _, w in pw]))
    assert list(call["start"]) == [0, 5, 10, 15, 20]
    assert np.array_equal(call["y"], np.stack([q.mean() for q in q_outs]))
    assert np.array_equal(call["mu_v"], q_v.m) and np.array_equal(call["Sigma_v"], q_v.S)
    assert np.array_equal(meta.engine.noise, Wbar) and meta.engine.kernel[0] == 0.7 and meta.engine.kernel[2] == 1e-7
    assert out[1] is lefts[1] and out[2] is lefts[2]                      # the reference's NaN -> the left message
    for t in (0, 3):
        _, m, c = U.shifted_moments(pw[t][0], pw[t][1], logpdf_of(t, pw[t][0]))
        assert isinstance(out[t], MvNormalMeanCovariance)
        np.testing.assert_allclose(out[t].m, m, rtol=1e-13)
        np.testing.assert_allclose(out[t].S, c, rtol=1e-12, atol=1e-16)
    # reference_fallback=False: the shifted moments everywhere -- they do not depend on the shift
    out2 = MS.marginal_in_batch(q_outs, lefts, q_v, PointMass(Wbar), theta, meta, reference_fallback=False)
    for t in (1, 2):
        _, m, c = U.shifted_moments(pw[t][0], pw[t][1], logpdf_of(t, pw[t][0]) - shift[t])
        np.testing.assert_allclose(out2[t].m, m, rtol=1e-12)
        np.testing.assert_allclose(out2[t].S, c, rtol=1e-11, atol=1e-16)


def test_multi_prod_logpdf_device_and_host_paths():
    D, d_out = 2, 2

    def logpdf_of(t, x):
        return 1.0 - 0.5 * np.sum((x + 0.2) ** 2, axis=1)
    meta = MultiSGPMeta(None, np.zeros((5, D)), None, None, None, None, SEARDKernel())
    meta.engine = Engine(d_out, logpdf_of)
    left = MvNormalMeanCovariance(np.array([0.1, -0.4]), np.array([[0.2, 0.05], [0.05, 0.1]]))
    closure = U.LogPdfClosure(lambda x: 0.0, multivariate=True)
    closure.in_node = (PointMass(np.array([0.3, 0.4])), MvNormalMeanCovariance(np.zeros(10), np.eye(10)), PointMass(np.eye(2)),
                       PointMass(np.array([1.0, 1.0, 1.0])), meta)
    got = MS.prod_logpdf(left, closure)                                   # the closure's node data: one device call
    assert len(meta.engine.calls) == 1 and list(meta.engine.calls[0]["start"]) == [0, 5]
    plain = U.LogPdfClosure(lambda x: float(logpdf_of(0, np.atleast_2d(x))[0]), multivariate=True)
    host = MS.prod_logpdf(left, plain)                                    # any other closure: host moments
    assert len(meta.engine.calls) == 1
    np.testing.assert_allclose(got.m, host.m, rtol=1e-13)
    np.testing.assert_allclose(got.S, host.S, rtol=1e-12)
    # the reference's arithmetic (MultiSGPnode.jl:37-44), unshifted
    pts, wts = srcubature().points_weights(left.m, left.S)
    g = wts * np.exp(logpdf_of(0, pts))
    m = g @ pts / g.sum()
    np.testing.assert_allclose(host.m, m, rtol=1e-13)
    np.testing.assert_allclose(host.S, ((pts - m) * g[:, None]).T @ (pts - m) / g.sum(), rtol=1e-12)
    assert MS.prod_logpdf(left, U.LogPdfClosure(lambda x: 900.0, multivariate=True)) is left
    assert MS.prod_logpdf(left, U.LogPdfClosure(lambda x: -900.0, multivariate=True)) is left


def test_uni_marginal_in_batch_uses_gauss_hermite_and_pads_the_variance():
    shift = np.array([0.5, 1000.0, -1.0])

    def logpdf_of(t, x):
        return shift[t] - 0.5 * (x[:, 0] - 0.2) ** 2 / 0.3
    meta = UniSGPMeta(None, np.zeros((5, 1)), None, None, None, None, SEARDKernel(), None, 0, 5, jitter=1e-6)
    meta.engine = Engine(1, logpdf_of)
    meta._batch["inducing_set"] = True
    lefts = [NormalMeanVariance(0.1, 0.2), NormalMeanVariance(-0.3, 0.1), NormalMeanVariance(0.6, 0.4)]
    q_outs = [PointMass(0.4), PointMass(-0.2), PointMass(1.0)]
    q_v = MvNormalMeanCovariance(np.arange(5.0), np.eye(5))
    out = U.marginal_in_batch(q_outs, lefts, q_v, PointMass(4.0), PointMass(np.array([0.9, 0.7])), meta)
    assert len(meta.engine.calls) == 1
    call = meta.engine.calls[0]
    assert list(call["start"]) == [0, 21, 42, 63] and call["X"].shape == (63, 1) and call["y"].shape == (3, 1)
    assert meta.engine.noise[0, 0] == 4.0
    assert out[1] is lefts[1]
    for t in (0, 2):
        assert isinstance(out[t], NormalMeanVariance)
        # what the existing one-node product returns for the same closure (both add 1e-6 to the variance)
        one = U.prod_logpdf(lefts[t], U.LogPdfClosure(lambda x, t=t: logpdf_of(t, np.asarray(x).reshape(-1, 1))))
        assert out[t].mean() == pytest.approx(one.mean(), rel=1e-12) and out[t].var() == pytest.approx(one.var(), rel=1e-10)
    out2 = U.marginal_in_batch(q_outs, lefts, q_v, PointMass(4.0), PointMass(np.array([0.9, 0.7])), meta, reference_fallback=False)
    assert isinstance(out2[1], NormalMeanVariance) and np.isfinite(out2[1].mean())



# ------------------------------------------------------------------------------------------------
# 6. the shape cases of tests/test_gpu_in_message_shapes.py: the vectorised restatement, drift guards, the mean-rounding term,
#    zero weights, and the faults the comparisons must see
SHAPES = sorted(R.SHAPE_CASES)


@pytest.mark.parametrize("name", ALL)
def test_vectorised_restatement_is_the_oracle_closure(name):
    """vector_logpdf against O.multi_rule_in_logpdf on cases a-f.  The linear and the S term, closure value minus the closure's
    own Q_ff term (the same sum(Kinv .* k k'), same order): 1e-12 relative.  The Q_ff term through Cholesky solves and through
    the explicit inverse differ by the inverse's conditioning error, which no order of summation removes (2.9e-8 of logpdf in
    case c): it is held to the model's own term for it, 50 eps 1/2 tr(W) cond(K_uu) sigma2."""
    c, cc = R.reference(name), R.make_case(name)
    v = R.vector_logpdf(cc)
    with R.oracle_family(cc["family"]):
        Kinv = O.cholinv(O.kernelmatrix(cc["sigma2"], cc["ell"], cc["Xu"]) + cc["jitter"] * np.eye(cc["M"]))
        K = O.kernelmatrix(cc["sigma2"], cc["ell"], cc["Xu"], cc["X"])
    trW = np.trace(cc["W"])
    qff = np.array([-0.5 * trW * (cc["sigma2"] - np.sum(Kinv * np.outer(k, k))) for k in K.T])
    rest_closure = c["lp"] - qff
    A = np.linalg.solve(np.linalg.cholesky(kuu_of(cc)), K)
    qff_chol = -0.5 * trW * (cc["sigma2"] - np.sum(A * A, axis=0))
    rest_vector = v["lp"] - qff_chol
    rel = float(np.max(np.abs(rest_vector - rest_closure) / np.maximum(np.abs(rest_closure), np.abs(qff))))
    q_ratio = float(np.max(np.abs(v["lp"] - c["lp"])) / (50 * R.EPS * 0.5 * trW * c["cond_kuu"] * cc["sigma2"]))
    print(f"case {name}: linear and S terms differ by {rel:.2e} relative, logpdf by {q_ratio:.3g} x the Q_ff term of the bound")
    assert rel <= 1e-12
    assert q_ratio <= 1.0


def kuu_of(cc):
    with R.oracle_family(cc["family"]):
        return O.kernelmatrix(cc["sigma2"], cc["ell"], cc["Xu"]) + cc["jitter"] * np.eye(cc["M"])


def test_shape_case_shapes():
    for name in SHAPES:
        c, k = R.shape_reference(name), R.SHAPE_CASES[name]
        assert (c["M"], c["D"], c["d_out"], c["family"]) == (k["M"], k["D"], k["d_out"], k["family"])
        assert list(np.diff(c["start"])) == list(k["sizes"]) and c["X"].shape == (sum(k["sizes"]), k["D"])
        assert c["Sigma_v"].shape == (k["M"] * k["d_out"],) * 2 and np.array_equal(c["Sigma_v"], c["Sigma_v"].T)
    assert [R.SHAPE_CASES[f"dim{D}"]["D"] for D in R.DIMS] == [5, 7, 9, 16, 31, 32]
    assert R.DIM_SIZES == [1, 64, 65, 129, 200, 3] and R.LIMIT_SIZES == [1, 70, 9]
    many = R.shape_reference("many")
    assert many["nodes"] == 1001 and len(many["X"]) == 2001 and (many["nodes"] + 3) // 4 == 251 and many["nodes"] % 4 == 1
    assert (R.SHAPE_CASES["limit1"]["M"], R.SHAPE_CASES["limit4"]["M"] * 4) == (4032, 4032)
    for D in R.DIMS:                                                       # isotropic: one lengthscale goes to the device
        assert len(R.shape_reference(f"dim{D}iso")["ell_dev"]) == 1 and len(R.shape_reference(f"dim{D}")["ell_dev"]) == D
        assert R.shape_reference(f"dim{D}")["ell"].argmin() == D - 1 and len(set(R.shape_reference(f"dim{D}")["ell"])) == D
    for fam in R.FAMILIES:                                                 # five coincident and five near-coincident points
        c = R.shape_reference(f"{fam}x2")
        p = c["start"][1]
        assert np.array_equal(c["X"][p:p + 5], c["Xu"][:5])
        d = np.linalg.norm(c["X"][p + 5:p + 10] - c["Xu"][5:10], axis=1)
        assert np.all((d > 0) & (d < 1e-8))


@pytest.mark.parametrize("name", SHAPES)
def test_shape_case_numbers_do_not_drift(name):
    c = R.shape_reference(name)
    rel = float((c["tol"] / np.maximum(np.abs(c["lp"]), 1.0)).max())
    print(f"case {name}: cond(K_uu) {c['cond_kuu']:.3e} cond(S) {c['cond_S']:.1f} max tol/max(|logpdf|, 1) {rel:.2e} "
          f"logpdf in [{c['lp'].min():.1f}, {c['lp'].max():.1f}]")
    assert all(np.all(np.isfinite(c[k])) for k in ("lp", "tol", "log_norm", "mean", "cov"))
    if name.startswith("limit"):                                           # 4032 / 1008 inducing inputs in a 2-D box, jitter 1e-6
        assert 5e7 <= c["cond_kuu"] <= 2e9 and 1e3 <= c["cond_S"] <= 1e5
    elif name.startswith("w_") or c["D"] < 5:                              # the ELL table's lengthscales, jitter 1e-8
        assert 1.0 <= c["cond_kuu"] <= 8e7 and 1.0 <= c["cond_S"] <= 800
    else:                                                                  # sqrt(D)-scaled lengthscales: K_uu far from singular
        assert 10 <= c["cond_kuu"] <= 5e4 and 50 <= c["cond_S"] <= 800
    assert rel <= 5e-5
    K = R.kernel_of(c)(c["sigma2"], c["ell"], c["Xu"], c["X"])
    if c["M"] > 1:
        assert float(np.median(K.max(axis=0))) > 1e-3                      # kernel values do not collapse


@pytest.mark.parametrize("name", SHAPES)
def test_mean_rounding_term_covers_the_kernels_summation_order(name):
    """The kernel's order of sums in float64 against mpmath on the reference's own logpdf: that alone stays within the added
    term (mean: m_term; cov: m_term^2 + the model's 1e-13 max |cov|; log_norm: the model's 1e-13 |log_norm|), and so does the
    NumPy reference.  Without the term a one-point node's bound is 0 and its cov ~ 5e-32."""
    c = R.shape_reference(name)
    args = (c["X"], c["wts"], c["start"], c["lp"])
    exact = R.mp_moments(*args)
    m = R.mean_rounding_term(c["X"], c["wts"], c["start"])
    allowed = (1e-13 * np.abs(exact[0]), m, m * m + 1e-13 * np.abs(exact[2]).reshape(len(m), -1).max(axis=1))
    worst = 0.0
    for got in (R.kernel_order_moments(*args), (c["log_norm"], c["mean"], c["cov"])):
        for g, e, b in zip(got, exact, allowed):
            worst = max(worst, float(np.max(np.abs(g - e).reshape(len(m), -1).max(axis=1) / b)))
    print(f"case {name}: summation order alone / mean-rounding term {worst:.3g}")
    assert worst <= 0.5                                                    # (the term holds a factor 2 for the reference's rounding)


def test_zero_weight_points_take_no_part():
    """The moments of a node with zero-weight points are those over its positively weighted points, the shift taken over
    those; where the largest logpdf lies 850 above them on a zero-weight point the all-points shift gives NaN."""
    for name in ("w_some_zero", "w_top_zero_near", "w_top_zero_far"):
        c = R.shape_reference(name)
        X, w, st, lp = c["X"], c["wts"], c["start"], c["lp"]
        assert np.count_nonzero(w[st[0]:st[1]] == 0) == 4
        keep = w > 0
        st_pos = np.concatenate([[0], np.cumsum([np.count_nonzero(keep[st[t]:st[t + 1]]) for t in range(c["nodes"])])])
        for a, b in zip(R.node_moments(X[keep], w[keep], st_pos, lp[keep]), (c["log_norm"], c["mean"], c["cov"])):
            assert np.array_equal(a, b)
        assert all(np.all(np.isfinite(c[k])) for k in ("log_norm", "mean", "cov"))
        all_points = R.node_moments(X, w, st, lp)
        if name == "w_some_zero":
            continue
        zero, pos = lp[st[2]:st[2] + 3], lp[st[2] + 3:st[3]]
        assert np.all(w[st[2]:st[2] + 3] == 0) and np.all(w[st[2] + 3:st[3]] > 0)
        gap, spread = zero.max() - pos.max(), zero.max() - pos.min()
        print(f"case {name}: largest zero-weight logpdf {gap:.1f} above the largest positively weighted one, {spread:.1f} above the smallest")
        if name == "w_top_zero_near":
            assert 299 <= gap <= 301 and spread < 700 and np.isfinite(all_points[0][2])
            for a, b, bound in zip(all_points, (c["log_norm"], c["mean"], c["cov"]), c["bounds"]):
                assert np.max(np.abs(a[2] - b[2])) <= bound[2]             # the all-points shift is still within bound here
        else:
            assert 849 <= gap <= 851 and not np.isfinite(all_points[0][2]) and np.all(np.isnan(all_points[1][2]))


def _fault_gap(c, lp=None, moments_from=None):
    """Largest error / bound over the compared outputs when the closure values become `lp` (moments follow) or the moments are
    taken by moments_from(lp) instead."""
    lp = c["lp"] if lp is None else lp
    mom = R.shape_node_moments(c["X"], c["wts"], c["start"], lp) if moments_from is None else moments_from(lp)
    return max(R.worst_ratios(c, lp, *mom).values())


def _with_ell(c, ell):
    lp = R.vector_logpdf(dict(c, ell=ell))["lp"]
    return lp + (c["lp"] - R.vector_logpdf(c)["lp"])                       # (the fault's shift, on the reference's own values)


FAULTS = ["drop_last_dim", "drop_dims_from_8", "swap_lengthscales", "se_for_matern", "lost_lane_round", "node_start_shifted",
          "sigma_block_stride_mp", "drop_last_yw_row"]


@pytest.mark.parametrize("fault", FAULTS)
def test_shape_checks_see_the_faults(fault):
    """Each fault a kernel on this path could have, applied to the NumPy reference on every case it can occur in, moves at least
    one compared output by >= 100 x its bound."""
    gaps = {}
    for name in SHAPES:
        k = R.SHAPE_CASES[name]
        if name.startswith("limit"):
            continue                                                       # (the limit cases' paths are the small cases' paths)
        c = R.shape_reference(name)
        D, M, d_out, st = c["D"], c["M"], c["d_out"], c["start"]
        if fault == "drop_last_dim" and name.startswith("dim"):
            e = c["ell"].copy(); e[D - 1] = np.inf
            gaps[name] = _fault_gap(c, _with_ell(c, e))
        elif fault == "drop_dims_from_8" and name.startswith("dim") and D > 8:
            e = c["ell"].copy(); e[8:] = np.inf
            gaps[name] = _fault_gap(c, _with_ell(c, e))
        elif fault == "swap_lengthscales" and name.startswith("dim") and not k["iso"]:
            e = c["ell"].copy(); e[[0, D - 1]] = e[[D - 1, 0]]
            gaps[name] = _fault_gap(c, _with_ell(c, e))
        elif fault == "se_for_matern" and k["family"] != "se":
            shift = R.vector_logpdf(dict(c, family="se"))["lp"] - R.vector_logpdf(c)["lp"]
            gaps[name] = _fault_gap(c, c["lp"] + shift)
        elif fault == "lost_lane_round" and max(k["sizes"]) > 128:
            w = c["wts"].copy()
            for t in range(c["nodes"]):
                w[st[t] + 128:st[t + 1]] = 0.0                             # the points 128.. of a node never summed
            gaps[name] = _fault_gap(c, moments_from=lambda lp: R.shape_node_moments(c["X"], w, st, lp))
        elif fault == "node_start_shifted" and (name.startswith("dim") or name == "many"):
            def shifted(lp):
                mom = R.shape_node_moments(c["X"], c["wts"], st, lp)
                return tuple(np.roll(m, -1, axis=0) for m in mom)          # node t from the points of node t + 1
            gaps[name] = _fault_gap(c, moments_from=shifted)
        elif fault == "sigma_block_stride_mp" and name.startswith("ragged") and M % 64:
            bad = R.padded_blocks(c["Sigma_v"], M, d_out, (M + 63) // 64 * 64)
            assert np.array_equal(R.padded_blocks(c["Sigma_v"], M, d_out, M), c["Sigma_v"])
            shift = R.vector_logpdf(c, Sigma_v=bad)["lp"] - R.vector_logpdf(c)["lp"]
            gaps[name] = _fault_gap(c, c["lp"] + shift)
        elif fault == "drop_last_yw_row" and d_out > 1 and not name.startswith(("dim", "w_")):
            yw = c["Y"] @ c["W"]
            yw[:, -1] = 0.0
            shift = R.vector_logpdf(c, yw=yw)["lp"] - R.vector_logpdf(c)["lp"]
            gaps[name] = _fault_gap(c, c["lp"] + shift)
    assert gaps
    worst = min(gaps, key=gaps.get)
    print(f"fault {fault}: smallest gap {gaps[worst]:.3g} x its bound (case {worst}, {len(gaps)} cases)")
    assert gaps[worst] >= 100, gaps


def test_shifted_moments_host_mirror_ignores_zero_weights():
    c = R.shape_reference("w_top_zero_far")
    st = c["start"]
    sl = slice(st[2], st[3])
    ln, m, S = U.shifted_moments(c["X"][sl], c["wts"][sl], c["lp"][sl])
    assert np.isfinite(ln) and abs(ln - c["log_norm"][2]) <= c["bounds"][0][2]
    assert np.max(np.abs(m - c["mean"][2])) <= c["bounds"][1][2] and np.max(np.abs(S - c["cov"][2])) <= c["bounds"][2][2]
