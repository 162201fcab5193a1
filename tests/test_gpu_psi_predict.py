"""sgp_psi_predict against the NumPy restatement (tests/psi_predict_ref.py) at the smallest shapes at which each part can go wrong -- see
CASES -- with its determinism, state, failure and refusal contracts, and the Python layer on it (predictive(psi="exact"),
train.forecast_gpssm).

Bounds: VALUE_RTOL of the exact-Psi suites (1e-8) on the magnitudes that cancel -- per entry of C_f
delta_ij (sigma2 + |tr(Kinv Psi2_t)|) + |tr(R^(ij) Psi2_t)| + |mean_i mean_j|, per entry of cross sum_m |mu_m Psi1[m]| |S P_1 (z_m - m)|.
The measured error / bound is printed per case.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import psi_predict_ref as R
from tests import psi_stats_ref as PR
from tests import theta_descend_ref as DR

pytestmark = pytest.mark.gpu

VALUE_RTOL = 1e-8
SIGMA2 = 0.9
JITTER = 1e-8

# name: (d_out, M, D, T, shared lengthscale, cov)
CASES = {
    "smallest_M": (1, 1, 2, 65, False, "full"),
    "single_node": (2, 48, 2, 1, False, "full"),
    "T63": (2, 48, 2, 63, False, "full"),
    "T65": (2, 48, 2, 65, False, "full"),
    "T257": (2, 48, 2, 257, False, "full"),
    "T300": (2, 48, 2, 300, False, "full"),
    "padded_second_tile_D1": (1, 65, 1, 63, True, "full"),
    "shared_ell_D5_dout4": (4, 65, 5, 65, True, "full"),
    "six_tiles": (2, 130, 2, 65, False, "full"),
    "D8": (1, 65, 8, 63, False, "full"),
    "D9": (2, 65, 9, 63, False, "full"),
    "D32": (3, 65, 32, 63, False, "full"),
    "cov_null": (3, 65, 5, 65, False, "null"),
    "cov_zero": (3, 65, 5, 65, False, "zero"),
    "cov_rank1": (3, 65, 5, 65, False, "rank1"),
}


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


# (M, D): lengthscale over sqrt(D) where the default would leave K_uu ill conditioned (it stays below 1e5)
SCALES = {(65, 1): 0.06, (130, 2): 0.2, (64, 2): 0.3, (128, 2): 0.15, (17, 1): 0.2}


@functools.lru_cache(maxsize=None)
def case(name):
    """The three cov_* cases share one seed, so that they differ in the covariances alone."""
    seed_name = "cov_null" if name.startswith("cov_") else name
    return problem(name, CASES[name], 1700 + sorted(CASES).index(seed_name))


def problem(name, spec, seed, subset=None):
    """The inputs of a case and the reference's results (computed once; arrays not to be written to), built as
    tests/test_gpu_psi_in.py builds its cases: q(v) is one VMP update from an isotropic prior over the exact statistics.
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
    A = rng.normal(size=(T, D, D)) * 0.3 * ell.mean() / np.sqrt(D)
    a = rng.normal(size=(T, D, 1)) * 0.3 * ell.mean()
    S_full = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(D)
    S = {"full": S_full, "rank1": a @ a.transpose(0, 2, 1), "zero": np.zeros((T, D, D)), "null": None}[cov]
    Y = np.sin(mean @ rng.normal(size=(D, d_out)) / np.sqrt(D) * 2.0) + 0.05 * rng.normal(size=(T, d_out))
    B = rng.normal(size=(d_out, d_out))
    W = 20.0 * (B @ B.T / d_out + np.eye(d_out))
    sel = slice(None) if subset is None else subset
    psi1, psi2 = PR.psi_stats(Xu, SIGMA2, ell, mean[sel], S_full[sel])   # (q(v) from the full covariances in every cov_* case)
    Sig = np.linalg.inv(np.kron(W, psi2) + np.eye(d_out * M) / 50.0)
    Sig = 0.5 * (Sig + Sig.T)
    mu = Sig @ ((psi1.T @ Y[sel]) @ W.T).T.ravel()
    Rv = Sig + np.outer(mu, mu)
    ell_arg = ell[:1] if shared else ell
    out, Cf, cross, mag, cmag = R.predict(SIGMA2, ell_arg, mean[sel], None if S is None else S[sel], Rv, mu, Xu, d_out, JITTER)
    return dict(name=name, d_out=d_out, M=M, D=D, T=T, ell=ell_arg, mean=mean, S=S, W=W, Xu=Xu, mu=mu, Sig=Sig, Rv=Rv,
                out=out, Cf=Cf, cross=cross, mag=mag, cmag=cmag)


def install(dev, c, posterior=True):
    dev.set_inducing(c["Xu"])
    dev.set_kernel(SIGMA2, c["ell"], JITTER)
    dev.set_noise(c["W"])
    if posterior:
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)


def device(G, c, posterior=True):
    dev = G.SGPDevice(max(8, c["T"]), c["M"], c["D"], d_out=c["d_out"])
    install(dev, c, posterior)
    return dev


def full(C_f, d_out):
    """C_f as (T, d_out, d_out), whatever d_out"""
    return np.asarray(C_f).reshape(-1, d_out, d_out)


def error_over_bound(Cf, cross, Cf_ref, cross_ref, mag, cmag):
    def over(got, ref, mag):                 # where the magnitude is exactly zero (nothing to cancel) equality is demanded
        safe = np.where(mag > 0, mag, 1.0)
        return float(np.max(np.where(mag > 0, np.abs(got - ref) / (VALUE_RTOL * safe), np.where(got == ref, 0.0, np.inf))))
    return over(Cf, Cf_ref, mag), over(cross, cross_ref, cmag)


def assert_close(label, Cf, cross, c, ref=None):
    Cf_ref, cross_ref, mag, cmag = ref if ref is not None else (c["Cf"], c["cross"], c["mag"], c["cmag"])
    ec, ex = error_over_bound(full(Cf, c["d_out"]), cross, Cf_ref, cross_ref, mag, cmag)
    print(f"psi_predict {label}: C_f error / bound {ec:.3g}; cross error / bound {ex:.3g} (bound = {VALUE_RTOL:g} x magnitude)")
    assert ec <= 1.0
    assert ex <= 1.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_moments_match_the_restatement(G, name):
    c = case(name)
    T, d, D = c["T"], c["d_out"], c["D"]
    with device(G, c) as dev:
        m, Cf, cross = dev.psi_predict(c["mean"], c["S"], want_cross=True)
        m2, Cf2, cross2 = dev.psi_predict(c["mean"], c["S"], want_cross=True)
        m3, none_C, none_X = dev.psi_predict(c["mean"], c["S"], want_cov=False)
        stats_mean = dev.psi_stats(c["mean"], c["S"], want_psi1=False, want_psi2=False, want_out=True)[2]
    assert m.shape == (T, d) and Cf.shape == ((T,) if d == 1 else (T, d, d)) and cross.shape == (T, D, d)
    assert np.array_equal(m, stats_mean)                                         # bitwise sgp_psi_stats' :out means
    assert np.array_equal(full(Cf, d), full(Cf, d).transpose(0, 2, 1))           # exactly symmetric
    assert np.array_equal(m, m2) and np.array_equal(Cf, Cf2) and np.array_equal(cross, cross2)      # two calls agree bitwise
    assert none_C is None and none_X is None and np.array_equal(m, m3)
    assert np.max(np.abs(m - c["out"]) / np.sqrt(np.einsum("tii->ti", c["mag"]))) <= VALUE_RTOL
    assert_close(name, Cf, cross, c)


def test_without_a_covariance_it_is_predict_var(G):
    c, z = case("cov_null"), case("cov_zero")
    d = c["d_out"]
    with device(G, c) as dev:
        m, Cf, cross = dev.psi_predict(c["mean"], None, want_cross=True)
        mz, Cfz, crossz = dev.psi_predict(z["mean"], z["S"], want_cross=True)
        mp, Cp = dev.predict_var(c["mean"], c["mu"], c["Sig"])
    assert np.all(cross == 0.0) and not np.any(np.signbit(cross))
    for a, b in ((m, mz), (Cf, Cfz), (cross, crossz)):
        assert a.tobytes() == b.tobytes()                                        # S = 0 given is bitwise S = NULL
    assert_close("cov = NULL against sgp_predict_var", Cf, cross, c, (full(Cp, d), np.zeros_like(cross), c["mag"], c["cmag"]))
    assert np.max(np.abs(m - np.reshape(mp, m.shape))) <= VALUE_RTOL * np.sqrt(c["mag"].max())


@pytest.mark.parametrize("name", ["padded_second_tile_D1", "cov_rank1"])
def test_the_noise_flag_adds_the_inverse_of_W(G, name):
    c = case(name)
    d = c["d_out"]
    with device(G, c) as dev:
        _, plain, _ = dev.psi_predict(c["mean"], c["S"])
        _, noisy, _ = dev.psi_predict(c["mean"], c["S"], noise=True)
    Winv = np.linalg.inv(c["W"])
    err = np.max(np.abs(full(noisy, d) - full(plain, d) - Winv) / np.abs(Winv))
    # (the difference of two rounded sums: eps (|C_f| + |W^-1|) / |W^-1| stays below 1e-12 here)
    print(f"psi_predict {name}: noise - plain against inv(W) rel {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", ["T300", "T257"])
def test_the_chunk_size_changes_no_bit(G, name, monkeypatch):
    c = case(name)
    with device(G, c) as dev:
        a = dev.psi_predict(c["mean"], c["S"], want_cross=True)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "64")
    with device(G, c) as dev:
        b = dev.psi_predict(c["mean"], c["S"], want_cross=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_changes_nothing_the_sweep_keeps_and_honours_a_later_posterior(G):
    c = case("T65")
    with device(G, c, posterior=False) as dev:
        dev.set_prior_isotropic(50.0)
        dev.sweep_local_psi(c["mean"], c["S"], np.zeros((c["T"], c["d_out"])) + c["out"])
        dev.sweep_finish()
        mu, Sig, Uv = dev.posterior()
        before = (dev.sweep_kind(), dev.stats(), (mu, Sig, Uv))
        m, Cf, cross = dev.psi_predict(c["mean"], c["S"], want_cross=True)
        after = (dev.sweep_kind(), dev.stats(), dev.posterior())
        assert before[0] == after[0]
        for a, b in zip(before[1] + before[2], after[1] + after[2]):
            assert np.array_equal(a, b)
        ref = R.predict(SIGMA2, c["ell"], c["mean"], c["S"], Sig + np.outer(mu, mu), mu, c["Xu"], c["d_out"], JITTER)
        assert_close("the sweep's own q(v)", Cf, cross, c, ref[1:])
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)              # a later set_posterior is the q(v) of the next call
        m, Cf, cross = dev.psi_predict(c["mean"], c["S"], want_cross=True)
    assert_close("after set_posterior", Cf, cross, c)


def test_an_indefinite_covariance_reports_its_node(G):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = case("T65")
    bad = c["S"].copy()
    bad[40] = -10.0
    bad[3] = -10.0
    with device(G, c) as dev:
        with pytest.raises(G.PosDefException) as ei:
            dev.psi_predict(c["mean"], bad)
        assert ei.value.info == 4 and "node 3" in str(ei.value) and "sgp_psi_predict" in str(ei.value)
        info = (C.c_int64 * 2)()
        m, Sb, out = as_f64(c["mean"]), as_f64(bad), np.empty((c["d_out"], c["T"]))
        rc = dev._lib.sgp_psi_predict(dev._h, ptr(m), ptr(Sb), c["T"], 0, ptr(out), None, None, info)
        assert rc == 4 and list(info) == [0, 4]
        _, Cf, cross = dev.psi_predict(c["mean"], c["S"], want_cross=True)       # the handle is as good as before
    assert_close("after an indefinite node", Cf, cross, c)


def test_a_singular_K_uu_reports_its_minor(G):
    from gaussianprocessnode_amd._lib import as_f64, ptr
    c = case("T63")
    Xu = c["Xu"].copy()
    Xu[17] = Xu[5]                                                              # two equal inducing inputs, jitter 0
    with device(G, c) as dev:
        dev.set_inducing(Xu)
        dev.set_kernel(SIGMA2, c["ell"], 0.0)
        dev.set_posterior(c["mu"], np.linalg.cholesky(c["Rv"]).T)
        mean = as_f64(c["mean"])
        out, Cf, info = np.empty((2, c["T"])), np.empty((c["T"], 2, 2)), (C.c_int64 * 2)()
        rc = dev._lib.sgp_psi_predict(dev._h, ptr(mean), None, c["T"], 0, ptr(out), ptr(Cf), None, info)
        assert rc > 0 and list(info) == [rc, 0]
        assert b"sgp_psi_predict" in dev._lib.sgp_last_error(dev._h) and b"K_uu" in dev._lib.sgp_last_error(dev._h)
        with pytest.raises(G.PosDefException):
            dev.psi_predict(c["mean"], c["S"])
        dev.psi_predict(c["mean"], c["S"], want_cov=False)                      # (the means need no K_uu)


def test_refusals(G):
    from gaussianprocessnode_amd._lib import SGP_PREDICT_NOISE, as_f64, ptr
    c = case("T63")
    mean, S = c["mean"], c["S"]

    def refused(dev, text, *args, **kw):
        with pytest.raises(G.SGPError) as ei:
            dev.psi_predict(*(args or (mean, S)), **kw)
        assert "status -1" in str(ei.value) and "sgp_psi_predict" in str(ei.value) and text in str(ei.value), str(ei.value)

    with G.SGPDevice(64, c["M"], c["D"], d_out=c["d_out"]) as dev:
        refused(dev, "set_inducing and set_kernel first")
        install(dev, c, posterior=False)
        refused(dev, "q(v)")
        install(dev, c)
        nan_mean, inf_cov = mean.copy(), S.copy()
        nan_mean[3, 0], inf_cov[2, 0, 0] = np.nan, np.inf
        refused(dev, "mean must be finite", nan_mean, S)
        refused(dev, "cov must be finite", mean, inf_cov)
        m, Sc, out = as_f64(mean), as_f64(S), np.empty((c["d_out"], c["T"]))
        rc = dev._lib.sgp_psi_predict(dev._h, ptr(m), ptr(Sc), c["T"], 0, None, None, None, None)
        assert rc == -1 and b"sgp_psi_predict: out_mean must not be NULL" in dev._lib.sgp_last_error(dev._h)
        rc = dev._lib.sgp_psi_predict(dev._h, ptr(m), ptr(Sc), c["T"], SGP_PREDICT_NOISE | 8, ptr(out), None, None, None)
        assert rc == -1 and b"sgp_psi_predict: unknown flags" in dev._lib.sgp_last_error(dev._h)
        assert dev._lib.sgp_psi_predict(dev._h, None, None, 0, 0, ptr(out), None, None, None) == 0        # no nodes: nothing done
        dev.set_noise(np.array([[1.0, 2.0], [2.0, 1.0]]))
        refused(dev, "not positive definite", mean, S, noise=True)
        dev.psi_predict(mean, S)                                                # (the noise is only looked at under the flag)
        dev.set_noise(c["W"])
        dev.set_kernel_family("matern32")
        refused(dev, "SGP_KERNEL_SE only")
        dev.set_kernel_family("se")
        dev.set_allreduce(lambda buf, count, stream: 0)
        refused(dev, "all-reduce hook")
        dev.set_allreduce(None)
        dev.psi_predict(mean, S)
    c1 = case("padded_second_tile_D1")
    with device(G, c1) as dev:
        dev.train_begin(c1["mean"], np.zeros(c1["T"]), np.zeros(2))
        with pytest.raises(G.SGPError) as ei:
            dev.psi_predict(c1["mean"], c1["S"])
        assert "status -1" in str(ei.value) and "sgp_psi_predict" in str(ei.value)
        assert "a device-paced training run is open" in str(ei.value)
        dev.train_end()


# ---- the Python layer on top of it ----
def pendulum_model(c):
    """meta, q_v, q_w, q_theta of a case on the pendulum grid, at the case's kernel"""
    from gaussianprocessnode_amd.cubature import srcubature
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel
    meta = MultiSGPMeta(srcubature(), c["Xu"], None, None, None, None, SEARDKernel(), jitter=JITTER)
    return meta, MvNormalMeanCovariance(c["mu"], c["Sig"]), PointMass(c["W"]), PointMass(np.concatenate([[SIGMA2], c["ell"]]))


def close_engines(meta):
    for eng in (meta.engine, getattr(meta, "_aux_engine_out", None)):
        if eng is not None:
            eng.close()


def test_predictive_exact_takes_one_input_and_a_list(G):
    from gaussianprocessnode_amd import multisgp as MS
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
    c = case("T63")
    meta, q_v, q_w, q_theta = pendulum_model(c)
    Winv = np.linalg.inv(c["W"])
    try:
        m1, C1 = MS.predictive(MvNormalMeanCovariance(c["mean"][5], c["S"][5]), q_v, q_w, q_theta, meta, psi="exact")
        qs = [MvNormalMeanCovariance(c["mean"][t], c["S"][t]) for t in range(4)] + [PointMass(c["mean"][4])]
        ml, Cl = MS.predictive(qs, q_v, q_w, q_theta, meta, noise=False, psi="exact")
        ma, Ca = MS.predictive(c["mean"][:3], q_v, q_w, q_theta, meta, noise=False, psi="exact")
        mc, Cc = MS.predictive(c["mean"][:3], q_v, q_w, q_theta, meta, noise=False)
        with pytest.raises(ValueError):
            MS.predictive(qs, q_v, q_w, q_theta, meta, psi="other")
    finally:
        close_engines(meta)
    assert m1.shape == (2,) and C1.shape == (2, 2) and ml.shape == (5, 2) and Cl.shape == (5, 2, 2) and ma.shape == (3, 2)
    assert np.all(np.abs(C1 - Winv - c["Cf"][5]) <= VALUE_RTOL * (c["mag"][5] + np.abs(Winv)))
    assert np.all(np.abs(Cl[:4] - c["Cf"][:4]) <= VALUE_RTOL * c["mag"][:4])
    assert np.all(np.abs(ml[:4] - c["out"][:4]) <= VALUE_RTOL * np.sqrt(c["mag"][:4].max()))
    point = R.predict(SIGMA2, c["ell"], c["mean"][:5], None, c["Rv"], c["mu"], c["Xu"], 2, JITTER)
    assert np.all(np.abs(Cl[4] - point[1][4]) <= VALUE_RTOL * point[3][4])
    assert np.all(np.abs(Ca - point[1][:3]) <= VALUE_RTOL * point[3][:3])
    assert np.all(np.abs(Ca - Cc) <= 2 * VALUE_RTOL * point[3][:3])             # plain points: the cubature route's own answer


def test_predictive_exact_of_the_single_output_node(G):
    from gaussianprocessnode_amd import unisgp as US
    from gaussianprocessnode_amd.distributions import GammaShapeRate, MvNormalMeanCovariance, PointMass
    from gaussianprocessnode_amd.meta import SEARDKernel, UniSGPMeta
    c = case("padded_second_tile_D1")
    meta = UniSGPMeta(None, c["Xu"], None, None, None, None, SEARDKernel(), None, 0, 8, jitter=JITTER)
    q_v, q_theta = MvNormalMeanCovariance(c["mu"], c["Sig"]), PointMass(np.concatenate([[SIGMA2], c["ell"]]))
    w = float(c["W"][0, 0])
    try:
        m, v = US.predictive([MvNormalMeanCovariance(c["mean"][t], c["S"][t]) for t in range(3)], q_v, GammaShapeRate(w, 1.0), q_theta,
                             meta, psi="exact")
        m1, v1 = US.predictive(MvNormalMeanCovariance(c["mean"][1], c["S"][1]), q_v, GammaShapeRate(w, 1.0), q_theta, meta,
                               noise=False, psi="exact")
    finally:
        for eng in (meta.engine, meta._batch.get("aux_engine")):
            if eng is not None:
                eng.close()
    assert m.shape == (3,) and v.shape == (3,) and isinstance(m1, float) and isinstance(v1, float)
    assert np.all(np.abs(v - 1.0 / w - c["Cf"][:3, 0, 0]) <= VALUE_RTOL * (c["mag"][:3, 0, 0] + 1.0 / w))
    assert abs(v1 - c["Cf"][1, 0, 0]) <= VALUE_RTOL * c["mag"][1, 0, 0] and abs(m1 - c["out"][1, 0]) <= VALUE_RTOL * np.sqrt(c["mag"][1, 0, 0])


def test_forecast_rolls_a_batch_of_trajectories(G):
    from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance
    from gaussianprocessnode_amd.train import forecast_gpssm
    c = case("T63")
    meta, q_v, q_w, q_theta = pendulum_model(c)
    B, steps = 3, 4
    q0 = [MvNormalMeanCovariance(c["mean"][t], c["S"][t]) for t in range(B)]
    try:
        means, covs = forecast_gpssm(q0, steps, q_v, q_w, q_theta, meta)
        one_m, one_C = forecast_gpssm(q0[1], 1, q_v, q_w, q_theta, meta, noise=False)
    finally:
        close_engines(meta)
    assert means.shape == (steps, B, 2) and covs.shape == (steps, B, 2, 2) and one_m.shape == (1, 1, 2)
    Winv = np.linalg.inv(c["W"])
    m_in, S_in = c["mean"][:B], c["S"][:B]
    for k in range(steps):                                   # each step against the restatement at the device's own previous output
        out, Cf, _, mag, _ = R.predict(SIGMA2, c["ell"], m_in, S_in, c["Rv"], c["mu"], c["Xu"], 2, JITTER)
        ec = np.max(np.abs(covs[k] - Cf - Winv) / (VALUE_RTOL * (mag + np.abs(Winv))))
        em = np.max(np.abs(means[k] - out) / (VALUE_RTOL * np.sqrt(np.einsum("tii->ti", mag))))
        print(f"forecast_gpssm step {k + 1}: covariance error / bound {ec:.3g}, mean error / bound {em:.3g}")
        assert ec <= 1.0 and em <= 1.0
        np.linalg.cholesky(covs[k])
        m_in, S_in = means[k], covs[k]
    assert np.all(np.abs(one_C[0, 0] - c["Cf"][1]) <= VALUE_RTOL * c["mag"][1])
