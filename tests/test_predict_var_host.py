"""Predictive variances without a GPU: the entry point is declared and exported, and the node mirrors' host logic -- test
points, the law of total variance over cubature points, the noise flag, the probit class probability -- is checked against a
stand-in engine that returns known per-point (mean, variance)."""
import os
import re

import numpy as np
import pytest

from gaussianprocessnode_amd import multisgp as MS
from gaussianprocessnode_amd import unisgp as U
from gaussianprocessnode_amd.cubature import ghcubature, srcubature
from gaussianprocessnode_amd.distributions import (MvNormalMeanCovariance, NormalMeanVariance, PointMass, GammaShapeRate,
                                                   WishartFast)
from gaussianprocessnode_amd.meta import MultiSGPMeta, SEARDKernel, UniSGPMeta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_var_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    assert re.search(r"int\s+sgp_predict_var\s*\(", txt)
    assert re.search(r"#define\s+SGP_PREDICT_NOISE\s+1\b", txt)
    from gaussianprocessnode_amd import _build, _lib
    assert "sgp_predict_var" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "sgp_predict_var")
    assert b"sgp_predict_var" in open(_build.build(), "rb").read()


class StandIn:
    """The SGPDevice interface the mirrors use, with per-point results that are known functions of the test point."""

    def __init__(self, d_out=1):
        self.n_max, self.d_out, self.calls = 10 ** 6, d_out, []
        self.noise = None

    def set_inducing(self, Xu):
        pass

    def set_kernel(self, sigma2, ell, jitter=0.0):
        self.kernel = (sigma2, np.asarray(ell), jitter)

    def set_noise(self, W, E_log_w=None):
        self.noise = np.atleast_2d(np.asarray(W, dtype=np.float64))

    def close(self):
        pass

    @staticmethod
    def latent(X, d_out):
        s = X.sum(axis=1)
        m = np.stack([np.sin(s + o) for o in range(d_out)], axis=1)
        C = np.empty((len(X), d_out, d_out))
        for i in range(d_out):
            for j in range(d_out):
                C[:, i, j] = 0.1 * np.exp(-0.5 * s * s) * (1.0 if i == j else 0.3) + 0.05 * (i == j)
        return m, C

    def predict_var(self, Xstar, mu_v=None, Sigma_v=None, noise=False):
        X = np.asarray(Xstar, dtype=np.float64)
        self.calls.append(dict(X=X, mu_v=mu_v, Sigma_v=Sigma_v, noise=noise))
        m, C = self.latent(X, self.d_out)
        if noise:
            C = C + np.linalg.inv(self.noise)
        if self.d_out == 1:
            return m[:, 0], C[:, 0, 0]
        return m, C


def uni_meta(D=1, method=None):
    meta = UniSGPMeta(method, np.zeros((5, D)), None, None, None, None, SEARDKernel(), None, 0, 5)
    meta.engine = StandIn()
    meta._batch["inducing_set"] = True
    return meta


def qv(Q=5):
    return MvNormalMeanCovariance(np.arange(Q, dtype=float), np.eye(Q))


def test_uni_predictive_points_and_noise_flag():
    meta = uni_meta(D=2)
    X = np.array([[0.1, 0.2], [0.5, -0.3], [1.0, 1.0]])
    theta = PointMass(np.array([0.7, 1.1, 1.3]))
    m, v = U.predictive(X, qv(), PointMass(4.0), theta, meta, noise=False)
    m_ref, C_ref = StandIn.latent(X, 1)
    assert np.array_equal(m, m_ref[:, 0]) and np.array_equal(v, C_ref[:, 0, 0])
    call = meta.engine.calls[-1]
    assert call["noise"] is False and np.array_equal(call["X"], X)
    assert np.array_equal(call["mu_v"], np.arange(5.0)) and np.array_equal(call["Sigma_v"], np.eye(5))   # the explicit q_v
    assert meta.engine.kernel[0] == 0.7
    m2, v2 = U.predictive(X, qv(), GammaShapeRate(8.0, 2.0), theta, meta, noise=True)
    assert meta.engine.calls[-1]["noise"] is True and meta.engine.noise[0, 0] == 4.0        # mean(q_w) reached the engine
    np.testing.assert_allclose(v2, v + 0.25, rtol=1e-15)
    assert np.array_equal(m2, m)
    mp, vp = U.predictive(PointMass(X[1]), qv(), PointMass(4.0), theta, meta, noise=False)
    assert mp == m[1] and vp == v[1]


def test_uni_predictive_uncertain_input_is_the_total_variance_over_the_cubature():
    method = ghcubature(11)
    meta = uni_meta(D=1, method=method)
    q_in = NormalMeanVariance(0.3, 0.2)
    m, v = U.predictive(q_in, qv(), PointMass(4.0), PointMass(np.array([1.0, 1.0])), meta, noise=True)
    assert len(meta.engine.calls) == 1                                   # one engine call over all cubature points
    pts, wts = method.points_weights(0.3, 0.2)
    ms, Cs = StandIn.latent(np.asarray(pts).reshape(-1, 1), 1)
    vs = Cs[:, 0, 0] + 0.25
    mean = float(np.sum(wts * ms[:, 0]))
    var = float(np.sum(wts * (vs + ms[:, 0] ** 2)) - mean ** 2)
    assert isinstance(m, float) and isinstance(v, float)
    assert m == pytest.approx(mean, rel=1e-14) and v == pytest.approx(var, rel=1e-12)


def test_combine_total_variance_matrix_form():
    rng = np.random.default_rng(0)
    S, d = 7, 3
    w = rng.uniform(0.1, 1.0, S)
    w /= w.sum()
    m = rng.normal(size=(S, d))
    A = rng.normal(size=(S, d, d))
    C = A @ A.transpose(0, 2, 1)
    mean, cov = U.combine_total_variance(w, m, C)
    ref_mean = sum(w[s] * m[s] for s in range(S))
    ref_cov = sum(w[s] * (C[s] + np.outer(m[s], m[s])) for s in range(S)) - np.outer(ref_mean, ref_mean)
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-14)
    np.testing.assert_allclose(cov, ref_cov, rtol=1e-12, atol=1e-14)
    # a law of total variance over one point is that point's own moments
    m1, v1 = U.combine_total_variance(np.ones(1), np.array([0.4]), np.array([0.3]))
    assert m1 == 0.4 and v1 == pytest.approx(0.3, rel=1e-15)


def test_multi_predictive_points_uncertain_input_and_noise():
    d_out = 2
    meta = MultiSGPMeta(srcubature(), np.zeros((4, 2)), None, None, None, None, SEARDKernel())
    meta.engine = StandIn(d_out)
    Wbar = np.array([[3.0, 0.5], [0.5, 2.0]])
    q_w = WishartFast(5.0, 5.0 * np.linalg.inv(Wbar))                  # mean(q_w) = Wbar
    W_used = MS._mean_W(q_w)
    np.testing.assert_allclose(W_used, Wbar, rtol=1e-14)
    theta = PointMass(np.array([0.7, 1.1, 1.3]))
    X = np.array([[0.1, 0.2], [0.5, -0.3]])
    m, C = MS.predictive(X, qv(8), q_w, theta, meta, noise=True)
    m_ref, C_ref = StandIn.latent(X, d_out)
    assert m.shape == (2, d_out) and C.shape == (2, d_out, d_out)
    np.testing.assert_allclose(C, C_ref + np.linalg.inv(W_used), rtol=1e-14)
    assert np.array_equal(meta.engine.noise, W_used) and meta.engine.calls[-1]["noise"] is True
    q_in = MvNormalMeanCovariance(np.array([0.2, -0.1]), np.array([[0.3, 0.05], [0.05, 0.2]]))
    mu, cov = MS.predictive(q_in, qv(8), q_w, theta, meta, noise=False)
    pts, wts = srcubature().points_weights(q_in.m, q_in.S)
    ms, Cs = StandIn.latent(np.asarray(pts), d_out)
    ref_mean = np.einsum("s,si->i", wts, ms)
    ref_cov = np.einsum("s,sij->ij", wts, Cs + ms[:, :, None] * ms[:, None, :]) - np.outer(ref_mean, ref_mean)
    np.testing.assert_allclose(mu, ref_mean, rtol=1e-14)
    np.testing.assert_allclose(cov, ref_cov, rtol=1e-12, atol=1e-15)
    assert meta.engine.calls[-1]["noise"] is False


def test_probit_predictive_matches_ndtr():
    from scipy.special import ndtr
    meta = uni_meta(D=2)
    X = np.array([[0.1, 0.2], [0.5, -0.3], [1.0, 1.0], [-2.0, 0.4]])
    q_w = PointMass(5.0)
    p = U.probit_predictive(X, qv(), q_w, PointMass(np.array([1.0, 1.0, 1.0])), meta)
    m, C = StandIn.latent(X, 1)
    ref = ndtr(m[:, 0] / np.sqrt(1.0 + C[:, 0, 0] + 1.0 / 5.0))
    np.testing.assert_allclose(p, ref, rtol=1e-14)
    assert meta.engine.calls[-1]["noise"] is True
    p1 = U.probit_predictive(PointMass(X[2]), qv(), q_w, PointMass(np.array([1.0, 1.0, 1.0])), meta)
    assert isinstance(p1, float) and p1 == pytest.approx(ref[2], rel=1e-14)
