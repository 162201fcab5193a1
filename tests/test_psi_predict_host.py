"""The closed-form prediction at Gaussian inputs, without a GPU: the NumPy restatement (tests/psi_predict_ref.py) against a tensor
Gauss-Hermite rule over the plain per-point predictive and the law of total variance; its S = 0 and rank-1 limits; definiteness; the
three injected faults; and the entry point's boundary (header, export, argument types, kernels in the built library).

Bound: 1e-10 of the magnitudes `predict` returns.  The 40-node rule is converged there for ell >= 0.5 and |S| <= 0.1: the integrands are
Gaussians in x no narrower than ell / sqrt(2) under a density no wider than sqrt(0.1)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import psi_predict_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2, JITTER, TOL = 0.9, 1e-8, 1e-10


def problem(D, d_out, M=7, T=3, seed=0, cov="full"):
    rng = np.random.default_rng(100 * D + 10 * d_out + seed)
    Xu = np.stack([rng.permutation(np.linspace(-1.5, 1.5, M)) for _ in range(D)], axis=1)    # (evenly spread: K_uu well conditioned)
    ell = np.array([0.6, 0.9])[:D]
    mean = rng.uniform(-1.2, 1.2, (T, D))
    A = rng.normal(size=(T, D, D))
    if cov == "rank1":
        A[:, :, 1:] = 0.0
    S = A @ A.transpose(0, 2, 1)
    S *= 0.09 / np.linalg.norm(S, 2, axis=(1, 2))[:, None, None]       # |S_t|_2 = 0.09 <= 0.1
    B = rng.normal(size=(d_out * M, d_out * M))
    Sig = 0.05 * (B @ B.T / (d_out * M) + 0.1 * np.eye(d_out * M))
    mu = rng.normal(size=d_out * M)
    return dict(D=D, d_out=d_out, M=M, T=T, Xu=Xu, ell=ell, mean=mean, S=S, Sig=Sig, mu=mu, Rv=Sig + np.outer(mu, mu))


def restated(p, cov="S", fault=None):
    S = p["S"] if isinstance(cov, str) else cov
    return R.predict(SIGMA2, p["ell"], p["mean"], S, p["Rv"], p["mu"], p["Xu"], p["d_out"], JITTER, fault=fault)


def quadrature(p, n=40):
    """mean, C_f and cross by the tensor rule over m + chol(S) xi and the law of total variance"""
    x1, w1 = np.polynomial.hermite_e.hermegauss(n)
    w1 = w1 / np.sqrt(2.0 * np.pi)
    D, d = p["D"], p["d_out"]
    xi = np.array(list(itertools.product(x1, repeat=D)))               # (n^D, D)
    w = np.prod(np.array(list(itertools.product(w1, repeat=D))), axis=1)
    out, Cf, cross = np.empty((p["T"], d)), np.empty((p["T"], d, d)), np.empty((p["T"], D, d))
    for t in range(p["T"]):
        L = np.linalg.cholesky(p["S"][t]) if np.linalg.matrix_rank(p["S"][t]) == D else rank_factor(p["S"][t])
        X = p["mean"][t] + xi @ L.T
        m, Cp = R.point_predictive(SIGMA2, p["ell"], X, p["Sig"], p["mu"], p["Xu"], d, JITTER)
        out[t] = w @ m
        Cf[t] = np.einsum("s,sij->ij", w, Cp + m[:, :, None] * m[:, None, :]) - np.outer(out[t], out[t])
        cross[t] = np.einsum("s,sd,si->di", w, X - p["mean"][t], m)
    return out, Cf, cross


def rank_factor(S):
    """A square factor F with F F' = S of a singular positive semi-definite S"""
    w, V = np.linalg.eigh(S)
    return V * np.sqrt(np.maximum(w, 0.0))


def assert_within(label, got, ref, mag, cmag):
    e_m = np.max(np.abs(got[0] - ref[0]) / np.sqrt(np.einsum("tii->ti", mag)))
    e_c = np.max(np.abs(got[1] - ref[1]) / mag)
    e_x = np.max(np.abs(got[2] - ref[2]) / np.where(cmag > 0, cmag, 1.0))
    print(f"psi_predict restatement, {label}: error / magnitude mean {e_m:.3g} C_f {e_c:.3g} cross {e_x:.3g} (bound {TOL:g})")
    return max(e_m, e_c, e_x)


@pytest.mark.parametrize("D,d_out", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_the_restatement_is_the_integral(D, d_out):
    p = problem(D, d_out)
    out, Cf, cross, mag, cmag = restated(p)
    assert assert_within(f"D {D} d_out {d_out} against the 40-node rule", (out, Cf, cross), quadrature(p), mag, cmag) <= TOL


def test_rank_one_covariances():
    p = problem(2, 2, cov="rank1")
    assert np.all(np.linalg.matrix_rank(p["S"]) == 1)
    out, Cf, cross, mag, cmag = restated(p)
    assert assert_within("rank-1 S against the 40-node rule", (out, Cf, cross), quadrature(p), mag, cmag) <= TOL


@pytest.mark.parametrize("D,d_out", [(1, 1), (2, 2)])
def test_without_input_uncertainty_it_is_the_plain_predictive(D, d_out):
    p = problem(D, d_out)
    m, Cp = R.point_predictive(SIGMA2, p["ell"], p["mean"], p["Sig"], p["mu"], p["Xu"], d_out, JITTER)
    for label, cov in (("S = 0", np.zeros_like(p["S"])), ("cov = None", None)):
        out, Cf, cross, mag, cmag = restated(p, cov)
        assert assert_within(label, (out, Cf, cross), (m, Cp, np.zeros_like(cross)), mag, cmag) <= TOL
        assert np.all(cross == 0.0)


def test_every_covariance_is_positive_semi_definite():
    for D, d_out in ((1, 2), (2, 2)):
        p = problem(D, d_out, T=8, seed=3)
        _, Cf, _, mag, _ = restated(p)
        low = np.linalg.eigvalsh(0.5 * (Cf + Cf.transpose(0, 2, 1)))[:, 0]
        print(f"psi_predict restatement, D {D}: smallest eigenvalue of C_f {low.min():.3g}")
        assert np.all(low >= -TOL * mag.max())


@pytest.mark.parametrize("fault", ["keep_mean_sq", "p2_cross", "offdiag_once"])
def test_the_checks_catch_an_injected_fault(fault):
    p = problem(2, 2)
    out, Cf, cross, mag, cmag = restated(p, fault=fault)
    assert assert_within(f"fault {fault}", (out, Cf, cross), quadrature(p), mag, cmag) > 1e4 * TOL


def test_the_entry_point_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    name = "sgp_psi_predict"
    assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
    fn = getattr(_lib.load(), name)
    dp = C.POINTER(C.c_double)
    assert list(fn.argtypes) == [C.c_void_p, dp, dp, C.c_int64, C.c_int32, dp, dp, dp, C.POINTER(C.c_int64)]
    for kernel in (b"k_psi_pred_prep", b"k_psi_pred_weights", b"k_psi2_pred_accumulate", b"k_psi_pred_finish"):
        assert kernel in blob, kernel
    from gaussianprocessnode_amd import SGPDevice, multisgp, train, unisgp
    assert callable(SGPDevice.psi_predict) and callable(train.forecast_gpssm)
    import inspect
    for mod in (multisgp, unisgp):
        assert inspect.signature(mod.predictive).parameters["psi"].default == "cubature"
