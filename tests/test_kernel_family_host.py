"""Kernel families (SGP_KERNEL_SE / MATERN12 / MATERN32 / MATERN52) on the host side, no GPU: the C ABI declares and the binding
exports them, the Matern restatement the GPU tests compare against is pinned to an independent implementation
(sklearn.gaussian_process.kernels.Matern), MaternARDKernel maps theta as SEARDKernel does and its family reaches the engine
from every node mirror and driver, and the GPU tests' fixtures tell the four families apart.

The oracle evaluates every kernel through its module-level `kernelmatrix`, so a Matern oracle is the oracle with that name
replaced (`monkeypatch.setattr(O, "kernelmatrix", matern(family))`)."""
import math
import os
import re

import numpy as np
import pytest

from gaussianprocessnode_amd import meta as Mt
from gaussianprocessnode_amd import multisgp as MS
from gaussianprocessnode_amd import train as TR
from gaussianprocessnode_amd import unisgp as U
from gaussianprocessnode_amd.distributions import MvNormalMeanCovariance, PointMass
from oracle import sgp_oracle as O
from tests.cpu_engine import OracleDevice
from tests.test_gpu_parity import post_tol, relF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["se", "matern12", "matern32", "matern52"]
MATERN = ["matern12", "matern32", "matern52"]
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}
_SE_KERNELMATRIX = O.kernelmatrix


# ------------------------------------------------------------------------------------------------
# the restatement (KernelFunctions.jl definitions; `with_lengthscale` divides the inputs by ell)

def kappa(family, s):
    """kappa(r), r = sqrt(s), of k = sigma2 kappa."""
    s = np.asarray(s, dtype=np.float64)
    r = np.sqrt(s)
    if family == "se":
        return np.exp(-0.5 * s)
    if family == "matern12":
        return np.exp(-r)
    if family == "matern32":
        a = math.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if family == "matern52":
        a = math.sqrt(5.0) * r
        return (1.0 + a + 5.0 * s / 3.0) * np.exp(-a)
    raise ValueError(family)


def phi(family, s):
    """The factor of dk/dell_d = sigma2 phi (a_d - b_d)^2 / ell_d^3 (matern12: 0 at r = 0)."""
    s = np.asarray(s, dtype=np.float64)
    r = np.sqrt(s)
    if family == "se":
        return np.exp(-0.5 * s)
    if family == "matern12":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, np.exp(-r) / np.where(r > 0, r, 1.0), 0.0)
    if family == "matern32":
        return 3.0 * np.exp(-math.sqrt(3.0) * r)
    if family == "matern52":
        a = math.sqrt(5.0) * r
        return (5.0 / 3.0) * (1.0 + a) * np.exp(-a)
    raise ValueError(family)


def scaled_sq_dist(ell, A, B=None):
    """s[i, j] = sum_d ((A[i, d] - B[j, d]) / ell_d)^2 by direct differences (as the oracle's SE kernelmatrix)."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    B = A if B is None else np.atleast_2d(np.asarray(B, dtype=np.float64))
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64).ravel(), (A.shape[1],))
    As, Bs = A / ell, B / ell
    s = np.zeros((A.shape[0], B.shape[0]))
    for d in range(A.shape[1]):
        t = As[:, d:d + 1] - Bs[None, :, d]
        s += t * t
    return s


def matern(family):
    """A drop-in for oracle.sgp_oracle.kernelmatrix(sigma2, ell, A, B=None) evaluating `family`."""
    if family == "se":
        return _SE_KERNELMATRIX

    def kernelmatrix(sigma2, ell, A, B=None):
        return float(sigma2) * kappa(family, scaled_sq_dist(ell, A, B))
    return kernelmatrix


# ------------------------------------------------------------------------------------------------
# 1. the ABI

def _header():
    return open(os.path.join(ROOT, "include", "sgp_hip.h")).read()


def test_header_declares_the_families_and_the_binding_exports_them():
    from gaussianprocessnode_amd import _lib
    txt = _header()
    for name, value in [("SE", 0), ("MATERN12", 1), ("MATERN32", 2), ("MATERN52", 3)]:
        assert re.search(rf"#define\s+SGP_KERNEL_{name}\s+{value}\b", txt), name
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+sgp_set_kernel_family\s*\(\s*sgp_handle\s*\*\s*h\s*,\s*int32_t\s+family\s*\)", code)
    assert re.search(r"int\s+sgp_kernelmatrix_family\s*\(\s*int32_t\s+device\s*,\s*int32_t\s+family\s*,", code)
    assert "sgp_set_kernel_family" in _lib.EXPORTS and "sgp_kernelmatrix_family" in _lib.EXPORTS
    assert (_lib.SGP_KERNEL_SE, _lib.SGP_KERNEL_MATERN12, _lib.SGP_KERNEL_MATERN32, _lib.SGP_KERNEL_MATERN52) == (0, 1, 2, 3)
    assert [_lib.family_id(f) for f in FAMILIES] == [0, 1, 2, 3] and _lib.family_id(None) == 0
    with pytest.raises(ValueError):
        _lib.family_id("matern72")


# ------------------------------------------------------------------------------------------------
# 2. the restatement against sklearn's Matern

@pytest.mark.parametrize("family", MATERN)
def test_restatement_values_match_sklearn(family):
    sk = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(int(10 * NU[family]))
    for D in [1, 3, 8]:
        A, B = rng.normal(size=(40, D)), rng.normal(size=(31, D))
        ell = rng.uniform(0.4, 2.5, D)
        ref = sk.Matern(length_scale=ell, nu=NU[family])(A, B)
        np.testing.assert_allclose(matern(family)(1.0, ell, A, B), ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(matern(family)(2.3, ell, A, B), 2.3 * ref, rtol=1e-13, atol=0)
    iso = sk.Matern(length_scale=1.3, nu=NU[family])(A, B)
    np.testing.assert_allclose(matern(family)(1.0, [1.3], A, B), iso, rtol=1e-13, atol=0)
    assert np.all(np.diag(matern(family)(0.7, ell, A)) == 0.7)           # k(x, x) = sigma2 for every family


@pytest.mark.parametrize("family", MATERN)
def test_restatement_lengthscale_factor_matches_sklearn_gradient(family):
    sk = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(7)
    D = 4
    A = rng.normal(size=(25, D))
    ell = rng.uniform(0.5, 2.0, D)
    K, dK = sk.Matern(length_scale=ell, nu=NU[family])(A, eval_gradient=True)      # dK[..., d] = dk / dlog ell_d
    s = scaled_sq_dist(ell, A)
    for d in range(D):
        delta2 = (A[:, d:d + 1] - A[None, :, d]) ** 2
        mine = phi(family, s) * delta2 / ell[d] ** 3
        np.testing.assert_allclose(mine, dK[:, :, d] / ell[d], rtol=1e-10, atol=1e-14)


# ------------------------------------------------------------------------------------------------
# 3. MaternARDKernel and the family on its way to the engine

def test_matern_ard_kernel_maps_theta_as_se():
    theta = np.array([-0.3, 0.2, 1.7, -2.0])
    for sp in (False, True):
        s2, ell = Mt.SEARDKernel(sp)(theta)
        for nu, fam in [(0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52")]:
            k = Mt.MaternARDKernel(nu, softplus_params=sp)
            m2, mell = k(theta)
            assert m2 == s2 and np.array_equal(mell, ell)
            assert k.family == fam and k.nu == nu
    assert Mt.SEARDKernel().family == "se"
    assert Mt.kernel_family(lambda th: (1.0, np.ones(1))) == "se"           # a plain callable stays SE
    with pytest.raises(ValueError):
        Mt.MaternARDKernel(3.5)


class FamilyRecorder(OracleDevice):
    """The oracle engine with kernel families: records the family of every set_kernel and evaluates it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.families = []

    def set_kernel(self, sigma2, ell, jitter=0.0, family=None):
        self.families.append(family)
        super().set_kernel(sigma2, ell, jitter)

    def set_kernel_family(self, family):
        self.families.append(family)

    def set_targets(self, y, y_var=None):
        self.set_data(self.X, y, y_var)

    def sweep_local(self, stream=0):
        pass

    def set_posterior(self, mu_v, Uv):
        self.post = (mu_v, Uv)

    def w_stats(self):
        return np.zeros(self.n), np.zeros(self.n)


class MultiFamilyRecorder(FamilyRecorder):
    """... for the MultiSGP mirror (d_out > 1, which the oracle engine does not sweep): placeholders after the setters."""

    def set_output_cov_sum(self, S):
        pass

    def sweep(self, stream=0):
        self.calls.append(("sweep", self.n))

    def posterior(self, want_cov=True, want_uv=True):
        Q = self.M * self.d_out
        return np.zeros(Q), np.eye(Q), np.eye(Q)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_reaches_the_engine_from_every_rule_and_driver(family, monkeypatch):
    monkeypatch.setattr(O, "kernelmatrix", matern(family))
    kern = Mt.SEARDKernel() if family == "se" else Mt.MaternARDKernel(NU[family])
    rng = np.random.default_rng(11)
    N, M = 9, 4
    # UniSGP :v rule batch (the node mirror's sweep)
    X = rng.uniform(-2, 2, N)
    eng = FamilyRecorder(N, M, 1)
    meta = Mt.make_uni_meta(None, np.linspace(-2, 2, M), kern, N, engine=eng, jitter=1e-8)
    theta, w = PointMass(np.array([1.0, 1.0])), PointMass(25.0)
    y = rng.normal(size=N)
    q = MvNormalMeanCovariance(np.zeros(M), 50.0 * np.eye(M))
    for i in range(N):
        q = U.prod(q, U.rule_v(PointMass(y[i]), PointMass(X[i]), w, theta, meta))
    assert eng.families and set(eng.families) == {family}
    # MultiSGP sweep
    T, d_out = 6, 2
    eng = MultiFamilyRecorder(T, M, 2, d_out)
    mmeta = Mt.MultiSGPMeta(None, rng.uniform(-2, 2, (M, 2)), None, None, None, None, kern, Mt.GPCache(), jitter=1e-12)
    mmeta.engine = eng
    eng.set_inducing(mmeta.Xu)
    ins = [PointMass(x) for x in rng.uniform(-2, 2, (T, 2))]
    outs = [PointMass(v) for v in rng.normal(size=(T, d_out))]
    prior = MvNormalMeanCovariance(np.zeros(M * d_out), 10.0 * np.eye(M * d_out))
    MS.sweep(mmeta, outs, ins, PointMass(np.eye(d_out)), PointMass(np.array([1.0, 1.0, 1.0])), prior, E_logdet_W=0.0)
    assert eng.families and set(eng.families) == {family}
    # host-paced perform_inference and the VMP drivers
    Xt = rng.uniform(-2, 2, (12, 1))
    yt = np.sin(Xt[:, 0])
    eng = FamilyRecorder(6, M, 1)
    TR.perform_inference(np.zeros(2), Xt, yt, np.linspace(-2, 2, M), eng, batch_size=6, epochs=1, family=family)
    assert len(eng.families) == 2 and set(eng.families) == {family}
    eng = FamilyRecorder(12, M, 1)
    TR.vmp_regression([1.0, 1.0], Xt, yt, np.linspace(-2, 2, M), eng, iterations=2, family=family)
    assert eng.families == [family]


def test_se_only_engine_keeps_working_and_refuses_other_families():
    class SEOnly(OracleDevice):
        pass
    eng = SEOnly(4, 3, 1)
    Mt.set_engine_kernel(eng, 1.0, [1.0], 0.0, "se")
    assert eng.s2 == 1.0
    with pytest.raises(TypeError):
        Mt.set_engine_kernel(eng, 1.0, [1.0], 0.0, "matern32")
    with pytest.raises(TypeError):
        TR._set_family(eng, "matern52")
    TR._set_family(eng, "se")


# ------------------------------------------------------------------------------------------------
# 4. the GPU tests' fixtures discriminate between the families

SHAPES = [("toy-C1", 50, 20, 1, 100.0, 1e-8, False), ("banana-C4", 1000, 128, 2, 3.0, 1e-8, True),
          ("kin40k-T", 1500, 512, 8, 1e4, 0.0, False)]


@pytest.mark.parametrize("name,N,M,D,w,jit,cls", SHAPES, ids=[s[0] for s in SHAPES])
def test_fixtures_discriminate_between_families(name, N, M, D, w, jit, cls, monkeypatch):
    from tests.test_gpu_kernel_family import case_inputs
    X, Xu, y, vy, s2, ell = case_inputs(name, N, M, D, cls)
    res = {}
    for fam in FAMILIES:
        monkeypatch.setattr(O, "kernelmatrix", matern(fam))
        r = O.vmp_sweep(Xu, X, y, vy, s2, ell, w, E_logw=math.log(w) - 0.01, jitter=jit, Lambda0=np.eye(M) / 50.0,
                        xi0=np.zeros(M))
        cond_L = np.linalg.cond(np.eye(M) / 50.0 + w * r.stats.Psi2)
        res[fam] = (r.stats.Psi2, r.mu_v, post_tol(cond_L))
    for i, a in enumerate(FAMILIES):
        for b in FAMILIES[i + 1:]:
            assert relF(res[a][0], res[b][0]) > 100 * 1e-13, (a, b)
            assert relF(res[a][1], res[b][1]) > 100 * max(res[a][2], res[b][2]), (a, b)
