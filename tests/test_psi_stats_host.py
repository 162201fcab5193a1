"""The NumPy restatement of the closed-form SE Psi-statistics (tests/psi_stats_ref.py) validated without a GPU and without the
closed form: against tensor Gauss-Hermite quadrature of k and k k', against the point kernel at S = 0, against the cubature
restatement (cubature.py + oracle.sgp_oracle) as S -> 0, and with the three faults a closed form of this shape can have injected."""
import numpy as np
import pytest

from gaussianprocessnode_amd.cubature import srcubature
from oracle import sgp_oracle as O
from tests import psi_stats_ref as R

S2 = 0.8
ORDER = 60
# Measured on the CPU at the two cases below: order 60 against order 70 differs by at most 3.4e-16 (absolute, entries up to 0.8) in
# both statistics -- the quadrature has converged to rounding (order 40 against 50 still differs by 4.8e-13 in Psi2 at D = 1).
CONVERGED = 5e-16
MARGIN = 4.0            # closed form against quadrature: the convergence figure times 4 (measured: at most 5e-16)


def quadrature(Xu, ell, m, S, p):
    """E[k(Xu, x)] and E[k(Xu, x) k(x, Xu)] under N(m, S) by tensor Gauss-Hermite quadrature of order p."""
    D = len(m)
    x, w = np.polynomial.hermite.hermgauss(p)
    w = w / np.sqrt(np.pi)
    xi = np.stack([g.ravel() for g in np.meshgrid(*([x] * D), indexing="ij")], axis=1)
    ws = np.prod(np.stack([g.ravel() for g in np.meshgrid(*([w] * D), indexing="ij")], axis=1), axis=1)
    K = O.kernelmatrix(S2, ell, Xu, m + np.sqrt(2.0) * xi @ np.linalg.cholesky(S).T)
    return K @ ws, (K * ws) @ K.T


def case(D):
    """A full covariance with eigenvalues from 0.3 ell^2 up to ell^2 (the smallest lengthscale's)."""
    rng = np.random.default_rng(D)
    Xu = rng.uniform(-2, 2, (7, D))
    ell = np.linspace(0.9, 1.4, D)
    m = rng.uniform(-1, 1, D)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    S = Q @ np.diag(np.linspace(1.0, 0.3, D) * ell.min() ** 2) @ Q.T
    return Xu, ell, m, 0.5 * (S + S.T)


@pytest.fixture(scope="module", params=[1, 2])
def quad_case(request):
    Xu, ell, m, S = case(request.param)
    return Xu, ell, m, S, quadrature(Xu, ell, m, S, ORDER), quadrature(Xu, ell, m, S, ORDER + 10)


def test_the_quadrature_has_converged_and_the_closed_form_meets_it(quad_case):
    Xu, ell, m, S, q, q10 = quad_case
    conv = max(np.abs(q[0] - q10[0]).max(), np.abs(q[1] - q10[1]).max())
    e1 = np.abs(R.psi1_node(Xu, S2, ell, m, S) - q10[0]).max()
    e2 = np.abs(R.psi2_node(Xu, S2, ell, m, S) - q10[1]).max()
    print(f"D={len(m)}: order {ORDER} vs {ORDER + 10}: {conv:.3g}; closed form vs quadrature: psi1 {e1:.3g} psi2 {e2:.3g}")
    assert conv <= CONVERGED
    assert e1 <= MARGIN * CONVERGED and e2 <= MARGIN * CONVERGED


@pytest.mark.parametrize("fault,hits_psi1", [("drop2", False), ("no_det", True), ("zbar", False)])
def test_injected_faults_are_caught(quad_case, fault, hits_psi1):
    """A dropped factor 2 in Lambda + 2 S, a missing determinant factor, z-bar replaced by z_m: each moves Psi2 (and the missing
    determinant Psi1 too) by 4e-2 or more -- thirteen orders of magnitude above the bound."""
    Xu, ell, m, S, _, q10 = quad_case
    e1 = np.abs(R.psi1_node(Xu, S2, ell, m, S, fault) - q10[0]).max()
    e2 = np.abs(R.psi2_node(Xu, S2, ell, m, S, fault) - q10[1]).max()
    assert e2 > 1e-2
    assert (e1 > 1e-2) == hits_psi1


@pytest.mark.parametrize("D", [1, 2, 5])
def test_zero_covariance_is_the_point_kernel_exactly(D):
    rng = np.random.default_rng(D)
    Xu, ell, mean = rng.uniform(-2, 2, (9, D)), np.linspace(0.9, 1.4, D), rng.uniform(-2, 2, (4, D))
    K = O.kernelmatrix(S2, ell, mean, Xu)
    psi1, psi2 = R.psi_stats(Xu, S2, ell, mean, np.zeros((4, D, D)))
    np.testing.assert_allclose(psi1, K, rtol=1e-14, atol=0)
    np.testing.assert_allclose(psi2, K.T @ K, rtol=1e-14, atol=1e-300)
    assert np.array_equal(R.psi_stats(Xu, S2, ell, mean, None)[0], psi1)


def test_the_cubature_statistics_approach_the_exact_ones_and_differ_at_large_covariance():
    """The first independent measurement of the cubature path (srcubature, 2 D + 1 points), D = 2, relative to the largest entry:
        S = 1e-6 Lambda:  Psi1 2.0e-13   Psi2 6.7e-13        S = 1e-4 Lambda:  Psi1 2.0e-9   Psi2 6.7e-9
        S = 1e-2 Lambda:  Psi1 2.0e-5    Psi2 6.5e-5         S = Lambda:       Psi1 4.2e-2   Psi2 1.6e-1
    The gap falls as |S|^2 (a degree-3 rule) and is 4 % / 16 % of the largest entry at S = Lambda."""
    rng = np.random.default_rng(0)
    D = 2
    Xu, ell, m = rng.uniform(-2, 2, (7, D)), np.array([1.0, 1.3]), rng.uniform(-1, 1, D)
    gaps = {}
    for scale in (1e-6, 1e-4, 1e-2, 1.0):
        S = scale * np.diag(ell ** 2)
        pts, w = srcubature().points_weights(m, S)
        _, c1, c2 = O.psi_statistics(Xu, pts, w, S2, ell)
        e1, e2 = R.psi1_node(Xu, S2, ell, m, S), R.psi2_node(Xu, S2, ell, m, S)
        gaps[scale] = (np.abs(c1 - e1).max() / np.abs(e1).max(), np.abs(c2 - e2).max() / np.abs(e2).max())
        print(f"S = {scale:g} Lambda: cubature vs exact psi1 {gaps[scale][0]:.3g} psi2 {gaps[scale][1]:.3g}")
    assert max(gaps[1e-6]) < 1e-11 and max(gaps[1e-4]) < 1e-7 and max(gaps[1e-2]) < 1e-3
    assert gaps[1e-6][1] < gaps[1e-4][1] < gaps[1e-2][1] < gaps[1.0][1]
    assert gaps[1.0][0] > 1e-2 and gaps[1.0][1] > 5e-2


def test_packed_statistics_of_an_exact_sweep():
    rng = np.random.default_rng(3)
    T, M, D, dout = 6, 5, 2, 2
    Xu, ell, mean = rng.normal(size=(M, D)), np.array([1.1, 0.9]), rng.normal(size=(T, D))
    A = rng.normal(size=(T, D, D)) * 0.3
    S, Y = A @ A.transpose(0, 2, 1), rng.normal(size=(T, dout))
    uni, multi = R.exact_suff_stats(Xu, S2, ell, mean, S, Y, cov_sum=0.5 * np.eye(dout))
    psi1, psi2 = R.psi_stats(Xu, S2, ell, mean, S)
    assert np.array_equal(multi.Psi2, psi2) and np.allclose(multi.B, sum(np.outer(psi1[t], Y[t]) for t in range(T)), rtol=1e-14)
    assert np.allclose(multi.Ryy, Y.T @ Y + 0.5 * np.eye(dout)) and multi.s_kk == S2 * T and multi.n == T and uni.n == T
    w = rng.uniform(0, 2, T)
    w[1] = 0.0
    assert np.allclose(R.psi_stats(Xu, S2, ell, mean, S, w)[1], sum(w[t] * R.psi2_node(Xu, S2, ell, mean[t], S[t]) for t in range(T)))
