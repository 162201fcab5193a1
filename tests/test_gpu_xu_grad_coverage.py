"""The inducing-input gradient on the device (sgp_theta_objective_xu) where no other suite takes it (cases, launch arithmetic,
reference and bound: tests/xu_grad_coverage.py): a workgroup of k_xu_grad_uf walking two and three point blocks at T = 3, 4 and 10 --
`xs` over the next block's A panel, `sums[wc]` carried in LDS, a short last range -- all 16 k_xu_grad_uf<FAM, DO> and k_xu_grad_uu
with off-diagonal tiles on both sides of the diagonal, the point count at which the range length steps, data points on, 1e-6 and 1e-9
from and 60 / 2000 lengthscales from inducing inputs, and `train.optimize_inducing` started from a subset of the data.

Per case, one device run: set_inducing / set_data(weights, n_nodes = N) / set_kernel / set_prior_isotropic(50) / set_noise(W), sweep,
posterior, set_kernel at the new theta unless the case is `fresh`, theta_objective(want_grad=True), theta_objective_xu(want_grad=True)
twice.  Bound: rtol 1e-6, atol 1e-9 max|ref| (tests/test_gpu_xu_grad.py) plus the input-rounding term of the near pairs, which the
reference computes.  Measured: profiles/xu_grad_coverage.txt.
"""
import functools

import numpy as np
import pytest

from tests import multi_theta_ref as R
from tests import xu_grad_coverage as XC
from tests.test_gpu_xu_grad import COND_MAX, device_for, problem
from tests.xu_grad_ref import analytic_grad_xu

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """One device run of the case and the reference at its q(v), shared by the tests below (not to be written to)."""
    import gaussianprocessnode_amd as G
    c = XC.inputs(name)
    ps, p = c["p_sweep"], c["p"]
    out = dict(c=c)
    with device_for(G, c["X"], c["om"], c["Y"], c["Xu"], c["d_out"], ps[0], ps[1:], c["jitter"], c["family"], c["W"]) as dev:
        dev.sweep()
        mu, Sig, _ = dev.posterior(want_uv=False)
        if not c["fresh"]:
            dev.set_kernel(p[0], p[1:], c["jitter"], family=c["family"])
        out["theta"] = dev.theta_objective(want_grad=True, n_ell=c["n_ell"])
        out["first"] = dev.theta_objective_xu(want_grad=True)
        out["second"] = dev.theta_objective_xu(want_grad=True)
    out["ref"] = XC.reference(c, mu, Sig)
    out["bound"] = XC.bound(c, out["ref"], XC.rounding_term(c, mu, Sig))
    return out


@pytest.mark.parametrize("name", list(XC.CASES))
def test_grad_xu_meets_the_restatement(name):
    out = evaluated(name)
    c, gxu, ref, bnd = out["c"], out["first"][2], out["ref"], out["bound"]
    assert gxu.shape == ref.shape == (c["M"], c["D"]) and np.all(np.isfinite(gxu))
    T, nblk, range_len, nranges, last_len, last_pts = XC.geometry(c["N"], c["M"])
    got = XC.ratio(gxu, ref, bnd)
    print(f"theta_objective_xu {name}: T {T} nblk {nblk} ranges {nranges} of {range_len} (the last of {last_len}, its last block of "
          f"{last_pts} points); grad_xu error / bound = {got:.3g}")
    assert got <= 1.0, got


@pytest.mark.parametrize("name", list(XC.CASES))
def test_value_and_theta_gradient_are_bitwise_those_of_theta_objective(name):
    out = evaluated(name)
    (val, grad), (v1, g1, _), (v2, g2, _) = out["theta"], out["first"], out["second"]
    assert grad.shape == (1 + out["c"]["n_ell"],)
    assert v1 == val and np.array_equal(g1, grad)
    assert v2 == val and np.array_equal(g2, grad)


@pytest.mark.parametrize("name", list(XC.CASES))
def test_a_second_identical_call_agrees_bitwise(name):
    """fixed-order sums: the blocks of a range in order, the ranges in order"""
    out = evaluated(name)
    assert np.array_equal(out["first"][2], out["second"][2])


@pytest.mark.parametrize("name", list(XC.SPECIAL_CASES))
def test_the_rows_of_the_coincident_and_near_inducing_inputs(name):
    """compared alone: a failure there is not to hide in the maximum over M x D"""
    out = evaluated(name)
    c, gxu, ref, bnd = out["c"], out["first"][2], out["ref"], out["bound"]
    rows = XC.special_rows(c)
    assert np.all(np.isfinite(gxu[rows]))
    per_row = {row: XC.ratio(gxu, ref, bnd, [row]) for row in rows}
    print(f"theta_objective_xu {name}: error / bound in the rows of the coincident and near inducing inputs: "
          + ", ".join(f"{row}: {v:.3g}" for row, v in per_row.items()))
    assert max(per_row.values()) <= 1.0, per_row


def test_optimize_inducing_from_a_subset_of_the_data():
    """Xu = X[:M] exactly, as the reference's experiments start: at step 0 every inducing row has a coincident data point (Matern-5/2;
    20 AdaMax steps against the NumPy loop of tests/test_gpu_xu_grad.py::test_optimize_inducing_matches_the_numpy_loop, its rtol)."""
    import gaussianprocessnode_amd as G
    from gaussianprocessnode_amd import train as TR
    from gaussianprocessnode_amd.meta import softplus
    from oracle import sgp_oracle as O
    N, M, D, d_out, jitter, steps, family = 200, 12, 2, 1, 1e-8, 20, "matern52"
    X, om, Y, _, W = problem(N, M, D, d_out, seed=9801)
    Xu = X[:M].copy()
    theta0 = O.invsoftplus(np.array([0.9, 1.0, 1.2]))
    with device_for(G, X, om, Y, Xu, d_out, 0.9, np.array([1.0, 1.2]), jitter, family, W) as dev:
        dev.sweep()
        mu, Sig, Uv = dev.posterior()
        th, Z, vals = TR.optimize_inducing(theta0, Xu, dev, q_v=(mu, Uv), steps=steps, optimizer=TR.AdaMax(), jitter=jitter)
    assert np.array_equal(Xu, X[:M]) and vals.shape == (steps,)
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(Z)) and np.all(np.isfinite(th))
    Rv = Sig + np.outer(mu, mu)
    x = np.concatenate([theta0, Xu.ravel()])
    opt = TR.AdaMax()
    for _ in range(steps):
        p = softplus(x[:3])
        z = x[3:].reshape(M, D)
        assert np.linalg.cond(R.kernelmatrix(family, p[0], p[1:], z) + jitter * np.eye(M)) < COND_MAX
        a = (p[0], p[1:], X, om, Y, Rv, mu, W, z, jitter, family)
        g = np.concatenate([R.analytic_grad(*a, n_ell=D) / (1.0 + np.exp(-x[:3])), analytic_grad_xu(*a).ravel()])
        assert np.all(np.isfinite(g))
        opt.update(x, g)
    assert not np.allclose(Z, Xu) and not np.allclose(th, theta0)
    np.testing.assert_allclose(th, x[:3], rtol=1e-6)
    np.testing.assert_allclose(Z, x[3:].reshape(M, D), rtol=1e-6)
