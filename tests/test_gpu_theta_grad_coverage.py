"""The theta gradient on the device where the K loop of k_theta_grad_uf is split unevenly over blockIdx.z (1 < KS < T, slices of
unequal length), which no other suite reaches (cases and launch arithmetic: tests/theta_grad_coverage.py): the reference's own
M = 600 / minibatch 500 shape, the smallest T with an uneven split, all 16 k_theta_grad_uf<FAM, DO>, the point counts across which KS
steps 3 -> 2 -> 1, data points on, next to and far from inducing inputs, sgp_theta_objective_xu at T = 5 and 10, and
k_theta_grad_fold over 480 partial blocks behind an all-reduce hook.

Per case: set_inducing / set_data(weights, n_nodes = N) / set_kernel / set_prior_isotropic(50) / set_noise(W), sweep, posterior,
set_kernel at the new theta unless the case is `fresh`, theta_objective(want_grad=True).  Bounds, taken unchanged from
tests/test_gpu_multi_theta.py, tests/test_gpu_envelope.py and tests/test_gpu_xu_grad.py, which hold them against the same restatement
under the same cond(K_uu) < 1e6: value rel 1e-8; gradient and grad_xu rtol 1e-6, atol 1e-9 max|g_ref|.
Measured: profiles/theta_grad_coverage.txt.
"""
import functools
import math

import numpy as np
import pytest

from tests import theta_grad_coverage as TC
from tests.test_gpu_xu_grad import device_for
from tests.xu_grad_ref import analytic_grad_xu

pytestmark = pytest.mark.gpu

XU_CASES = ("kin40k_m600_se", "t5_ks4_m52_dout4")
HOOK_CASES = ("kin40k_m600_se", "kin40k_m600_se_fresh")


@functools.lru_cache(maxsize=None)
def evaluated(name, hook=False):
    """One device run of the case and the restatement at its q(v), shared by the tests below (not to be written to)."""
    import gaussianprocessnode_amd as G
    c = TC.inputs(name)
    ps, p = c["p_sweep"], c["p"]
    out = dict(c=c)
    with device_for(G, c["X"], c["om"], c["Y"], c["Xu"], c["d_out"], ps[0], ps[1:], c["jitter"], c["family"], c["W"]) as dev:
        if hook:
            dev.set_allreduce(lambda buf, count, stream: None)                               # single rank: the sum is the identity
        dev.sweep()
        out["mu"], out["Sig"], _ = dev.posterior(want_uv=False)
        if not c["fresh"]:
            dev.set_kernel(p[0], p[1:], c["jitter"], family=c["family"])
        out["first"] = dev.theta_objective(want_grad=True, n_ell=c["n_ell"])
        out["second"] = dev.theta_objective(want_grad=True, n_ell=c["n_ell"])
        if name in XU_CASES and not hook:
            out["xu"] = dev.theta_objective_xu(want_grad=True)
            out["xu_second"] = dev.theta_objective_xu(want_grad=True)
    out["ref"] = TC.reference(c, out["mu"], out["Sig"])
    return out


def assert_meets_the_restatement(label, out):
    c, (val, grad), (ref, g_ref) = out["c"], out["first"], out["ref"]
    assert grad.shape == (1 + c["n_ell"],)
    T, nblk, KS, slices = TC.geometry(c["N"], c["M"])
    ratio = TC.grad_ratio(grad, g_ref)
    print(f"theta_objective {label}: T {T} nblk {nblk} KS {KS} slices {slices}; value rel {abs(val - ref) / abs(ref):.3g} "
          f"(bound 1e-08); gradient error / bound = {ratio:.3g}")
    assert math.isclose(val, ref, rel_tol=1e-8), (val, ref)
    np.testing.assert_allclose(grad, g_ref, rtol=1e-6, atol=1e-9 * np.abs(g_ref).max())


@pytest.mark.parametrize("name", list(TC.CASES))
def test_value_and_gradient_meet_the_restatement(name):
    out = evaluated(name)
    if out["c"]["special"]:
        assert math.isfinite(out["first"][0]) and np.all(np.isfinite(out["first"][1]))
    assert_meets_the_restatement(name, out)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_a_second_identical_call_agrees_bitwise(name):
    """fixed-order sums: with several slices per tile row the partial index (z, y, x) is what keeps the promise"""
    out = evaluated(name)
    assert out["first"][0] == out["second"][0] and np.array_equal(out["first"][1], out["second"][1])


@pytest.mark.parametrize("name", XU_CASES)
def test_theta_objective_xu_where_the_theta_gradient_splits_unevenly(name):
    """the xu kernels have ranges of their own, and T = 5 and T = 10 are new to them too"""
    out = evaluated(name)
    c, (val, grad), (v1, g1, x1), (v2, g2, x2) = out["c"], out["first"], out["xu"], out["xu_second"]
    assert v1 == val and np.array_equal(g1, grad)                                            # bitwise those of theta_objective
    assert v2 == val and np.array_equal(g2, grad) and np.array_equal(x1, x2)
    mu, p = out["mu"], c["p"]
    ref = analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], out["Sig"] + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"],
                           c["family"])                                                      # (TC.reference asserted cond(K_uu))
    assert x1.shape == ref.shape == (c["M"], c["D"])
    print(f"theta_objective_xu {name}: grad_xu error / bound = {TC.grad_ratio(x1, ref):.3g}")
    np.testing.assert_allclose(x1, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("name", HOOK_CASES)
def test_the_hook_s_fold_over_uneven_slices(name):
    """k_theta_grad_fold over 8 x 10 x 6 = 480 partial blocks, the all-reduce an identity"""
    c = TC.inputs(name)
    T, nblk, KS, _ = TC.geometry(c["N"], c["M"])
    assert nblk * T * KS == 480
    out = evaluated(name, hook=True)
    assert_meets_the_restatement(name + " (hook)", out)
    assert out["first"][0] == out["second"][0] and np.array_equal(out["first"][1], out["second"][1])
