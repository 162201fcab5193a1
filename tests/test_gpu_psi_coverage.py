"""The exact-Psi calls at every compiled kernel instantiation and tiling path the per-call suites leave out (cases and ledger:
tests/psi_coverage.py): A the template instantiations and the DCAP 8 -> 32 switch, B a slice of k_psi2_in_accumulate /
k_psi2_pred_accumulate that walks two work units, C tile and block edges without padding and one node range over 528 tiles, D nodes
whose statistics vanish among ordinary ones.

Problems, restatements, error measures and bounds are those of tests/test_gpu_psi_{stats,sweep,theta,theta_descend,in,predict}.py,
imported from there: 1e-13 of the largest entry for Psi1, Psi2 and the :out means; value 1e-8, gradient rtol 1e-6 / atol 1e-9 max|g|;
the descent's 1e-6.  Every comparison also asserts what those suites assert per case: two calls agree bitwise, Psi2, Gamma and C_f are
exactly symmetric, sgp_psi_predict's mean is bitwise sgp_psi_stats' :out mean.  Measured errors: profiles/psi_coverage.txt.
"""
import functools
import time

import numpy as np
import pytest

from tests import psi_coverage as PC
from tests import psi_in_ref as RI
from tests import psi_predict_ref as RP
from tests import psi_stats_ref as RS
from tests import test_gpu_psi_in as PI
from tests import test_gpu_psi_predict as PP
from tests import test_gpu_psi_stats as PS
from tests import test_gpu_psi_sweep as PW
from tests import test_gpu_psi_theta as PT
from tests import test_gpu_psi_theta_descend as PD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def subset_of(name, T):
    return PC.multi_unit_subset(T) if name.endswith("multi_unit") else None


@functools.lru_cache(maxsize=None)
def in_case(name):
    seed, spec = PC.IN_CASES[name]
    return PI.problem(name, spec, seed, subset_of(name, spec[3]))


@functools.lru_cache(maxsize=None)
def predict_case(name):
    seed, spec = PC.PREDICT_CASES[name]
    return PP.problem(name, spec, seed, subset_of(name, spec[3]))


@functools.lru_cache(maxsize=None)
def theta_case(name):
    seed, spec = PC.THETA_CASES[name]
    return PT.problem(name, spec, seed)


# ---- one call with the properties every suite asserts of it ----
def in_grad(dev, c, mean=None, S=None):
    mean, S = (c["mean"], c["S"]) if mean is None else (mean, S)
    T, D = mean.shape
    U, gamma, Gamma = dev.psi_in_grad(mean, S, c["Y"][:T])
    U2, gamma2, Gamma2 = dev.psi_in_grad(mean, S, c["Y"][:T])
    assert U.shape == (T,) and gamma.shape == (T, D) and Gamma.shape == (T, D, D)
    assert np.array_equal(Gamma, Gamma.transpose(0, 2, 1))                       # exactly symmetric
    assert np.array_equal(U, U2) and np.array_equal(gamma, gamma2) and np.array_equal(Gamma, Gamma2)    # two calls agree bitwise
    return U, gamma, Gamma


def predict(dev, c, mean=None, S=None):
    mean, S = (c["mean"], c["S"]) if mean is None else (mean, S)
    (T, D), d = mean.shape, c["d_out"]
    m, Cf, cross = dev.psi_predict(mean, S, want_cross=True)
    m2, Cf2, cross2 = dev.psi_predict(mean, S, want_cross=True)
    stats_mean = dev.psi_stats(mean, S, want_psi1=False, want_psi2=False, want_out=True)[2]
    assert m.shape == (T, d) and Cf.shape == ((T,) if d == 1 else (T, d, d)) and cross.shape == (T, D, d)
    assert np.array_equal(m, stats_mean)                                         # bitwise sgp_psi_stats' :out means
    assert np.array_equal(PP.full(Cf, d), PP.full(Cf, d).transpose(0, 2, 1))     # exactly symmetric
    assert np.array_equal(m, m2) and np.array_equal(Cf, Cf2) and np.array_equal(cross, cross2)      # two calls agree bitwise
    return m, PP.full(Cf, d), cross


def assert_predict_close(label, c, got, ref):
    """got = (mean, C_f (T, d, d), cross) of some nodes against ref = (mean, C_f, cross, mag, cmag) of the same nodes"""
    m, Cf, cross = got
    out, Cf_ref, cross_ref, mag, cmag = ref
    em = float(np.max(np.abs(m - out) / np.sqrt(np.einsum("tii->ti", mag))))
    print(f"psi_predict {label}: mean error {em:.3g} (bound {PP.VALUE_RTOL:g} x magnitude)")
    assert em <= PP.VALUE_RTOL
    PP.assert_close(label, Cf, cross, c, (Cf_ref, cross_ref, mag, cmag))


def reference(c, sel=slice(None)):
    return tuple(c[k][sel] for k in ("out", "Cf", "cross", "mag", "cmag"))


def compare_in(G, name, sums_to_theta=False):
    c = in_case(name)
    with PI.device(G, c) as dev:
        got = in_grad(dev, c)
        f = dev.theta_objective_psi(c["mean"], c["S"], c["Y"]) if sums_to_theta else None
    PI.assert_close(name, got, (c["U"], c["gamma"], c["Gamma"]))
    if sums_to_theta:
        total = got[0].sum() + 0.5 * np.trace(c["W"]) * PI.SIGMA2 * c["T"]
        print(f"psi_in_grad {name}: sum of energies against theta_objective_psi rel {abs(total - f) / abs(f):.3g}")
        assert abs(total - f) <= 1e-8 * abs(f)


def compare_predict(G, name, noise=False):
    c = predict_case(name)
    d = c["d_out"]
    with PP.device(G, c) as dev:
        got = predict(dev, c)
        noisy = dev.psi_predict(c["mean"], c["S"], noise=True)[1] if noise else None
    assert_predict_close(name, c, got, reference(c))
    if noise:
        Winv = np.linalg.inv(c["W"])
        # the difference of two rounded sums: eps (|C_f| + |W^-1|) / |W^-1|, which these inputs keep below 1e-12
        assert np.finfo(float).eps * np.max((np.abs(c["Cf"]) + np.abs(Winv)) / np.abs(Winv)) < 1e-12
        err = np.max(np.abs(PP.full(noisy, d) - got[1] - Winv) / np.abs(Winv))
        print(f"psi_predict {name}: noise - plain against inv(W) rel {err:.3g}")
        assert err <= 1e-12


def compare_theta(G, name):
    c = theta_case(name)
    with PT.device(G, c) as dev:
        f, g = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        f2, g2 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"], want_grad=True)
        f3 = dev.theta_objective_psi(c["mean"], c["S"], c["Y"])
    assert g.shape == (1 + c["n_ell"],)
    assert f == f2 == f3 and np.array_equal(g, g2)               # two calls agree bitwise
    PT.assert_close(name, f, g, c["f"], c["g"])


def compare_stats(G, name):
    seed, (d_out, M, D, T, cov, weights, scale) = PC.STATS_CASES[name]
    psi1, psi2, out = PS.check(G, M, D, T, seed, cov=cov, d_out=d_out, weights=weights, ell_scale=scale)
    # nothing of the padding rows up to the tile edge comes back
    assert psi1.shape == (T, M) and psi2.shape == (M, M) and out.shape == (T, d_out)
    assert np.all(np.isfinite(psi1)) and np.all(np.isfinite(psi2)) and np.all(np.isfinite(out))
    return psi1, psi2, out


# ---- A. the instantiation matrix ----
@pytest.mark.parametrize("name", ["in_D3", "in_D4", "in_D6", "in_D7"])
def test_psi_in_grad_at_every_dimension_no_other_suite_runs(G, name):
    compare_in(G, name, sums_to_theta=True)


@pytest.mark.parametrize("name", ["pred_D9_dout1", "pred_D32_dout4", "pred_D16_dout4", "pred_D17_dout1"])
def test_psi_predict_at_the_wide_instantiations_and_the_lds_reread_of_the_prep(G, name):
    compare_predict(G, name, noise=True)


@pytest.mark.parametrize("name", ["theta_D8", "theta_D9", "theta_D9_shared"])
def test_theta_objective_psi_across_the_dcap_switch(G, name):
    compare_theta(G, name)


def test_theta_descend_psi_beyond_the_dcap_switch(G):
    seed, spec = PC.DESCEND_CASES["descend_D9"]
    PD.compare(G, PD.problem("descend_D9", spec, seed))


@pytest.mark.parametrize("name", ["stats_D7", "stats_D8", "stats_D9", "stats_D16", "stats_D17", "stats_D9_rank1"])
def test_psi_stats_across_the_dcap_switch_and_the_staging_remainders(G, name):
    compare_stats(G, name)


# ---- B. a slice that walks two work units ----
def assert_two_units_per_slice(c):
    T, M = c["T"], c["M"]
    assert PC.psi_in_units(M) == 3 and PC.psi_in_slices(T, M) == 2            # slice 0 walks units 0 and 2, slice 1 unit 1
    assert PC.psi_in_slices(T - 1, M) == 3 and PC.psi_in_slices(256, M) == 3  # one node fewer, and a call of 256: one unit each


def test_psi_in_grad_where_a_slice_walks_two_units(G, monkeypatch):
    c = in_case("in_multi_unit")
    assert_two_units_per_slice(c)
    T, sub = c["T"], PC.multi_unit_subset(c["T"])
    mean, S, Y = c["mean"], c["S"], c["Y"]
    start = time.perf_counter()
    with PI.device(G, c) as dev:
        got = in_grad(dev, c)
        wall = time.perf_counter() - start
        shorter = dev.psi_in_grad(mean[:-1], S[:-1], Y[:-1])
        first = dev.psi_in_grad(mean[:256], S[:256], Y[:256])
        last = dev.psi_in_grad(mean[-256:], S[-256:], Y[-256:])
    print(f"psi_in_grad in_multi_unit: T {T}, device set up and two calls in {wall:.2f} s")
    assert all(np.all(np.isfinite(x)) for x in got)
    PI.assert_close("in_multi_unit, 2671 nodes", tuple(x[sub] for x in got), (c["U"], c["gamma"], c["Gamma"]))
    PI.assert_close("in_multi_unit, first 256 nodes against a call of 256", tuple(x[:256] for x in got), first)
    PI.assert_close("in_multi_unit, last 256 nodes against a call of 256", tuple(x[-256:] for x in got), last)
    # three slices of one unit each at T - 1: the slice count is the one thing that may change the order of a node's sum
    PI.assert_close("in_multi_unit, T - 1 nodes (three slices)", tuple(x[:-1] for x in got), shorter)
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "4096")
    with PI.device(G, c) as dev:
        chunked = dev.psi_in_grad(mean, S, Y)
    for x, y in zip(got, chunked):
        assert np.array_equal(x, y)


def test_psi_predict_where_a_slice_walks_two_units(G, monkeypatch):
    c = predict_case("pred_multi_unit")
    assert_two_units_per_slice(c)
    T, sub = c["T"], PC.multi_unit_subset(c["T"])
    mean, S = c["mean"], c["S"]
    start = time.perf_counter()
    with PP.device(G, c) as dev:
        got = predict(dev, c)
        wall = time.perf_counter() - start
        first = predict(dev, c, mean[:256], S[:256])
        last = predict(dev, c, mean[-256:], S[-256:])
    print(f"psi_predict pred_multi_unit: T {T}, device set up, two calls and the :out means in {wall:.2f} s")
    assert all(np.all(np.isfinite(x)) for x in got)
    assert_predict_close("pred_multi_unit, 2671 nodes", c, tuple(x[sub] for x in got), reference(c))
    n = len(sub)
    assert np.array_equal(sub[:256], np.arange(256)) and np.array_equal(sub[-256:], np.arange(T - 256, T))
    for label, nodes, part, small in (("first", slice(0, 256), slice(0, 256), first), ("last", slice(T - 256, T), slice(n - 256, n), last)):
        assert_predict_close(f"pred_multi_unit, {label} 256 nodes against a call of 256", c, tuple(x[nodes] for x in got),
                             small + (c["mag"][part], c["cmag"][part]))
    monkeypatch.setenv("SGP_PREDICT_CHUNK", "4096")
    with PP.device(G, c) as dev:
        chunked = dev.psi_predict(mean, S, want_cross=True)
    for x, y in zip(got, (chunked[0], PP.full(chunked[1], c["d_out"]), chunked[2])):
        assert np.array_equal(x, y)


# ---- C. edges without padding ----
@pytest.mark.parametrize("name", ["stats_M64", "stats_M128"])
def test_psi_stats_where_the_tile_has_no_padding_row(G, name):
    compare_stats(G, name)


def test_exact_sweep_where_the_tile_has_no_padding_row(G):
    PW.test_exact_sweep_matches_the_oracle_on_the_restated_statistics(G, 2, 64, 2, 65)


def test_theta_objective_psi_where_the_tile_has_no_padding_row(G):
    compare_theta(G, "theta_M64")


@pytest.mark.parametrize("name", ["in_M64", "in_T256", "in_T512"])
def test_psi_in_grad_at_a_full_tile_and_at_full_workgroups(G, name):
    compare_in(G, name)


@pytest.mark.parametrize("name", ["pred_M64", "pred_M128", "pred_T256", "pred_T512"])
def test_psi_predict_at_full_tiles_and_at_full_workgroups(G, name):
    compare_predict(G, name)


def test_psi_stats_with_one_node_range_over_528_tiles(G):
    _, (d_out, M, D, T, _, _, _) = PC.STATS_CASES["stats_one_range_M1985"]
    assert PC.psi_ranges(T, M) == (1, T) and PC.psi_ranges(T, M - 1)[0] == 2    # 528 lower tiles: one range; 496: still two
    psi1, psi2, out = compare_stats(G, "stats_one_range_M1985")
    assert psi2.shape == (1985, 1985) and np.array_equal(psi2, psi2.T)
    assert np.max(psi2) > 1e3 * np.median(psi2)                                  # (far from flat at these lengthscales)


# ---- D. nodes whose statistics vanish, among ordinary ones ----
FAR, WIDE = PC.FAR_NODE, PC.WIDE_NODE


def kept(T, *nodes):
    return np.setdiff1d(np.arange(T), nodes)


def exactly_zero(x, no_negative_zero=False):
    return not np.any(x) and not (no_negative_zero and np.any(np.signbit(x)))


def test_vanishing_nodes_psi_stats(G):
    seed, (d_out, M, D, T, cov, _, scale) = PC.STATS_CASES["stats_special"]
    Xu, ell, mean0, S0, mu = PS.problem(M, D, T, seed, cov=cov, d_out=d_out, ell_scale=scale)
    mean, S = PC.with_special_nodes(Xu, ell, mean0, S0)
    ones = np.ones(T)
    no_wide, neither = ones.copy(), ones.copy()
    no_wide[WIDE], neither[[FAR, WIDE]] = 0.0, 0.0
    with PS.device(G, Xu, ell, d_out) as dev:
        psi1, psi2, out = dev.psi_stats(mean, S, None, mu, want_out=True)
        again = dev.psi_stats(mean, S, None, mu, want_out=True)
        psi2_no_wide = dev.psi_stats(mean, S, no_wide, want_psi1=False)[1]
        psi1_o, psi2_o, out_o = dev.psi_stats(mean0, S0, neither, mu, want_out=True)
    r1, r2 = RS.psi_stats(Xu, 0.8, ell, mean, S)
    ref_out = np.stack([psi1 @ mu[d * M:(d + 1) * M] for d in range(d_out)], axis=1)
    e1, e2, eo = PS.rel_max(psi1, r1), PS.rel_max(psi2, r2), PS.rel_max(out, ref_out)
    wide = float(np.max(np.abs(psi1[WIDE] - r1[WIDE])) / np.max(np.abs(r1[WIDE])))
    print(f"psi_stats stats_special: psi1 {e1:.3g} psi2 {e2:.3g} out {eo:.3g}; the wide node's psi1 row, relative to its own "
          f"largest entry {wide:.3g}")
    assert np.array_equal(psi2, psi2.T)
    for a, b in zip((psi1, psi2, out), again):
        assert np.array_equal(a, b)
    assert e1 < PS.TOL and e2 < PS.TOL and eo < PS.TOL and wide < PS.TOL
    assert exactly_zero(r1[FAR]) and exactly_zero(psi1[FAR], no_negative_zero=True) and exactly_zero(out[FAR], no_negative_zero=True)
    # the far node adds nothing to Psi2, and no other node's statistics change for the two being there
    assert np.array_equal(psi2_no_wide, psi2_o)
    rest = kept(T, FAR, WIDE)
    assert np.array_equal(psi1[rest], psi1_o[rest]) and np.array_equal(out[rest], out_o[rest])


def test_vanishing_nodes_psi_in_grad(G):
    c = in_case("in_special")
    T = c["T"]
    mean, S = PC.with_special_nodes(c["Xu"], c["ell"], c["mean"], c["S"])
    ref = RI.evaluate(PI.SIGMA2, c["ell"], mean, S, c["Y"], c["Rv"], c["mu"], c["W"], c["Xu"], c["jitter"])
    with PI.device(G, c) as dev:
        got = in_grad(dev, c, mean, S)
        ordinary = dev.psi_in_grad(c["mean"], c["S"], c["Y"])
    for x, r in zip(got, ref):
        assert exactly_zero(r[FAR]) and exactly_zero(x[FAR])                    # where the restatement is zero: equality
    others, rest = kept(T, FAR), kept(T, FAR, WIDE)
    PI.assert_close("in_special, the wide node", tuple(x[[WIDE]] for x in got), tuple(r[[WIDE]] for r in ref))
    PI.assert_close("in_special, all but the far node", tuple(x[others] for x in got), tuple(r[others] for r in ref))
    for x, o in zip(got, ordinary):
        assert np.array_equal(x[rest], o[rest])


def test_vanishing_nodes_psi_predict(G):
    c = predict_case("pred_special")
    T, d = c["T"], c["d_out"]
    mean, S = PC.with_special_nodes(c["Xu"], c["ell"], c["mean"], c["S"])
    ref = RP.predict(PP.SIGMA2, c["ell"], mean, S, c["Rv"], c["mu"], c["Xu"], d, PP.JITTER)
    with PP.device(G, c) as dev:
        got = predict(dev, c, mean, S)
        ordinary = predict(dev, c)
    m, Cf, cross = got
    assert exactly_zero(ref[0][FAR]) and exactly_zero(ref[2][FAR]) and exactly_zero(ref[4][FAR])
    assert exactly_zero(m[FAR], no_negative_zero=True) and exactly_zero(cross[FAR], no_negative_zero=True)       # zero, and no negative zero
    assert np.array_equal(ref[1][FAR], PP.SIGMA2 * np.eye(d))                                  # the prior term alone
    assert_predict_close("pred_special, the far node", c, tuple(x[[FAR]] for x in got), tuple(r[[FAR]] for r in ref))
    assert_predict_close("pred_special, the wide node", c, tuple(x[[WIDE]] for x in got), tuple(r[[WIDE]] for r in ref))
    assert_predict_close("pred_special, all nodes", c, got, ref)
    rest = kept(T, FAR, WIDE)
    for x, o in zip(got, ordinary):
        assert np.array_equal(x[rest], o[rest])
