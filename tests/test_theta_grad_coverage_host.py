"""Host checks behind tests/test_gpu_theta_grad_coverage.py: the case table of tests/theta_grad_coverage.py against the launch
arithmetic of the theta gradient's data half (every new case splits the K loop unevenly, no earlier shape did), a guard on the two
source lines that arithmetic restates, what every comparison rests on (cond(K_uu), positive weights, the special points where the
case says they are), and the NumPy restatement against central differences at the r = 0 and underflow points, which the device test
cannot show.
"""
import inspect
import os

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import multi_theta_ref as R
from tests import theta_descend_ref as TD
from tests import theta_grad_coverage as TC
from tests import train_step_ref as TS
from tests.test_gpu_xu_grad import COND_MAX, SHAPES as XU_SHAPES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianprocessnode_amd", "csrc")
REDERIVE = "the K split of the theta gradient changed: re-derive the case table of tests/theta_grad_coverage.py"


def shape_of(name):
    return TC.CASES[name][1][:2]


# (T, nblk, KS, slice lengths) as the table of the cases states them
GEOMETRY = {
    TC.KIN40K: (10, 8, 6, (1, 2, 2, 1, 2, 2)),
    TC.T3_KS2: (3, 57, 2, (1, 2)),
    TC.T4_KS3: (4, 33, 3, (1, 1, 2)),
    TC.T5_KS4: (5, 21, 4, (1, 1, 1, 2)),
}


@pytest.mark.parametrize("shape", list(GEOMETRY))
def test_geometry_of_the_uneven_shapes(shape):
    assert TC.geometry(*shape) == GEOMETRY[shape]


@pytest.mark.parametrize("name", [n for n in TC.CASES if n not in TC.BOUNDARY_CASES])
def test_every_case_but_the_boundary_ones_splits_unevenly(name):
    assert shape_of(name) in GEOMETRY
    T, nblk, KS, slices = TC.geometry(*shape_of(name))
    assert 1 < KS < T and len(set(slices)) >= 2 and sum(slices) == T and min(slices) >= 1, (name, T, nblk, KS, slices)


def test_the_boundary_cases_step_the_split_down():
    got = [TC.geometry(*shape_of(n)) for n in TC.BOUNDARY_CASES]
    assert [g[1] for g in got] == [56, 57, 85, 86] and [g[2] for g in got] == [3, 2, 2, 1] and all(g[0] == 3 for g in got)
    assert [g[3] for g in got] == [(1, 1, 1), (1, 2), (1, 2), (3,)]


def test_no_shape_the_suite_had_before_splits_between_one_and_T():
    """The statement of the gap these cases close.  (A later suite may add such a shape; this list is what there was.)"""
    shapes = [s for group in TC.OLD_SHAPES.values() for s in group]
    shapes += [(s[0], s[1]) for s in XU_SHAPES]
    shapes += [(n, spec[1]) for spec in TS.GAUSS.values() for _, n, learn, _ in spec[8] if learn]
    shapes += [(spec[6], spec[2]) for spec in TD.SHAPES.values()]
    assert len(shapes) > 40
    for N, M in shapes:
        T, _, KS, slices = TC.geometry(N, M)
        assert KS in (1, T) and len(set(slices)) == 1, (N, M, T, KS)


def test_the_restated_lines_are_still_in_the_source():
    with open(os.path.join(CSRC, "sgp_api.hip")) as f:
        api = f.read()
    with open(os.path.join(CSRC, "sgp_kernels.hip.h")) as f:
        kernels = f.read()
    assert "512 / std::max(1, h->nblk * T)" in api, REDERIVE
    begin, end = kernels.index("void __launch_bounds__(256) k_theta_grad_uf("), kernels.index("void __launch_bounds__(256) k_theta_grad_uu(")
    assert begin < end and "T * ks / KS" in kernels[begin:end], REDERIVE


def test_every_case_has_its_own_seed_and_is_run_by_the_gpu_suite():
    from tests import test_gpu_theta_grad_coverage as GC
    seeds = [seed for seed, _ in TC.CASES.values()]
    assert len(set(seeds)) == len(seeds)
    assert len(TC.CASES) == len(TC.UNEVEN_CASES) + len(TC.EVERY_INST_CASES) + len(TC.BOUNDARY_CASES) + len(TC.SPECIAL_CASES)   # no name twice
    for test in (GC.test_value_and_gradient_meet_the_restatement, GC.test_a_second_identical_call_agrees_bitwise):
        (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
        assert list(mark.args[1]) == list(TC.CASES)
    assert set(GC.XU_CASES) | set(GC.HOOK_CASES) <= set(TC.CASES)
    assert "evaluated(name, hook=True)" in inspect.getsource(GC.test_the_hook_s_fold_over_uneven_slices)


def test_every_instantiation_is_a_case():
    pairs = {(TC.CASES[n][1][4], TC.CASES[n][1][3]) for n in TC.EVERY_INST_CASES}
    assert pairs == {(f, d) for f in TC.FAMILIES for d in (1, 2, 3, 4)}
    specs = [TC.CASES[n][1] for n in TC.EVERY_INST_CASES]
    for column in (5, 6, 8):                                                     # shared / ARD, weights, fresh: both values occur
        assert {s[column] for s in specs} == {False, True}


@pytest.mark.parametrize("name", list(TC.CASES))
def test_conditioning_and_weights(name):
    c = TC.inputs(name)
    for p in (c["p"], c["p_sweep"]):
        cond = TC.kuu_cond(c, p)
        assert cond < COND_MAX, (name, cond)
    print(f"{name}: cond(K_uu + jitter I) = {TC.kuu_cond(c):.2e}")
    assert (c["om"] is not None) == c["weighted"]
    assert np.all(c["omega"] > 0.0) and c["X"].shape == (c["N"], c["D"]) and c["Xu"].shape == (c["M"], c["D"])


@pytest.mark.parametrize("name", list(TC.SPECIAL_CASES))
def test_the_special_points_are_where_the_case_says(name):
    c = TC.inputs(name)
    X, Xu, N = c["X"], c["Xu"], c["N"]
    rows = list(TC.SPECIAL_ROWS)
    assert sorted(set(r // TC.TILE for r in rows)) == [0, 1, 2]                  # rows from every tile row
    last = (N // TC.TILE) * TC.TILE
    assert N % TC.TILE and last == 3584
    kinds = (TC.COINCIDENT, TC.NEAR, TC.FAR)
    assert all(len(k) == 5 and k[0] < TC.TILE and k[-1] >= last for k in kinds)  # the first in point block 0, the last in the partial block
    assert len(set(TC.COINCIDENT + TC.NEAR + TC.FAR + TC.VERY_FAR)) == 17 and TC.VERY_FAR[0] < TC.TILE <= last <= TC.VERY_FAR[1] < N
    assert np.array_equal(X[list(TC.COINCIDENT)], Xu[rows])
    gap = np.abs(X[list(TC.NEAR)] - Xu[rows])
    assert np.all(gap > 0.0) and np.all(gap < 1e-8)
    for p in (c["p"], c["p_sweep"]):
        ell = R.full_ell(p[1:], c["D"])
        s = R.scaled_sq_dist(ell, Xu, X)
        assert np.all(s[:, list(TC.FAR)] >= TC.FAR_ELLS ** 2 * c["D"]) and np.all(s[:, list(TC.VERY_FAR)] >= TC.VERY_FAR_ELLS ** 2 * c["D"])
        assert np.all(s[rows, list(TC.COINCIDENT)] == 0.0)
        near = s[rows, list(TC.NEAR)]
        assert np.all(near > 0.0) and np.all(near < 1e-15)
        Kuf = R.kernelmatrix(c["family"], p[0], ell, Xu, X)
        assert not np.any(Kuf[:, list(TC.VERY_FAR)])                             # exactly 0 for every family
        assert np.any(Kuf[:, list(TC.FAR)]) == (c["family"] != "se")             # SE: exactly 0; Matern: tiny, not 0
        assert np.max(Kuf[:, list(TC.FAR)]) < 1e-40
    ordinary = np.setdiff1d(np.arange(N), TC.COINCIDENT + TC.NEAR + TC.FAR + TC.VERY_FAR)
    assert np.all(np.abs(X[ordinary]) <= 1.7)


@pytest.mark.parametrize("name", list(TC.SPECIAL_CASES))
def test_the_restatement_meets_central_differences_at_the_special_points(name):
    """multi_theta_ref.analytic_grad against central differences (step 1e-6) of batched_objective, at the tolerance the suite holds
    that pair to (tests/test_gpu_multi_theta.py): rtol 5e-5, atol 1e-6 max|g|.  The Matern-1/2 derivative term is 0 at r = 0."""
    c = TC.inputs(name)
    mu, Sig = TD.host_qv(c, O.invsoftplus(c["p_sweep"]))
    f, g = TC.reference(c, mu, Sig)
    assert np.isfinite(f) and np.all(np.isfinite(g))
    fd = np.array([(TC.reference(c, mu, Sig, c["p"] + 1e-6 * e)[0] - TC.reference(c, mu, Sig, c["p"] - 1e-6 * e)[0]) / 2e-6
                   for e in np.eye(1 + c["n_ell"])])
    print(f"{name}: analytic against central differences, max |diff| / max|g| = {np.abs(g - fd).max() / np.abs(fd).max():.2e}")
    np.testing.assert_allclose(g, fd, rtol=5e-5, atol=1e-6 * np.abs(fd).max())
