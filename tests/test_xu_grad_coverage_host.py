"""Host checks behind tests/test_gpu_xu_grad_coverage.py: the case table of tests/xu_grad_coverage.py against the launch arithmetic
of the inducing-input gradient's data half (every geometry case walks several point blocks per workgroup at T >= 3 or sits on the
step of that rule; no earlier shape did), a guard on the source lines that arithmetic restates, that the cases are discriminating
(a reference that lost a block, a range, a column half or half the K_uu part misses the bound by 10 x and more; so does one that
lost the coincident and near pairs, while the far points carry nothing), the input-rounding term of the bound against a float64
route that subtracts scaled coordinates as the device does, and the reference itself against mpmath at 60 digits.
"""
import functools
import os

import numpy as np
import pytest

from oracle import sgp_oracle as O
from tests import multi_theta_ref as R
from tests import theta_descend_ref as TD
from tests import xu_grad_coverage as XC
from tests.test_gpu_xu_grad import COND_MAX, SHAPES as XU_SHAPES
from tests.xu_grad_ref import analytic_grad_xu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianprocessnode_amd", "csrc")
REDERIVE = "the ranges of k_xu_grad_uf changed: re-derive the case table of tests/xu_grad_coverage.py"
DISCRIMINATION = 10.0


def shape_of(name):
    return XC.CASES[name][1][:2]


# (T, nblk, range_len, nranges, blocks in the last range, points in the last block) as the table of the cases states them
GEOMETRY = {
    XC.M600_LEN2: (10, 26, 2, 13, 2, 1),
    XC.M600_SHORT: (10, 27, 2, 14, 1, 36),
    XC.M600_LEN3: (10, 51, 3, 17, 3, 1),
    (5440, XC.BOUNDARY_M): (3, 85, 1, 85, 1, 64),
    (5441, XC.BOUNDARY_M): (3, 86, 2, 43, 2, 1),
    XC.T3_LEN2: (3, 86, 2, 43, 2, 60),
    XC.T4_LEN2: (4, 65, 2, 33, 1, 34),
}


@pytest.mark.parametrize("name", list(XC.CASES))
def test_geometry_of_every_case(name):
    assert XC.geometry(*shape_of(name)) == GEOMETRY[shape_of(name)]
    N, M = shape_of(name)
    assert N * M < 2e6
    blocks = XC.range_blocks(N, M)
    T, nblk, range_len, nranges, last_len, last_pts = XC.geometry(N, M)
    assert len(blocks) == nranges and blocks[0][0] == 0 and blocks[-1] == (nblk - last_len, nblk) and 1 <= last_pts <= XC.TILE
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and all(b1 - b0 == range_len for b0, b1 in blocks[:-1])


def test_what_the_cases_reach():
    geo = {n: XC.geometry(*shape_of(n)) for n in XC.CASES}
    long_ = [n for n in XC.CASES if n != "boundary_N5440"]
    assert all(geo[n][0] >= 3 and geo[n][2] >= 2 for n in long_)                             # several blocks per workgroup at T >= 3
    assert geo["boundary_N5440"][2] == 1 and geo["boundary_N5441"][2] == 2                   # the step of the rule at T = 3
    assert geo["m600_len3"][2] == 3
    assert {n for n in XC.CASES if geo[n][4] < geo[n][2]} == {"m600_short_last"} | set(XC.EVERY_INST_CASES)   # a short last range
    assert XC.inputs("t3_len2_D32")["D"] == 32
    assert XC.inputs("m600_len2")["fresh"] is False and XC.inputs("m600_len2_fresh")["fresh"] is True


def test_no_shape_the_suite_had_before_walks_blocks_at_three_tiles_or_has_a_short_last_range():
    """The statement of the gap these cases close.  (A later suite may add such a shape; this list is what there was.)"""
    shapes = [s for group in XC.OLD_SHAPES.values() for s in group]
    assert {(s[0], s[1]) for s in XU_SHAPES} <= set(shapes) and len(shapes) >= 13
    for N, M in shapes:
        T, nblk, range_len, nranges, last_len, _ = XC.geometry(N, M)
        assert not (range_len > 1 and T > 2), (N, M, T, range_len)
        assert last_len == range_len or (N, M) in ((8193, 128), (8193, 70)), (N, M, range_len, last_len)
    # (8193, .) has T = 2: 65 ranges of two, the last of one -- the only short last range there was, and not at T > 2
    assert all(XC.geometry(N, M)[0] == 2 and XC.geometry(N, M)[2:5] == (2, 65, 1) for N, M in ((8193, 128), (8193, 70)))


def test_the_restated_lines_are_still_in_the_source():
    with open(os.path.join(CSRC, "sgp_api.hip")) as f:
        api = f.read()
    with open(os.path.join(CSRC, "sgp_kernels.hip.h")) as f:
        kernels = f.read()
    begin, end = api.index("static void xu_ranges("), api.index('extern "C" int sgp_theta_objective_xu(')
    assert begin < end and "std::max(1, 256 / T)" in api[begin:end] and "(nblk + want - 1) / want" in api[begin:end], REDERIVE
    begin, end = kernels.index("void __launch_bounds__(256) k_xu_grad_uf("), kernels.index("void __launch_bounds__(256) k_xu_grad_uu(")
    assert begin < end and "b1 = min(nblk, b0 + range_len)" in kernels[begin:end], REDERIVE


def test_every_case_has_its_own_seed_and_is_run_by_the_gpu_suite():
    from tests import test_gpu_xu_grad_coverage as GC
    from tests import theta_grad_coverage as TC
    seeds = [seed for seed, _ in XC.CASES.values()]
    assert len(set(seeds)) == len(seeds) and not set(seeds) & {seed for seed, _ in TC.CASES.values()}
    assert len(XC.CASES) == len(XC.LONG_CASES) + len(XC.BOUNDARY_CASES) + len(XC.EVERY_INST_CASES) + len(XC.SPECIAL_CASES)
    for test in (GC.test_grad_xu_meets_the_restatement, GC.test_value_and_theta_gradient_are_bitwise_those_of_theta_objective,
                 GC.test_a_second_identical_call_agrees_bitwise):
        (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
        assert list(mark.args[1]) == list(XC.CASES)
    (mark,) = [m for m in GC.test_the_rows_of_the_coincident_and_near_inducing_inputs.pytestmark if m.name == "parametrize"]
    assert list(mark.args[1]) == list(XC.SPECIAL_CASES)


def test_every_instantiation_is_a_case():
    specs = [XC.CASES[n][1] for n in XC.EVERY_INST_CASES]
    assert {(s[4], s[3]) for s in specs} == {(f, d) for f in XC.FAMILIES for d in (1, 2, 3, 4)}
    for column in (5, 6, 8):                                                     # shared / ARD, weights, fresh: both values occur
        assert {s[column] for s in specs} == {False, True}
    assert {(XC.CASES[n][1][4], XC.CASES[n][1][3]) for n in XC.SPECIAL_CASES} == {(f, d) for f in XC.FAMILIES for d in (1, 2)}


@functools.lru_cache(maxsize=None)
def host_eval(name):
    """The case's reference, rounding term and bound at the host's q(v) (one VMP update at p_sweep, tests/theta_descend_ref.py)"""
    c = XC.inputs(name)
    mu, Sig = TD.host_qv(c, O.invsoftplus(c["p_sweep"]))
    ref = XC.reference(c, mu, Sig)
    term = XC.rounding_term(c, mu, Sig)
    return c, mu, Sig, ref, term, XC.bound(c, ref, term)


@pytest.mark.parametrize("name", list(XC.CASES))
def test_conditioning_and_weights(name):
    c = XC.inputs(name)
    for p in (c["p"], c["p_sweep"]):
        assert XC.kuu_cond(c, p) < COND_MAX, (name, XC.kuu_cond(c, p))
    print(f"{name}: cond(K_uu + jitter I) = {XC.kuu_cond(c):.2e}")
    assert (c["om"] is not None) == c["weighted"]
    assert np.all(c["omega"] > 0.0) and c["X"].shape == (c["N"], c["D"]) and c["Xu"].shape == (c["M"], c["D"])


def test_the_point_by_point_data_half_is_the_restatement_s():
    """uf_terms over every point is analytic_grad_xu without its K_uu half"""
    c, mu, Sig, _, _, _ = host_eval("every_inst_matern32_dout3")
    p = c["p"]
    g = analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"], c["family"],
                         uu_scale=0.0)
    np.testing.assert_allclose(XC.uf_terms(c, mu, Sig, np.arange(c["N"])), g, rtol=1e-12, atol=1e-12 * np.abs(g).max())


# ---- the cases are discriminating ----
def points_of(N, blocks, columns=range(XC.TILE)):
    return [XC.TILE * b + j for b in blocks for j in columns if XC.TILE * b + j < N]


@pytest.mark.parametrize("name", list(XC.GEOMETRY_CASES))
def test_a_reference_that_lost_part_of_the_sum_misses_the_bound(name):
    c, mu, Sig, ref, _, bnd = host_eval(name)
    N, M, p = c["N"], c["M"], c["p"]
    ranges = XC.range_blocks(N, M)
    nblk = XC.geometry(N, M)[1]
    lost = {
        "(a) every range's last block": ref - XC.uf_terms(c, mu, Sig, points_of(N, [b1 - 1 for _, b1 in ranges])),
        "(b) the last range": ref - XC.uf_terms(c, mu, Sig, points_of(N, range(*ranges[-1]))),
        "(c) the second column half of every block": ref - XC.uf_terms(c, mu, Sig, points_of(N, range(nblk), range(32, 64))),
        "(d) half the K_uu part": analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"],
                                                   c["jitter"], c["family"], uu_scale=0.5),
    }
    factors = {k: XC.ratio(v, ref, bnd) for k, v in lost.items()}
    print(f"{name}: error / bound without " + "; ".join(f"{k}: {v:.3g}" for k, v in factors.items()))
    assert all(v >= DISCRIMINATION for v in factors.values()), factors


def without_pairs(c, mu, Sig, ref, pairs):
    g = ref.copy()
    A = XC.coefficients(c, mu, Sig, [n for _, n in pairs])
    for j, (row, n) in enumerate(pairs):
        g[row] -= A[row, j] * XC.pair_factor_mp(c, row, n)
    return g


@pytest.mark.parametrize("name", list(XC.SPECIAL_CASES))
def test_the_special_pairs_carry_weight_and_the_far_points_none(name):
    c, mu, Sig, ref, _, bnd = host_eval(name)
    rows = XC.special_rows(c)
    lost = XC.ratio(without_pairs(c, mu, Sig, ref, tuple(c["coincident"]) + tuple(c["near"])), ref, bnd, rows)
    far = XC.ratio(ref - XC.uf_terms(c, mu, Sig, list(c["far"]) + list(c["very_far"])), ref, bnd)
    print(f"{name}: error / bound in rows {rows} without the coincident and near pairs {lost:.3g}; without the far points {far:.3g}")
    assert lost >= DISCRIMINATION, lost
    assert far <= 1.0, far


@pytest.mark.parametrize("name", list(XC.SPECIAL_CASES))
def test_the_special_points_are_where_the_case_says(name):
    c = XC.inputs(name)
    X, Xu, N, M = c["X"], c["Xu"], c["N"], c["M"]
    _, nblk, range_len, _, _, last_pts = XC.geometry(N, M)
    assert range_len == 2 and N - last_pts == (nblk - 1) * XC.TILE == 5440
    kinds = ([n for _, n in XC.COINCIDENT], [n for _, n in XC.NEAR_1E6], [n for _, n in XC.NEAR_1E9], list(XC.FAR), list(XC.VERY_FAR))
    for pts in kinds:                                    # the first block of a range, the second block of a range, the last block
        b = [n // XC.TILE for n in pts]
        assert b[0] % 2 == 0 and b[1] % 2 == 1 and b[1] < nblk - 1 and b[2] == nblk - 1 and pts[2] < N
    assert len({n for pts in kinds for n in pts}) == 15
    for pairs in (XC.COINCIDENT, XC.NEAR_1E6, XC.NEAR_1E9):
        assert sorted(row // XC.TILE for row, _ in pairs) == [0, 1, 2] and all(row < M for row, _ in pairs)
    assert all(np.array_equal(X[n], Xu[row]) for row, n in XC.COINCIDENT)
    for scale, pairs in ((1e-6, XC.NEAR_1E6), (1e-9, XC.NEAR_1E9)):
        gap = np.array([np.abs(X[n] - Xu[row]) for row, n in pairs])
        assert np.all(gap > 0.0) and np.all(gap < 6.0 * scale) and gap.max() > 0.1 * scale
    for p in (c["p"], c["p_sweep"]):
        ell = R.full_ell(p[1:], c["D"])
        s = R.scaled_sq_dist(ell, Xu, X)
        assert np.all(s[:, list(XC.FAR)] >= XC.FAR_ELLS ** 2 * c["D"]) and np.all(s[:, list(XC.VERY_FAR)] >= XC.VERY_FAR_ELLS ** 2 * c["D"])
        Kuf = R.kernelmatrix(c["family"], p[0], ell, Xu, X)
        assert not np.any(Kuf[:, list(XC.VERY_FAR)])                             # exactly 0 for every family
        assert np.any(Kuf[:, list(XC.FAR)]) == (c["family"] != "se")             # SE: exactly 0; Matern: tiny, not 0
        assert np.max(Kuf[:, list(XC.FAR)]) < 1e-40
        assert all(Kuf[row, n] == p[0] for row, n in XC.COINCIDENT)
    ordinary = np.setdiff1d(np.arange(N), [n for pts in kinds for n in pts])
    assert np.all(np.abs(X[ordinary]) <= 1.7)


# ---- the bound's input-rounding term ----
@pytest.mark.parametrize("name", list(XC.SPECIAL_CASES))
def test_the_scaled_coordinate_route_stays_inside_the_bound(name):
    """The reference with the near pairs' factors formed as the device forms them, against the reference: inside `bound` with a
    factor 2 to spare at XU_C_BOUND (settled here, on the CPU alone).  The plain float64 restatement (analytic_grad_xu: r from scaled
    coordinates, the direct difference as the vector) is printed beside it."""
    c, mu, Sig, ref, term, bnd = host_eval(name)
    base = XC.bound(c, ref)
    scaled = XC.substituted(c, mu, Sig, ref, tuple(c["near"]),
                            lambda c, row, n: XC.pair_factor_scaled(c, row, n) - XC.pair_factor_mp(c, row, n) + XC.pair_factor_f64(c, row, n))
    p = c["p"]
    plain = analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"], c["family"])
    rows = XC.special_rows(c)
    r_bound, r_base = XC.ratio(scaled, ref, bnd, rows), XC.ratio(scaled, ref, base, rows)
    print(f"{name}: scaled-coordinate route, error / bound {r_bound:.3g} (against the base bound alone {r_base:.3g}); plain float64 "
          f"restatement {XC.ratio(plain, ref, bnd, rows):.3g}; largest term / base bound {float((term / base).max()):.3g}")
    assert np.array_equal(scaled[np.setdiff1d(np.arange(c["M"]), rows)], ref[np.setdiff1d(np.arange(c["M"]), rows)])
    assert r_bound <= 0.5, r_bound
    if c["family"] != "matern12":
        assert float((term / base).max()) < 1e-6                                 # negligible but next to the kink


# ---- the reference's own accuracy ----
def thinned(c, M=20, N=200):
    """The special case cut to M inducing rows and N points, every special pair kept (indices remapped)"""
    special_n = sorted({n for _, n in tuple(c["coincident"]) + tuple(c["near"])} | set(c["far"]) | set(c["very_far"]))
    rows = XC.special_rows(c)
    keep_m = sorted(rows + [m for m in range(0, c["M"], 7) if m not in rows][:M - len(rows)])
    keep_n = sorted(special_n + [n for n in range(1, c["N"], 29) if n not in special_n][:N - len(special_n)])
    assert len(keep_m) == M and len(keep_n) == N
    rm, rn = {m: i for i, m in enumerate(keep_m)}, {n: i for i, n in enumerate(keep_n)}
    t = dict(c, name=c["name"] + " (thinned)", M=M, N=N, Xu=c["Xu"][keep_m], X=c["X"][keep_n], Y=c["Y"][keep_n], omega=c["omega"][keep_n])
    for key in ("coincident", "near"):
        t[key] = tuple((rm[row], rn[n]) for row, n in c[key])
    for key in ("far", "very_far"):
        t[key] = tuple(rn[n] for n in c[key])
    return t


def mp_grad_xu(c, mu, Sig, digits=XC.MP_DIGITS):
    """tests/xu_grad_ref.py in mpmath, every quantity from the direct differences"""
    import mpmath as mp
    with mp.workdps(digits):
        M, N, D, d = c["M"], c["N"], c["D"], c["d_out"]
        f = lambda a: mp.mpf(float(a))
        s2, fam = f(c["p"][0]), c["family"]
        ell = [f(e) for e in R.full_ell(c["p"][1:], D)]
        Xu, X = [[f(v) for v in row] for row in c["Xu"]], [[f(v) for v in row] for row in c["X"]]

        def kappa(r):
            if fam == "se":
                return mp.exp(-r * r / 2)
            if fam == "matern12":
                return mp.exp(-r)
            a = (mp.sqrt(3) if fam == "matern32" else mp.sqrt(5)) * r
            return (1 + a) * mp.exp(-a) if fam == "matern32" else (1 + a + a * a / 3) * mp.exp(-a)

        def dist(a, b):
            return mp.sqrt(sum(((a[k] - b[k]) / ell[k]) ** 2 for k in range(D)))
        r_uu = [[dist(Xu[i], Xu[j]) for j in range(M)] for i in range(M)]
        r_uf = [[dist(Xu[i], X[n]) for n in range(N)] for i in range(M)]
        Kuu = mp.matrix(M, M)
        Kuf = mp.matrix(M, N)
        for i in range(M):
            for j in range(M):
                Kuu[i, j] = s2 * kappa(r_uu[i][j]) + (f(c["jitter"]) if i == j else 0)
            for n in range(N):
                Kuf[i, n] = s2 * kappa(r_uf[i][n])
        Kinv = Kuu ** -1
        om = [f(v) for v in c["omega"]]
        W = mp.matrix(np.atleast_2d(c["W"]).tolist())
        trW = sum(W[i, i] for i in range(d))
        KufW = mp.matrix(M, N)
        for i in range(M):
            for n in range(N):
                KufW[i, n] = Kuf[i, n] * om[n]
        Psi2 = KufW * Kuf.T
        Rv = mp.matrix((Sig + np.outer(mu, mu)).tolist())
        S = mp.matrix(M, M)
        for a in range(d):
            for b in range(d):
                S += W[a, b] * Rv[a * M:(a + 1) * M, b * M:(b + 1) * M]
        GK = (S - trW * Kinv) * KufW
        mus = mp.matrix(np.asarray(mu).reshape(d, M).T.tolist())                               # M x d
        Yw = mp.matrix((c["omega"][:, None] * c["Y"].reshape(N, d)).tolist())                    # N x d
        A = GK - mus * (W * Yw.T)
        H = Kinv * Psi2 * Kinv
        g = np.empty((M, D))
        for m in range(M):
            zuf = [A[m, n] * s2 * XC.mp_phi(fam, r_uf[m][n], mp) for n in range(N)]
            zuu = [trW * H[m, j] * s2 * XC.mp_phi(fam, r_uu[m][j], mp) for j in range(M)]
            for k in range(D):
                g[m, k] = float((sum(zuf[n] * (X[n][k] - Xu[m][k]) for n in range(N))
                                 + sum(zuu[j] * (Xu[j][k] - Xu[m][k]) for j in range(M))) / ell[k] ** 2)
        return g


@pytest.mark.parametrize("name", ["special_matern12_dout1", "special_matern52_dout2"])
def test_the_reference_meets_mpmath_on_a_thinned_special_case(name):
    """M = 20, N = 200 with the same special pairs: the mpmath-corrected float64 reference within a tenth of the bound of the whole
    restatement at 60 digits; without the correction the Matern-1/2 rows at 1e-9 are not."""
    c = thinned(XC.inputs(name))
    assert XC.kuu_cond(c) < COND_MAX
    mu, Sig = TD.host_qv(c, O.invsoftplus(c["p_sweep"]))
    ref = XC.reference(c, mu, Sig)
    exact = mp_grad_xu(c, mu, Sig)
    bnd = XC.bound(c, exact, XC.rounding_term(c, mu, Sig))
    got = XC.ratio(ref, exact, bnd)
    p = c["p"]
    plain = analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"], c["family"])
    print(f"{name} thinned to M 20, N 200: reference against mpmath, error / bound {got:.3g}; uncorrected float64 restatement "
          f"{XC.ratio(plain, exact, bnd):.3g}")
    assert got <= 0.1, got


def test_the_matern12_convention_at_the_kink():
    """phi = 0 at r = 0, in the reference as in fam_kappa_phi; next to it phi (x - z) is a unit vector over ell"""
    import mpmath as mp
    assert R.phi("matern12", np.zeros(1))[0] == 0.0 and XC.mp_phi("matern12", mp.mpf(0), mp) == 0
    with open(os.path.join(CSRC, "sgp_kernels.hip.h")) as f:
        assert "phi = r > 0.0 ? e / r : 0.0;" in f.read()
    c = XC.inputs("special_matern12_dout1")
    ell = R.full_ell(c["p"][1:], c["D"])
    for row, n in c["coincident"]:
        assert not np.any(XC.pair_factor_mp(c, row, n)) and not np.any(XC.pair_factor_f64(c, row, n))
    for row, n in c["near"]:
        u = XC.pair_factor_mp(c, row, n) * ell / c["p"][0]                       # sigma2 phi t / ell -> phi t
        assert abs(np.linalg.norm(u) - 1.0) < 1e-5
