"""The cases of tests/test_gpu_xu_grad_coverage.py: the inducing-input gradient's data half (k_xu_grad_uf<FAM, DO>) where a workgroup
walks several point blocks at T >= 3 -- the `xs` panel over the next block's A panel, `sums[wc]` carried in LDS, a short last range --
at every (family, d_out) instantiation, across the point count where the range length steps, and with data points on, next to and far
from inducing inputs, where phi multiplies the difference itself (helper, no tests; imported by the GPU suite and by
tests/test_xu_grad_coverage_host.py, which holds the table to the launch arithmetic of csrc/sgp_api.hip).

Every case is (seed, spec) with spec = (N, M, D, d_out, family, one shared lengthscale, point weights, jitter, fresh), as in
tests/theta_grad_coverage.py; the seed is the case's own.  Problems, lengthscales and the device set-up are those of
tests/test_gpu_xu_grad.py; the restatement is tests/xu_grad_ref.py.

The bound is the project's gradient bound (rtol 1e-6, atol 1e-9 max|ref|) plus one input-rounding term over the near pairs.  The
device forms t_d = fl(x_d / ell_d) - fl(z_d / ell_d); with |x - z| << |x| its absolute error is delta_d <= 2 eps (|x_d| + |z_d|) /
ell_d whatever the difference, and dk/dz_md = sigma2 phi(r) t_d / ell_d moves by

    sigma2 [ phi(r) delta_d + |phi'(r)| |t_d| sum_e |t_e| delta_e / r ] / ell_d          (first order; r = |t|)

For Matern-1/2, phi = e^-r / r makes phi t a unit vector next to the kink, so this is sigma2 delta / (r ell): 1e-6 of the entry at
|x - z| = 1e-9.  For the other families and at 1e-6 it is far below the base bound.  XU_C_BOUND, the constant in front, was settled on
the CPU alone (tests/test_xu_grad_coverage_host.py::test_the_scaled_coordinate_route_stays_inside_the_bound; recorded in
profiles/xu_grad_coverage.txt): a float64 restatement that subtracts scaled coordinates as the device does, against the reference
below, whose near and coincident pairs come from mpmath on the direct differences.  The device's output never took part.
"""
import functools
import math

import numpy as np

from tests import multi_theta_ref as R
from tests.test_gpu_xu_grad import COND_MAX, lengthscales, problem
from tests.xu_grad_ref import analytic_grad_xu

TILE, WG_TARGET = 64, 256
FAMILIES = ("se", "matern12", "matern32", "matern52")
EPS = float(np.finfo(np.float64).eps)
XU_C_BOUND = 1.0            # worst ratio of the scaled-coordinate route at 1.0: see profiles/xu_grad_coverage.txt (<= 0.5: a factor 2 to spare)
MP_DIGITS = 60


def geometry(N, M):
    """(T, nblk, range_len, nranges, blocks in the last range, points in the last block) of the data half's launch, restated from
    xu_ranges (csrc/sgp_api.hip), which owns the ranges, and k_xu_grad_uf (csrc/sgp_kernels.hip.h), which owns a range's bounds:

        want = min(nblk, max(1, 256 / T))   range_len = ceil(nblk / want)   nranges = ceil(nblk / range_len)
        range g walks point blocks [g range_len, min(nblk, (g + 1) range_len))               T = ceil(M / 64), nblk = ceil(N / 64)
    """
    T, nblk = -(-M // TILE), -(-N // TILE)
    want = max(1, min(nblk, max(1, WG_TARGET // T)))
    range_len = -(-nblk // want)
    nranges = -(-nblk // range_len)
    b0 = (nranges - 1) * range_len
    return T, nblk, range_len, nranges, min(nblk, b0 + range_len) - b0, N - (nblk - 1) * TILE


def range_blocks(N, M):
    """[(b0, b1)] of every range, in launch order"""
    _, nblk, range_len, nranges, _, _ = geometry(N, M)
    return [(g * range_len, min(nblk, (g + 1) * range_len)) for g in range(nranges)]


# ---- cases: name -> (seed, (N, M, D, d_out, family, one shared lengthscale, point weights, jitter, fresh)) ----
M600_LEN2, M600_SHORT, M600_LEN3, T3_LEN2, T4_LEN2 = (1601, 600), (1700, 600), (3201, 600), (5500, 130), (4130, 200)
LONG_CASES = {
    # T 10: 13 ranges of 2, the last block holds one point
    "m600_len2": (9501, M600_LEN2 + (8, 1, "se", False, True, 1e-8, False)),
    "m600_len2_fresh": (9502, M600_LEN2 + (8, 1, "se", False, True, 1e-8, True)),
    # 14 ranges, the last of one block of 36 points
    "m600_short_last": (9503, M600_SHORT + (8, 4, "matern52", False, True, 1e-8, False)),
    # 17 ranges of 3, the last block holds one point
    "m600_len3": (9504, M600_LEN3 + (8, 2, "matern32", False, True, 1e-8, False)),
    # T 3, D 32: the full 16 KB `sums` halves carried over two blocks
    "t3_len2_D32": (9505, T3_LEN2 + (32, 1, "se", False, True, 1e-8, False)),
}
# nblk 85 | 86 at T = 3: 85 ranges of 1 | 43 ranges of 2, the step of the rule
BOUNDARY_M = 130
BOUNDARY_CASES = {
    f"boundary_N{N}": (9510 + i, (N, BOUNDARY_M, 3, 1, "matern52", False, True, 1e-8, False)) for i, N in enumerate((5440, 5441))
}
# all 16 k_xu_grad_uf<FAM, DO> at T 4, 33 ranges of 2, the last of one block of 34 points; weights, shared / ARD and fresh /
# re-evaluated alternate over the pairs as in tests/test_gpu_xu_grad.py::test_every_family_and_output_count
EVERY_INST_CASES = {
    f"every_inst_{family}_dout{d}": (9600 + 10 * f + d, T4_LEN2 + (6, d, family, d == 3, d != 2, 1e-8, d % 2 == 0))
    for f, family in enumerate(FAMILIES) for d in (1, 2, 3, 4)
}
# data points on, next to and far from inducing inputs; SE at D = 5: at D = 3 its K_uu is beyond COND_MAX (tests/theta_grad_coverage.py)
# The seeds: 9700 + 10 f + d + 100 k with the smallest k at which, on the CPU, a reference without the coincident and near pairs misses
# the bound tenfold in their rows (tests/test_xu_grad_coverage_host.py).  For Matern-1/2 every seed does (phi t is a unit vector); for
# the smooth families the pair's term is 1e-6 |A_mn| sigma2 phi / ell^2 and has to meet a small entry of the row.
SPECIAL_SEEDS = {("se", 1): 13401, ("se", 2): 10402, ("matern12", 1): 9711, ("matern12", 2): 9712,
                 ("matern32", 1): 9921, ("matern32", 2): 9822, ("matern52", 1): 10431, ("matern52", 2): 9932}
SPECIAL_CASES = {
    f"special_{family}_dout{d}": (SPECIAL_SEEDS[family, d], T3_LEN2 + (5 if family == "se" else 3, d, family, False, True, 1e-8, False))
    for family in FAMILIES for d in (1, 2)
}
GEOMETRY_CASES = {**LONG_CASES, **BOUNDARY_CASES, **EVERY_INST_CASES}
CASES = {**GEOMETRY_CASES, **SPECIAL_CASES}

# (N, M) at which the suite compared grad_xu with a reference before these cases (tests/test_gpu_xu_grad.py: SHAPES, every family and
# output count, central differences, optimize_inducing; tests/test_gpu_theta_grad_coverage.py: XU_CASES)
OLD_SHAPES = {
    "test_gpu_xu_grad": [(1, 17), (64, 70), (130, 128), (130, 70), (130, 17), (64, 128), (65, 17), (8193, 128), (8193, 70), (60, 5),
                         (200, 12)],
    "test_gpu_theta_grad_coverage": [(500, 600), (1344, 260)],
}

# ---- the special points of SPECIAL_CASES.  N = 5500, T = 3: 43 ranges of 2 point blocks, block b = points 64 b .. 64 b + 63; an even
# ---- block is the first of its range, an odd one the second; the last block, 85, holds 5440 .. 5499.
# Each kind: one point in the first block of a range, one in the second block of a range, one in the last block; the coincident and
# the near points' inducing rows come from tile rows 0, 1 and 2 (rows 128 and 129 are all of tile row 2).
COINCIDENT = ((3, 5), (70, 21 * 64 + 7), (129, 5450))              # (inducing row, point): X[n] = Xu[row], r = 0
NEAR_1E6 = ((40, 2 * 64 + 17), (100, 33 * 64 + 20), (128, 5460))   # X[n] = Xu[row] + 1e-6 x a normal draw
NEAR_1E9 = ((20, 4 * 64 + 30), (110, 45 * 64 + 3), (129, 5470))    # X[n] = Xu[row] + 1e-9 x a normal draw
FAR = (6 * 64 + 40, 57 * 64 + 11, 5480)                            # 60 lengthscales beyond the box in every dimension
VERY_FAR = (8 * 64 + 50, 69 * 64 + 1, 5490)                        # 2000 lengthscales: exp underflows, K_uf is exactly 0 for every family
FAR_ELLS, VERY_FAR_ELLS = 60.0, 2000.0


def with_special_points(X, Xu, ell_max, rng):
    X = X.copy()
    for row, n in COINCIDENT:
        X[n] = Xu[row]
    for scale, pairs in ((1e-6, NEAR_1E6), (1e-9, NEAR_1E9)):
        for row, n in pairs:
            X[n] = Xu[row] + scale * rng.normal(size=X.shape[1])
    X[list(FAR)] = 1.7 + FAR_ELLS * ell_max
    X[list(VERY_FAR)] = -1.7 - VERY_FAR_ELLS * ell_max
    return X


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's inputs (arrays not to be written to).  `p_sweep` = (sigma2, ell...) of the sweep that gives q(v), `p` where the
    objective is evaluated: as tests/test_gpu_xu_grad.py::check_against_restatement takes them.  `coincident`, `near`: (row, point)
    pairs; `far`, `very_far`: points (all empty but for SPECIAL_CASES)."""
    seed, (N, M, D, d_out, family, iso, weighted, jitter, fresh) = CASES[name]
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=seed, weighted=weighted)
    n_ell = 1 if iso else D
    ell0 = lengthscales(M, D, n_ell)
    p_sweep = np.concatenate([[0.9], ell0])
    p = p_sweep if fresh else np.concatenate([[1.05], ell0 * np.linspace(1.05, 0.95, n_ell)])
    special = name in SPECIAL_CASES
    if special:
        X = with_special_points(X, Xu, max(p_sweep[1:].max(), p[1:].max()), np.random.default_rng(seed + 50000))
    return dict(name=name, N=N, M=M, D=D, d_out=d_out, family=family, n_ell=n_ell, weighted=weighted, jitter=jitter, fresh=fresh,
                X=X, om=om, omega=np.ones(N) if om is None else om, Y=Y, Xu=Xu, W=W, p_sweep=p_sweep, p=p, special=special,
                coincident=COINCIDENT if special else (), near=NEAR_1E6 + NEAR_1E9 if special else (),
                far=FAR if special else (), very_far=VERY_FAR if special else ())


def kuu_cond(c, p=None):
    p = c["p"] if p is None else p
    Kuu = R.kernelmatrix(c["family"], p[0], R.full_ell(p[1:], c["D"]), c["Xu"])
    return np.linalg.cond(Kuu + c["jitter"] * np.eye(c["M"]))


def special_rows(c):
    return sorted({row for row, _ in tuple(c["coincident"]) + tuple(c["near"])})


# ---- the data half, point by point ----
def coefficients(c, mu, Sig, cols):
    """A[:, cols] of tests/xu_grad_ref.py: A_mn = omega_n (G k_n)_m - sum_d mu^(d)_m (omega_n W y_n)_d, G = S - tr(W) Kinv."""
    p, M, D, d = c["p"], c["M"], c["D"], c["d_out"]
    cols = np.asarray(cols, dtype=np.int64)
    ellf = R.full_ell(p[1:], D)
    W = np.atleast_2d(c["W"])
    Kinv = np.linalg.inv(R.kernelmatrix(c["family"], p[0], ellf, c["Xu"]) + c["jitter"] * np.eye(M))
    G = R.sum_rv_wbar(Sig + np.outer(mu, mu), W, M) - np.trace(W) * Kinv
    om = c["omega"][cols]
    Kuf = R.kernelmatrix(c["family"], p[0], ellf, c["Xu"], c["X"][cols])
    return (G @ Kuf) * om - mu.reshape(d, M).T @ (W @ (om[:, None] * c["Y"][cols].reshape(len(cols), d)).T)


def uf_terms(c, mu, Sig, cols):
    """The data half of analytic_grad_xu summed over the points `cols` alone, (M, D): what a kernel that skipped them would lose."""
    p, D = c["p"], c["D"]
    cols = np.asarray(cols, dtype=np.int64)
    if cols.size == 0:
        return np.zeros((c["M"], D))
    ellf = R.full_ell(p[1:], D)
    X = c["X"][cols]
    Z = coefficients(c, mu, Sig, cols) * (p[0] * R.phi(c["family"], R.scaled_sq_dist(ellf, c["Xu"], X)))
    return np.stack([np.sum(Z * (X[None, :, k] - c["Xu"][:, k:k + 1]), axis=1) / ellf[k] ** 2 for k in range(D)], axis=1)


def mp_phi(family, r, mp):
    """phi(r) of fam_kappa_phi in mpmath (Matern-1/2: 0 at r = 0, the kernel's convention)"""
    if family == "se":
        return mp.exp(-r * r / 2)
    if family == "matern12":
        return mp.exp(-r) / r if r > 0 else mp.mpf(0)
    if family == "matern32":
        return 3 * mp.exp(-mp.sqrt(3) * r)
    a = mp.sqrt(5) * r
    return mp.mpf(5) / 3 * (1 + a) * mp.exp(-a)


def abs_dphi(family, r):
    """|phi'(r)|, float64 (r > 0)"""
    if family == "se":
        return r * math.exp(-0.5 * r * r)
    if family == "matern12":
        return math.exp(-r) * (1.0 + r) / (r * r)
    if family == "matern32":
        return 3.0 * math.sqrt(3.0) * math.exp(-math.sqrt(3.0) * r)
    a = math.sqrt(5.0) * r
    return (5.0 / 3.0) * math.sqrt(5.0) * a * math.exp(-a)


def pair_factor_mp(c, row, n):
    """sigma2 phi(r) (x_d - z_d) / ell_d^2 of one (row, point) pair from the direct differences at MP_DIGITS digits, rounded to float64
    (D,): the float64 route divides by an r formed from scaled coordinates and loses eps |x| / |x - z| of it"""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        ell = [mp.mpf(float(e)) for e in R.full_ell(c["p"][1:], c["D"])]
        q = [mp.mpf(float(c["X"][n, d])) - mp.mpf(float(c["Xu"][row, d])) for d in range(c["D"])]
        r = mp.sqrt(sum((q[d] / ell[d]) ** 2 for d in range(c["D"])))
        f = mp.mpf(float(c["p"][0])) * mp_phi(c["family"], r, mp)
        return np.array([float(f * q[d] / ell[d] ** 2) for d in range(c["D"])])


def pair_factor_f64(c, row, n):
    """the same factor as analytic_grad_xu forms it"""
    ellf = R.full_ell(c["p"][1:], c["D"])
    s = R.scaled_sq_dist(ellf, c["Xu"][row:row + 1], c["X"][n:n + 1])[0, 0]
    return c["p"][0] * float(R.phi(c["family"], s)) * (c["X"][n] - c["Xu"][row]) / ellf ** 2


def pair_factor_scaled(c, row, n):
    """the same factor as the device forms it: t_d = fl(x_d / ell_d) - fl(z_d / ell_d) with 1 / ell_d rounded first, s = sum t_d^2,
    sigma2 phi(sqrt s) t_d / ell_d"""
    inv = 1.0 / R.full_ell(c["p"][1:], c["D"])
    t = c["X"][n] * inv - c["Xu"][row] * inv
    return c["p"][0] * float(R.phi(c["family"], float(np.sum(t * t)))) * t * inv


def substituted(c, mu, Sig, g, pairs, factor):
    """g with the (row, point) pairs' data-half terms replaced by A_mn factor(c, row, n)"""
    g = g.copy()
    if pairs:
        A = coefficients(c, mu, Sig, [n for _, n in pairs])
        for j, (row, n) in enumerate(pairs):
            g[row] += A[row, j] * (factor(c, row, n) - pair_factor_f64(c, row, n))
    return g


def rounding_term(c, mu, Sig):
    """The input-rounding term of `bound`, (M, D): over the near pairs
        |A_mn| sigma2 [ phi(r) delta_d + |phi'(r)| |t_d| sum_e |t_e| delta_e / r ] / ell_d,  delta_d = 2 eps (|x_d| + |z_d|) / ell_d
    with t and r from the direct differences (exact in float64: x - z by Sterbenz)."""
    term = np.zeros((c["M"], c["D"]))
    if not c["near"]:
        return term
    ellf = R.full_ell(c["p"][1:], c["D"])
    A = coefficients(c, mu, Sig, [n for _, n in c["near"]])
    for j, (row, n) in enumerate(c["near"]):
        x, z = c["X"][n], c["Xu"][row]
        t = (x - z) / ellf
        r = float(np.sqrt(np.sum(t * t)))
        delta = 2.0 * EPS * (np.abs(x) + np.abs(z)) / ellf
        ph = float(R.phi(c["family"], r * r))
        term[row] += abs(A[row, j]) * c["p"][0] * (ph * delta + abs_dphi(c["family"], r) * np.abs(t) * float(np.abs(t) @ delta) / r) / ellf
    return term


def reference(c, mu, Sig):
    """grad_xu of the restatement at the case's p with q(v) = N(mu, Sig), (M, D); the coincident and near pairs' factors come from
    mpmath.  Asserts what the comparison rests on: cond(K_uu + jitter I) < COND_MAX, K_uf exactly 0 at the very-far points and
    exactly sigma2 at the coincident pairs."""
    p = c["p"]
    cond = kuu_cond(c)
    assert cond < COND_MAX, f"{c['name']}: the inputs leave K_uu ill-conditioned ({cond:.1e}): it would compare rounding"
    if c["special"]:
        Kuf = R.kernelmatrix(c["family"], p[0], R.full_ell(p[1:], c["D"]), c["Xu"], c["X"])
        assert not np.any(Kuf[:, list(c["very_far"])])
        assert c["family"] != "se" or not np.any(Kuf[:, list(c["far"])])
        assert all(Kuf[row, n] == p[0] for row, n in c["coincident"])
    g = analytic_grad_xu(p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"], c["family"])
    return substituted(c, mu, Sig, g, tuple(c["coincident"]) + tuple(c["near"]), pair_factor_mp)


def bound(c, ref, term=None):
    """(M, D): rtol 1e-6, atol 1e-9 max|ref| (tests/test_gpu_xu_grad.py), plus XU_C_BOUND x the input-rounding term (`rounding_term`,
    computed from the reference's quantities; all zeros where the case has no near pair)"""
    base = 1e-6 * np.abs(ref) + 1e-9 * np.abs(ref).max()
    return base if term is None else base + XU_C_BOUND * term


def ratio(got, ref, bnd, rows=None):
    """max error / bound, over all entries or the inducing rows `rows` alone"""
    q = np.abs(got - ref) / bnd
    return float((q if rows is None else q[list(rows)]).max())
