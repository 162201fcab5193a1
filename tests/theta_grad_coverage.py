"""The cases of tests/test_gpu_theta_grad_coverage.py: the theta gradient's data half (k_theta_grad_uf<FAM, DO>) where its K loop is
split unevenly over blockIdx.z, at every (family, d_out) instantiation, at the point-block counts where the split changes, and with
data points on, next to and far from the inducing inputs (helper, no tests; imported by the GPU suite and by
tests/test_theta_grad_coverage_host.py, which holds the table to the launch arithmetic of csrc/sgp_api.hip).

Every case is (seed, spec) with spec = (N, M, D, d_out, family, one shared lengthscale, point weights, jitter, fresh); the seed is
the case's own, so that adding or removing a case leaves every other one as it is.  `fresh`: the objective is evaluated at the
sweep's own theta (nothing re-formed); otherwise at a new theta with q(v) held.  Problems, lengthscales and the device set-up are
those of tests/test_gpu_xu_grad.py; the restatement is tests/multi_theta_ref.py (d_out = 1: W is 1 x 1).
"""
import functools

import numpy as np

from tests import multi_theta_ref as R
from tests.test_gpu_xu_grad import COND_MAX, lengthscales, problem

TILE, GRID_TARGET = 64, 512
FAMILIES = ("se", "matern12", "matern32", "matern52")


def geometry(N, M):
    """(T, nblk, KS, slice lengths) of the data half's launch, restated from enqueue_theta_grad (csrc/sgp_api.hip), which owns KS,
    and k_theta_grad_uf (csrc/sgp_kernels.hip.h), which owns the slice bounds:

        KS = max(1, min(T, 512 / max(1, nblk * T)))        T = ceil(M / 64), nblk = ceil(N / 64)
        slice ks walks tile columns [T ks / KS, T (ks + 1) / KS)
    """
    T, nblk = -(-M // TILE), -(-N // TILE)
    KS = max(1, min(T, GRID_TARGET // max(1, nblk * T)))
    return T, nblk, KS, tuple(T * (ks + 1) // KS - T * ks // KS for ks in range(KS))


# ---- cases: name -> (seed, (N, M, D, d_out, family, one shared lengthscale, point weights, jitter, fresh)) ----
KIN40K, T3_KS2, T4_KS3, T5_KS4 = (500, 600), (3600, 130), (2100, 200), (1344, 260)
UNEVEN_CASES = {
    # the reference's own configuration: M = 600, minibatches of 500 (the last point block holds 52 points, 40 inducing rows are padded)
    "kin40k_m600_se": (9101, KIN40K + (8, 1, "se", False, False, 1e-8, False)),
    "kin40k_m600_se_fresh": (9102, KIN40K + (8, 1, "se", False, False, 1e-8, True)),
    "kin40k_m600_m52_dout4": (9103, KIN40K + (8, 4, "matern52", False, True, 1e-8, False)),
    # the smallest T with an uneven split (the last block holds 16 points, 62 rows are padded); D = 32: all 33 slots, the largest panels
    "t3_ks2_m32_dout2": (9104, T3_KS2 + (3, 2, "matern32", False, True, 1e-8, False)),
    "t3_ks2_se_D32": (9105, T3_KS2 + (32, 1, "se", False, True, 1e-8, False)),
    "t4_ks3_m12_dout3": (9106, T4_KS3 + (2, 3, "matern12", True, False, 1e-8, False)),
    "t5_ks4_m52_dout4": (9107, T5_KS4 + (5, 4, "matern52", False, True, 1e-8, False)),                 # the last block is full
}
# all 16 k_theta_grad_uf<FAM, DO> at one uneven shape; weights, shared / ARD and fresh / re-evaluated alternate over the pairs as in
# tests/test_gpu_xu_grad.py::test_every_family_and_output_count
EVERY_INST_CASES = {
    f"every_inst_{family}_dout{d}": (9200 + 10 * f + d, T4_KS3 + (6, d, family, d == 3, d != 2, 1e-8, d % 2 == 0))
    for f, family in enumerate(FAMILIES) for d in (1, 2, 3, 4)
}
# nblk 56 | 57 and 85 | 86 at T = 3: the two point counts across which the rule steps KS 3 -> 2 -> 1
BOUNDARY_M = 130
BOUNDARY_CASES = {
    f"boundary_N{N}": (9300 + i, (N, BOUNDARY_M, 3, 1, "matern52", False, True, 1e-8, False))
    for i, N in enumerate((3584, 3585, 5440, 5441))
}
# data points on, next to and far from inducing inputs (`with_special_points`); SE at D = 5: at D = 3 its K_uu is beyond COND_MAX
SPECIAL_CASES = {
    f"special_{family}_dout{d}": (9400 + 10 * f + d, T3_KS2 + (5 if family == "se" else 3, d, family, False, True, 1e-8, False))
    for f, family in enumerate(FAMILIES) for d in (1, 2)
}
CASES = {**UNEVEN_CASES, **EVERY_INST_CASES, **BOUNDARY_CASES, **SPECIAL_CASES}

# (N, M) at which the suite compared this gradient with a reference before these cases: every one has KS = 1 or KS = T
OLD_SHAPES = {
    "test_gpu_parity": [(600, 48), (2000, 200), (700, 70), (500, 64)],
    "test_gpu_dims, test_gpu_kernel_family": [(600, 48)],
    # N = nodes x (2 D + 1) cubature points, nodes = max(3 M, 150)
    "test_gpu_multi_theta": [(750, 48), (450, 20), (3168, 96), (21000, 200), (6600, 200), (1400, 48)],
    "test_gpu_envelope": [(3000, 4032), (420 * 9, 1008)],                        # (420 nodes of 2 x 4 + 1 cubature points)
}

# ---- the special points of SPECIAL_CASES (N = 3600: point block 0 is 0 .. 63, the partial last block 3584 .. 3599) ----
SPECIAL_ROWS = (3, 70, 129, 40, 100)                   # inducing rows from tile rows 0, 1, 2, 0, 1
COINCIDENT = (5, 700, 1500, 2500, 3590)                # X[n] = Xu[row]: r = 0
NEAR = (17, 800, 1600, 2600, 3595)                     # X[n] = Xu[row] + 1e-9 x a normal draw
FAR = (40, 900, 1700, 2700, 3599)                      # 60 lengthscales beyond the box in every dimension: SE K_uf is exactly 0
# 2000 lengthscales: K_uf is exactly 0 for every family (exp(-r) underflows past r = 746), k_theta_grad_uf's `kv != 0.0` branch
VERY_FAR = (50, 3597)
NEAR_SCALE, FAR_ELLS, VERY_FAR_ELLS = 1e-9, 60.0, 2000.0


def with_special_points(X, Xu, ell_max, rng):
    X = X.copy()
    rows = list(SPECIAL_ROWS)
    X[list(COINCIDENT)] = Xu[rows]
    X[list(NEAR)] = Xu[rows] + NEAR_SCALE * rng.normal(size=(len(rows), X.shape[1]))
    X[list(FAR)] = 1.7 + FAR_ELLS * ell_max
    X[list(VERY_FAR)] = -1.7 - VERY_FAR_ELLS * ell_max
    return X


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's inputs (arrays not to be written to).  `p_sweep` = (sigma2, ell...) of the sweep that gives q(v), `p` where the
    objective is evaluated: as tests/test_gpu_xu_grad.py::check_against_restatement takes them."""
    seed, (N, M, D, d_out, family, iso, weighted, jitter, fresh) = CASES[name]
    X, om, Y, Xu, W = problem(N, M, D, d_out, seed=seed, weighted=weighted)
    n_ell = 1 if iso else D
    ell0 = lengthscales(M, D, n_ell)
    p_sweep = np.concatenate([[0.9], ell0])
    p = p_sweep if fresh else np.concatenate([[1.05], ell0 * np.linspace(1.05, 0.95, n_ell)])
    if name in SPECIAL_CASES:
        X = with_special_points(X, Xu, max(p_sweep[1:].max(), p[1:].max()), np.random.default_rng(seed + 50000))
    return dict(name=name, N=N, M=M, D=D, d_out=d_out, family=family, n_ell=n_ell, weighted=weighted, jitter=jitter, fresh=fresh,
                X=X, om=om, omega=np.ones(N) if om is None else om, Y=Y, Xu=Xu, W=W, p_sweep=p_sweep, p=p,
                special=name in SPECIAL_CASES)


def kuu_cond(c, p=None):
    p = c["p"] if p is None else p
    Kuu = R.kernelmatrix(c["family"], p[0], R.full_ell(p[1:], c["D"]), c["Xu"])
    return np.linalg.cond(Kuu + c["jitter"] * np.eye(c["M"]))


def reference(c, mu, Sig, p=None):
    """(value, gradient) of the restatement at p (default: the case's) with q(v) = N(mu, Sig); asserts what the comparison rests on:
    cond(K_uu + jitter I) < COND_MAX, and K_uf exactly 0 where the case says so."""
    p = c["p"] if p is None else p
    cond = kuu_cond(c, p)
    assert cond < COND_MAX, f"{c['name']}: the inputs leave K_uu ill-conditioned ({cond:.1e}): it would compare rounding"
    if c["special"]:
        Kuf = R.kernelmatrix(c["family"], p[0], R.full_ell(p[1:], c["D"]), c["Xu"], c["X"])
        assert not np.any(Kuf[:, list(VERY_FAR)])
        assert c["family"] != "se" or not np.any(Kuf[:, list(FAR)])
        assert np.all(Kuf[list(SPECIAL_ROWS), list(COINCIDENT)] == p[0])
    args = (p[0], p[1:], c["X"], c["omega"], c["Y"], Sig + np.outer(mu, mu), mu, c["W"], c["Xu"], c["jitter"], c["family"])
    return R.batched_objective(*args), R.analytic_grad(*args, n_ell=c["n_ell"])


def grad_ratio(grad, ref):
    """error / bound of a gradient under rtol 1e-6, atol 1e-9 max|g_ref| (tests/test_gpu_xu_grad.py, tests/test_gpu_multi_theta.py)"""
    return float((np.abs(grad - ref) / (1e-6 * np.abs(ref) + 1e-9 * np.abs(ref).max())).max())
