"""Greedy inducing-input selection restated in NumPy (helper, no tests): the reference of tests/test_select_inducing_host.py and
tests/test_gpu_select_inducing.py, and the cases the two share.

The algorithm is the partial pivoted Cholesky factorisation of K_ff that include/sgp_hip.h states for sgp_select_inducing:
    d_i = sigma2, trace[0] = n sigma2; at step j: p_j = the lowest index among the largest stored d_i,
    c_j[i] = (k(x_i, x_p) - sum_{l<j} c_l[i] c_l[p]) / sqrt(d_p),  d_i <- d_i - c_j[i]^2,  d_p <- 0,  trace[j+1] = sum_i d_i,
stopping before step j when trace[j] <= tol trace[0] or max_i d_i <= min_var sigma2.  The sum over l is taken in the library's order
-- l = w, w + 4, ... ascending for w = 0 .. 3, then (s_0 + s_1) + (s_2 + s_3) -- though without fused multiply-adds, and the squared
distance over d ascending on inputs scaled by 1 / ell once.  Nothing here is written to agree with the device to the last bit: the
GPU suite compares picks only where the top two residuals are far apart (the gap condition of the host suite)."""
from collections import namedtuple

import numpy as np

SQRT3, SQRT5 = 1.7320508075688772935, 2.2360679774997896964
FAMILIES = ("se", "matern12", "matern32", "matern52")
SEL_TILE, SEL_FOLD_THREADS, SEL_RED_MAX = 64, 256, 512        # the device's tile, fold width and reduce threshold


def kappa(family, s):
    """k / sigma2 at the squared scaled distance s (any float dtype)"""
    one = s.dtype.type(1)
    if family == "se":
        return np.exp(-s / 2)
    r = np.sqrt(s)
    if family == "matern12":
        return np.exp(-r)
    if family == "matern32":
        a = s.dtype.type(3) ** s.dtype.type(0.5) * r
        return (one + a) * np.exp(-a)
    if family == "matern52":
        a = s.dtype.type(5) ** s.dtype.type(0.5) * r
        return (one + a + s.dtype.type(5) * s / s.dtype.type(3)) * np.exp(-a)
    raise ValueError(family)


def scaled(X, ell, dtype=np.float64):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64).reshape(-1), (X.shape[1],))
    return X.astype(dtype) * (dtype(1) / ell.astype(dtype))


def kernel_column(Xs, p, family, sigma2):
    s = np.zeros(len(Xs), dtype=Xs.dtype)
    for d in range(Xs.shape[1]):                              # over d ascending
        t = Xs[:, d] - Xs[p, d]
        s = s + t * t
    return Xs.dtype.type(sigma2) * kappa(family, s)


def kernel_matrix(X, Z, family, sigma2, ell):
    A, B = scaled(X, ell), scaled(Z, ell)
    s = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return sigma2 * kappa(family, s)


Selection = namedtuple("Selection", "idx trace gaps count resid")


def greedy_select(X, family, sigma2, ell, m, tol=0.0, min_var=1e-12, *, dtype=np.float64, pivots=None, keep_resid=False):
    """(idx, trace, gaps, count, resid).  idx (m,) int64 with -1 behind `count`; trace (m + 1,) float64 with NaN behind trace[count];
    gaps[j] = (largest - second-largest DISTINCT residual) / largest in front of step j (inf where all candidates tie).
    pivots: take these picks instead of the argmax (the stop rules still apply).  keep_resid: resid[j] = the residuals d the pick of
    step j was made from, j = 0 .. count (the last row: after the last step)."""
    Xs = scaled(X, ell, dtype)
    n = len(Xs)
    m = int(m)
    one = dtype(1)
    d = np.full(n, dtype(sigma2))
    C = np.zeros((m, n), dtype=dtype)
    idx = np.full(m, -1, dtype=np.int64)
    trace = np.full(m + 1, np.nan)
    gaps = np.full(m, np.nan)
    resid = []
    tr0 = tr = dtype(n) * dtype(sigma2)
    count = m
    for j in range(m + 1):
        trace[j] = float(tr)
        if keep_resid:
            resid.append(d.copy())
        if j == m:
            break
        dmax = d.max()
        if tr <= dtype(tol) * tr0 or dmax <= dtype(min_var) * dtype(sigma2):
            count = j
            break
        lower = d[d < dmax]
        gaps[j] = float((dmax - lower.max()) / dmax) if lower.size else np.inf
        p = int(np.flatnonzero(d == dmax)[0]) if pivots is None else int(pivots[j])      # the lowest index among the largest
        cp = C[:j, p].copy()
        part = [np.add.reduce(C[w:j:4] * cp[w:j:4, None], axis=0) if w < j else np.zeros(n, dtype=dtype) for w in range(4)]
        dot = (part[0] + part[1]) + (part[2] + part[3])
        c = (kernel_column(Xs, p, family, sigma2) - dot) / np.sqrt(d[p])
        C[j] = c
        d = d - c * c
        d[p] = 0 * one
        idx[j] = p
        tr = d.sum()
    return Selection(idx, trace, gaps, count, np.array(resid) if keep_resid else None)


def greedy_select_longdouble(X, family, sigma2, ell, m, tol=0.0, min_var=1e-12, **kw):
    """the same loop in np.longdouble"""
    return greedy_select(X, family, sigma2, ell, m, tol, min_var, dtype=np.longdouble, **kw)


def dense_trace(X, picks, family, sigma2, ell):
    """tr(K_ff - K_fZ K_ZZ^-1 K_Zf) of Z = X[picks], and cond(K_ZZ)"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    if len(picks) == 0:
        return len(X) * sigma2, 1.0
    Kzz = kernel_matrix(X[picks], X[picks], family, sigma2, ell)
    Kfz = kernel_matrix(X, X[picks], family, sigma2, ell)
    return len(X) * sigma2 - np.sum(Kfz * np.linalg.solve(Kzz, Kfz.T).T), np.linalg.cond(Kzz)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name, family, n, D, m, ard (one lengthscale per dimension), seed, sigma2, the isotropic lengthscale the ARD ones spread around
Case = namedtuple("Case", "name family n D m ard seed sigma2 ell0")


def case_data(c):
    """X (n, D) uniform in [-1, 1]^D and the lengthscale(s) of a case"""
    rng = np.random.default_rng(1000 + c.seed)
    X = rng.uniform(-1.0, 1.0, (c.n, c.D))
    ell = c.ell0 * (rng.uniform(0.7, 1.4, c.D) if c.ard else np.ones(1))
    return X, ell


# Index-for-index parity.  n covers 1, 63 / 64 / 65 (one workgroup of SEL_TILE = 64 candidates, full, and the first point of a second
# one), 257, 1000, 4099; 16385 = 256 * 64 + 1 (257 partials: a thread of the fold takes a second one), 32768 and 32769 (512 partials:
# the last count the step kernel folds itself; 513: the first with the reduce launch in between); m covers 1, 2, 65, 130 (the sum
# over l: each wave's unrolled groups of four, their remainders, and more than one group) and n itself where n <= 257.  The
# lengthscales keep K_ZZ of the picks well conditioned, so the residuals the picks are made from stay far above rounding.
PARITY_CASES = [
    Case("n1", "se", 1, 2, 1, False, 0, 0.8, 1.0),
    Case("n63_all", "matern32", 63, 1, 63, False, 0, 1.3, 0.3),
    Case("n64_all", "se", 64, 8, 64, True, 0, 0.7, 1.2),
    Case("n65_m2", "matern12", 65, 8, 2, True, 0, 2.0, 2.0),
    Case("n65_all", "matern52", 65, 2, 65, False, 0, 1.1, 0.3),
    Case("n257_all", "matern12", 257, 2, 257, False, 0, 0.9, 1.0),
    Case("n257_m130", "matern52", 257, 32, 130, True, 0, 1.0, 4.0),
    Case("n1000_m65", "matern12", 1000, 1, 65, False, 0, 1.5, 0.5),
    Case("n1000_m130", "se", 1000, 32, 130, False, 0, 1.0, 4.0),
    Case("n1000_m1", "matern32", 1000, 2, 1, True, 0, 0.6, 0.5),
    Case("n4099_m65", "matern32", 4099, 8, 65, True, 1, 1.2, 1.5),
    Case("n4099_m130", "matern12", 4099, 2, 130, True, 0, 0.8, 0.7),
    Case("n16385_m9", "matern52", 16385, 8, 9, False, 0, 1.0, 1.5),
    Case("n32768_m6", "se", 32768, 2, 6, False, 0, 1.0, 0.5),
    Case("n32769_m6", "matern12", 32769, 8, 6, True, 0, 1.4, 2.0),
]
GAP_MIN = 1e-6                                                # the least top-two gap of every case above, at every step

# stop rules: (case, tol, min_var); the tol lies between two trace values of the case (host suite: not within 1e-6 of either)
TOL_CASE = (Case("tol", "matern12", 1000, 2, 130, True, 0, 0.8, 0.7), 0.3, 0.0)
MINVAR_CASE = (Case("min_var", "se", 257, 1, 130, False, 0, 1.0, 0.6), 0.0, 1e-6)

# cross-check against the sweep's sum_I1: cond(K_ZZ) <= 1e6 (host suite)
SWEEP_CASES = [
    Case("sweep_se", "se", 1000, 2, 40, True, 0, 0.8, 0.5),
    Case("sweep_m52", "matern52", 600, 8, 130, False, 0, 1.2, 1.5),
]
SWEEP_COND_MAX = 1e6

# two more comparisons of picks index for index in the GPU suite, held to the gap condition like the parity cases: the valid call
# behind the refusals, and train.select_inducing (the kernel comes from raw theta: the lengthscales of the case through
# invsoftplus and back through the softplus the library's Python layer applies)
REFUSAL_CASE = Case("refusals", "se", 50, 3, 5, False, 2, 1.0, 1.0)
TRAIN_CASE = Case("train", "matern52", 700, 2, 30, True, 4, 0.8, 0.7)
INDEX_CASES = PARITY_CASES + [REFUSAL_CASE, TRAIN_CASE]


def train_case_inputs(case=TRAIN_CASE):
    """X, raw theta (sigma2 first) and p = softplus(theta), the kernel values train.select_inducing sets"""
    X, ell = case_data(case)
    p0 = np.concatenate([[case.sigma2], ell])
    theta = p0 + np.log(-np.expm1(-p0))
    return X, theta, np.maximum(theta, 0.0) + np.log1p(np.exp(-np.abs(theta)))


# greedy validity, where near-ties may occur
VALIDITY_CASE = Case("validity", "se", 20000, 8, 256, False, 0, 1.0, 1.5)
# E = max_j max_i |d_float64 - d_longdouble| / sigma2 of this module's two loops along the float64 picks of VALIDITY_CASE.
# The host suite measures it again and holds the stored bound to it; tests/test_gpu_select_inducing.py allows 8 E sigma2 (a different
# summation order and exp's last bit).
VALIDITY_E_MEASURED = 1.107e-15
VALIDITY_E = 2e-15


def validity_error(case=VALIDITY_CASE):
    """E of `case`, measured now"""
    X, ell = case_data(case)
    a = greedy_select(X, case.family, case.sigma2, ell, case.m, 0.0, 0.0, keep_resid=True)
    b = greedy_select_longdouble(X, case.family, case.sigma2, ell, case.m, 0.0, 0.0, pivots=a.idx, keep_resid=True)
    return float(np.max(np.abs(a.resid.astype(np.longdouble) - b.resid)) / case.sigma2)


# ---- the ledger of exported names --------------------------------------------------------------------------------------------
# tests/call_sequence_ref.ENTRY_POINTS classifies every exported sgp_* name (tests/test_call_sequences_host.py holds it to the header).
# sgp_select_inducing reads the handle's kernel and writes nothing of the handle, so it is a reader; what stands behind the
# class is tests/test_gpu_select_inducing.py::test_a_selection_changes_nothing_of_the_handle.  Its entry is made here, in the
# module both selection suites import, and so is present whenever the suite is collected.
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_select_inducing", CR.READER)


register_entry_point()
