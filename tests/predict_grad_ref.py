"""NumPy restatement of the predictive derivatives at test inputs (sgp_predict_grad), independent of the other reference modules:
its own kernel functions, cases and error bounds, shared by tests/test_predict_grad_host.py and tests/test_gpu_predict_grad.py.

With k = k(Xu, x), J = dk/dx (M x D), Kinv = (K_uu + jitter I)^-1, q(v) = N(mu_v, Sigma_v), block (i, j) of Sigma_v written
Sigma^(ij), and A_ij = Sigma^(ij) - delta_ij Kinv:
    k_m = sigma2 g(s_m),  s_m = sum_d ((x_d - u_md) / ell_d)^2,  J_md = 2 sigma2 g'(s_m) (x_d - u_md) / ell_d^2
    mean[o]              = k' mu^(o)
    jac[o, d]            = J_d' mu^(o)
    var[i, j]            = delta_ij sigma2 + k' A_ij k
    var_grad[i, j, d]    = J_d' A_ij k + k' A_ij J_d
    jac_cov[(i,d),(j,e)] = delta_ij delta_de c_fam sigma2 / ell_d^2 + J_d' A_ij J_e,   c_fam = -2 g'(0)
Three routes: "inverse" (float64, the explicit inverse), "cholesky" (float64, every product with Kinv a pair of triangular solves)
and "longdouble" (the panel, the factorisation and every contraction in np.longdouble: 11 more bits, rounded once at the end).

Bounds (`bounds`): a constant times eps times the sum of the absolute terms of each contraction.  A panel entry carries the
conditioning of its exponential, (1 + s_m / 2) roundings: pk = (1 + s / 2) |k|, pJ = (1 + s / 2) |J|.  A product with Kinv carries
cond(K_uu + jitter I), the relative error of an inverse formed from a Cholesky factor; the forms of var, which the device takes
through the factors of K_uu and Sigma_v, carry cond(Sigma_v) on their Sigma half:
    mean      C eps pk' |mu^(o)|
    jac       C eps pJ_d' |mu^(o)|
    var       C eps [delta_ij (sigma2 + cond_K pk' |Kinv| pk) + cond_S pk' |Sigma^(ij)| pk]
    var_grad  C eps [pJ_d' |Sigma^(ij)| pk + pk' |Sigma^(ij)| pJ_d + 2 delta_ij cond_K pJ_d' |Kinv| pk]
    jac_cov   C eps [delta_ij delta_de c_fam sigma2 / ell_d^2 + pJ_d' |Sigma^(ij)| pJ_e + delta_ij cond_K pJ_d' |Kinv| pJ_e]
C = C_BOUND = 20, the constant of tests/in_message_grad_ref.py, whose U = A [k | J] product and wavefront contraction this call
shares.  It was held on the CPU alone: tests/test_predict_grad_host.py measures the spread between the float64 routes and the
longdouble route over SPREAD_CASES in units of the bound at C = 1 and asserts that C_BOUND leaves a factor 4 above the worst of
them (the margin for another summation order: matrix-core tiles, fused multiply-adds, a 64-lane butterfly).  The device's output
never took part in choosing it."""
import functools
import math

import numpy as np

EPS = np.finfo(np.float64).eps
C_BOUND = 20.0
SIGMA2 = 0.8
FAMILIES = ("se", "matern32", "matern52")
C_FAM = {"se": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0}
SHARP_JITTER = 1e-3                       # cond(K_uu + jitter I) <= sigma2 M / jitter ~ 1e5: every entry is compared at 1e-9 or less


def g01(family, s):
    """(g, g') of k = sigma2 g(s) at s = r^2, in the dtype of s"""
    s = np.asarray(s)
    one = s.dtype.type(1)
    if family == "se":
        e = np.exp(-s / 2)
        return e, -e / 2
    r = np.sqrt(s)
    if family == "matern32":
        a = np.sqrt(s.dtype.type(3)) * r
        e = np.exp(-a)
        return (one + a) * e, -(s.dtype.type(3) / 2) * e
    if family == "matern52":
        a = np.sqrt(s.dtype.type(5)) * r
        e = np.exp(-a)
        return (one + a + s.dtype.type(5) * s / 3) * e, -(s.dtype.type(5) / 6) * (one + a) * e
    raise ValueError(f"{family}: no derivative")


def sqdist(A, B, ell):
    d = (A[:, None, :] - B[None, :, :]) / ell
    return np.sum(d * d, axis=2)


def kmat(family, sigma2, ell, A, B):
    return sigma2 * g01(family, sqdist(A, B, ell))[0]


def panel(c, X, dtype=np.float64):
    """k (n, M), J (n, M, D) and s (n, M) of the points X, from direct differences"""
    X, Xu, ell = (np.asarray(a, dtype=dtype) for a in (X, c["Xu"], c["ell"]))
    diff = X[:, None, :] - Xu[None, :, :]
    s = np.sum((diff / ell) ** 2, axis=2)
    g0, g1 = g01(c["family"], s)
    s2 = dtype(c["sigma2"])
    return s2 * g0, 2 * s2 * g1[:, :, None] * (diff / ell ** 2), s


def lengthscales(D, iso):
    """Distinct per dimension and scaled with sqrt(D), so that the points keep a few inducing inputs within reach at every D"""
    if iso:
        return np.full(D, 0.6 * math.sqrt(D))
    return math.sqrt(D) * np.linspace(0.8, 0.45, D)


def make_case(family, iso, d_out, D, M, ns, seed, jitter=SHARP_JITTER, dense=False, coincident=False):
    """Xu ~ U(-1.7, 1.7), the points 0.3 randn about inducing inputs picked at random, mu_v ~ 0.3 randn, a non-diagonal W,
    Sigma_v = 0.01 I + 0.02 U U' / 8 (rank 8, every cross block dense and not symmetric) or, with dense, a random SPD matrix
    B B' / Q + 0.05 I.  coincident: point 0 is inducing input 0, point 1 lies 1e-9 from inducing input 1."""
    rng = np.random.default_rng(seed)
    Q = M * d_out
    Xu = rng.uniform(-1.7, 1.7, (M, D))
    ell = lengthscales(D, iso)
    X = Xu[rng.integers(0, M, ns)] + 0.3 * rng.normal(size=(ns, D))
    if coincident:
        X[0] = Xu[0]
        X[1] = Xu[1 % M] + 1e-9 * rng.normal(size=D)
    mu_v = 0.3 * rng.normal(size=Q)
    if dense:
        B = rng.normal(size=(Q, Q))
        Sigma_v = B @ B.T / Q + 0.05 * np.eye(Q)
    else:
        U = rng.normal(size=(Q, 8))
        Sigma_v = 0.02 * (U @ U.T) / 8 + 0.01 * np.eye(Q)
    Bw = rng.normal(size=(d_out, d_out))
    W = Bw @ Bw.T / d_out + np.eye(d_out)
    return dict(family=family, iso=iso, d_out=d_out, D=D, M=M, sigma2=SIGMA2, ell=ell, ell_dev=ell[:1] if iso else ell, jitter=jitter,
                Xu=Xu, X=X, mu_v=mu_v, Sigma_v=Sigma_v, W=W)


# ---- the named cases -----------------------------------------------------------------------------------------------------------------
# grid: every family with isotropic and ARD lengthscales and every output count; D, M and ns walk their lists at different strides,
# so that every value occurs with every family and the (M, ns) pairs spread over the grid
DIMS, SIZES, COUNTS = (1, 3, 8, 9, 32), (5, 64, 65, 130), (1, 4, 17, 65)
CASES = {}
_i = 0
for _fam in FAMILIES:
    for _iso in (False, True):
        for _do in (1, 2, 4):
            _D, _M, _ns = DIMS[_i % 5], SIZES[_i % 4], COUNTS[(_i + _i // 4) % 4]
            CASES[f"{_fam}_{'iso' if _iso else 'ard'}_o{_do}_D{_D}_M{_M}_n{_ns}"] = dict(family=_fam, iso=_iso, d_out=_do, D=_D, M=_M,
                                                                                         ns=_ns, seed=4000 + _i)
            _i += 1
GRID = list(CASES)
# the (D, M, ns) corners the walk leaves out
CASES["se_ard_o4_D32_M130_n65"] = dict(family="se", iso=False, d_out=4, D=32, M=130, ns=65, seed=4100)
CASES["matern52_ard_o2_D1_M130_n1"] = dict(family="matern52", iso=False, d_out=2, D=1, M=130, ns=1, seed=4101)
CASES["matern32_iso_o1_D9_M5_n65"] = dict(family="matern32", iso=True, d_out=1, D=9, M=5, ns=65, seed=4102)
CORNERS = [n for n in CASES if n not in GRID]
# a random dense SPD Sigma_v at d_out = 2: cross blocks that are far from symmetric
CASES["dense"] = dict(family="se", iso=False, d_out=2, D=3, M=20, ns=17, seed=4200, dense=True)
# a point exactly on an inducing input and another 1e-9 away
for _fam in FAMILIES:
    CASES[f"coincident_{_fam}"] = dict(family=_fam, iso=False, d_out=2, D=3, M=65, ns=6, seed=4300 + len(_fam), coincident=True)
COINCIDENT = [f"coincident_{f}" for f in FAMILIES]
# chunking: 150 points
CASES["chunk"] = dict(family="matern52", iso=False, d_out=2, D=4, M=70, ns=150, seed=4400)
# the linearised rollout (d_out = D)
for _fam in ("se", "matern52"):
    CASES[f"rollout_{_fam}"] = dict(family=_fam, iso=False, d_out=2, D=2, M=30, ns=2, seed=4500 + len(_fam))
# the cases of the host file's spread measurement (the longdouble route factors K_uu in Python: M <= 70)
SPREAD_CASES = [n for n in GRID if CASES[n]["M"] <= 65][:10] + ["dense", "matern32_iso_o1_D9_M5_n65"] + COINCIDENT


def get_case(name):
    c = make_case(**CASES[name])
    c["name"] = name
    return c


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _ld_cholesky(A):
    """lower Cholesky factor in A's dtype (np.linalg has no longdouble): column by column"""
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def _ld_solve_lower(L, B, trans=False):
    """L^-1 B or L^-T B for lower L, in L's dtype"""
    n = len(L)
    X = np.array(B, dtype=L.dtype, copy=True)
    if not trans:
        for j in range(n):
            X[j] = X[j] / L[j, j]
            X[j + 1:] -= np.outer(L[j + 1:, j], X[j])
    else:
        for j in range(n - 1, -1, -1):
            X[j] = X[j] / L[j, j]
            X[:j] -= np.outer(L[j, :j], X[j])
    return X


def kinv_apply(c, route):
    """f(B) = Kinv B (B: M x anything) by the route"""
    M = c["M"]
    if route == "longdouble":
        t = np.longdouble
        Xu, ell = np.asarray(c["Xu"], dtype=t), np.asarray(c["ell"], dtype=t)
        L = _ld_cholesky(kmat(c["family"], t(c["sigma2"]), ell, Xu, Xu) + t(c["jitter"]) * np.eye(M, dtype=t))
        return lambda B: _ld_solve_lower(L, _ld_solve_lower(L, B), trans=True)
    Kuu = kmat(c["family"], c["sigma2"], c["ell"], c["Xu"], c["Xu"]) + c["jitter"] * np.eye(M)
    if route == "inverse":
        Kinv = np.linalg.inv(Kuu)
        Kinv = 0.5 * (Kinv + Kinv.T)
        return lambda B: Kinv @ B
    from scipy.linalg import cho_factor, cho_solve
    F = cho_factor(Kuu, lower=True)
    return lambda B: cho_solve(F, B)


def evaluate(c, X=None, route="cholesky", transpose_cross=False, noise=False):
    """dict(mean (n, o), jac (n, o, D), var (n, o, o), var_grad (n, o, o, D), jac_cov (n, o D, o D)) of the case's points (or of X),
    float64.  transpose_cross: the wrong reference that reads every block Sigma^(ij) transposed (what a GEMM that took A for
    symmetric would compute)."""
    t = np.longdouble if route == "longdouble" else np.float64
    X = np.asarray(c["X"] if X is None else X, dtype=np.float64).reshape(-1, c["D"])
    M, D, o, n = c["M"], c["D"], c["d_out"], len(X)
    k, J, _ = panel(c, X, t)
    P = np.concatenate([k[:, :, None], J], axis=2)                         # n x M x (1 + D)
    flat = P.transpose(1, 0, 2).reshape(M, -1)
    KP = kinv_apply(c, route)(flat).reshape(M, n, 1 + D).transpose(1, 0, 2)
    mu = np.asarray(c["mu_v"], dtype=t).reshape(o, M)
    Sig = np.asarray(c["Sigma_v"], dtype=t)
    ell = np.asarray(c["ell"], dtype=t)
    mean = k @ mu.T
    jac = np.einsum("nmd,om->nod", J, mu)
    var = np.zeros((n, o, o), dtype=t)
    vg = np.zeros((n, o, o, D), dtype=t)
    jc = np.zeros((n, o, D, o, D), dtype=t)
    prior = t(C_FAM[c["family"]]) * t(c["sigma2"]) / ell ** 2
    for i in range(o):
        for j in range(o):
            S = Sig[i * M:(i + 1) * M, j * M:(j + 1) * M]
            if transpose_cross:
                S = S.T
            U = np.einsum("ml,nlc->nmc", S, P)
            if i == j:
                U = U - KP
            var[:, i, j] = np.einsum("nm,nm->n", k, U[:, :, 0]) + (t(c["sigma2"]) if i == j else 0)
            vg[:, i, j] = np.einsum("nmd,nm->nd", J, U[:, :, 0]) + np.einsum("nm,nmd->nd", k, U[:, :, 1:])
            jc[:, i, :, j, :] = np.einsum("nmd,nme->nde", J, U[:, :, 1:])
            if i == j:
                jc[:, i, :, i, :] += np.diag(prior)
    if noise:
        var = var + np.linalg.inv(np.asarray(c["W"], dtype=np.float64)).astype(t)
    out = dict(mean=mean, jac=jac, var=var, var_grad=vg, jac_cov=jc.reshape(n, o * D, o * D))
    return {k_: np.asarray(v, dtype=np.float64) for k_, v in out.items()}


def joint_cov(c, X1, X2):
    """cov[(i, x), (j, x')] of the latent f at the point pairs (X1[p], X2[p]): (n, o, o) -- sgp_predict_joint's entry, float64:
    delta_ij (k(x, x') - k(x)' Kinv k(x')) + k(x)' Sigma^(ij) k(x')"""
    X1, X2 = (np.asarray(a, dtype=np.float64).reshape(-1, c["D"]) for a in (X1, X2))
    M, o = c["M"], c["d_out"]
    k1, k2 = panel(c, X1)[0], panel(c, X2)[0]
    kxx = c["sigma2"] * g01(c["family"], np.sum(((X1 - X2) / c["ell"]) ** 2, axis=1))[0]
    q = kxx - np.einsum("nm,mn->n", k1, kinv_apply(c, "cholesky")(k2.T))
    out = np.empty((len(X1), o, o))
    for i in range(o):
        for j in range(o):
            out[:, i, j] = np.einsum("nm,ml,nl->n", k1, c["Sigma_v"][i * M:(i + 1) * M, j * M:(j + 1) * M], k2) + (q if i == j else 0.0)
    return out


def bounds(c, X=None, cst=C_BOUND):
    """The bounds of the module docstring, keyed and shaped as `evaluate`'s outputs"""
    X = np.asarray(c["X"] if X is None else X, dtype=np.float64).reshape(-1, c["D"])
    M, D, o, n = c["M"], c["D"], c["d_out"], len(X)
    k, J, s = panel(c, X)
    w = 1.0 + 0.5 * s
    pk, pJ = w * np.abs(k), w[:, :, None] * np.abs(J)
    Kuu = kmat(c["family"], c["sigma2"], c["ell"], c["Xu"], c["Xu"]) + c["jitter"] * np.eye(M)
    cond_k = float(np.linalg.cond(Kuu))
    cond_s = float(np.linalg.cond(c["Sigma_v"]))
    aK = np.abs(np.linalg.inv(Kuu))
    amu = np.abs(c["mu_v"]).reshape(o, M)
    prior = C_FAM[c["family"]] * c["sigma2"] / np.asarray(c["ell"]) ** 2
    Kk, KJ = pk @ aK, np.einsum("ml,nle->nme", aK, pJ)
    var = np.zeros((n, o, o))
    vg = np.zeros((n, o, o, D))
    jc = np.zeros((n, o, D, o, D))
    for i in range(o):
        for j in range(o):
            aS = np.abs(c["Sigma_v"][i * M:(i + 1) * M, j * M:(j + 1) * M])
            Sk, SJ = np.einsum("ml,nl->nm", aS, pk), np.einsum("ml,nle->nme", aS, pJ)
            var[:, i, j] = cond_s * np.einsum("nm,nm->n", pk, Sk)
            vg[:, i, j] = np.einsum("nmd,nm->nd", pJ, Sk) + np.einsum("nm,nmd->nd", pk, SJ)
            jc[:, i, :, j, :] = np.einsum("nmd,nme->nde", pJ, SJ)
            if i == j:
                var[:, i, i] += c["sigma2"] + cond_k * np.einsum("nm,nm->n", pk, Kk)
                vg[:, i, i] += 2.0 * cond_k * np.einsum("nmd,nm->nd", pJ, Kk)
                jc[:, i, :, i, :] += np.diag(prior) + cond_k * np.einsum("nmd,nme->nde", pJ, KJ)
    out = dict(mean=pk @ amu.T, jac=np.einsum("nmd,om->nod", pJ, amu), var=var, var_grad=vg, jac_cov=jc.reshape(n, o * D, o * D))
    return {k_: cst * EPS * v for k_, v in out.items()}


def worst(err, bound):
    """Worst error / bound (a zero bound admits a zero error only; a non-finite error is infinitely wrong)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


OUTPUTS = ("mean", "jac", "var", "var_grad", "jac_cov")


def ratios(ref, tol, out):
    """Worst error / bound per output of `out` (a dict keyed as evaluate's; None entries are skipped) against ref at tol"""
    return {k: worst(np.abs(np.asarray(out[k]).reshape(ref[k].shape) - ref[k]), tol[k]) for k in OUTPUTS if out.get(k) is not None}


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests compare against for one case, computed once per process, arrays read-only: the inputs, `ref` (the
    Cholesky route) and `tol`"""
    c = get_case(name)
    c["ref"] = evaluate(c)
    c["tol"] = bounds(c)
    for d in (c, c["ref"], c["tol"]):
        for x in d.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return c


# ---- the linearised rollout ----------------------------------------------------------------------------------------------------------
def linearize_rollout(c, m0, S0, steps, noise=True):
    """The EKF-style rollout of B Gaussians N(m0[b], S0[b]) through the case's GP (d_out = D), a plain loop over the restatement:
    m' = mean(m), S' = Jac S Jac' + C_f(m) (+ W^-1).  Returns (means (steps, B, D), covs (steps, B, D, D))."""
    m, S = np.array(m0, dtype=np.float64), np.array(S0, dtype=np.float64)
    B, D = m.shape
    Winv = np.linalg.inv(c["W"])
    means, covs = np.empty((steps, B, D)), np.empty((steps, B, D, D))
    for k in range(steps):
        for b in range(B):
            r = evaluate(c, m[b][None, :])
            Jb = r["jac"][0]
            Cb = Jb @ S[b] @ Jb.T
            S[b] = 0.5 * (Cb + Cb.T) + r["var"][0] + (Winv if noise else 0.0)
            m[b] = r["mean"][0]
        means[k], covs[k] = m, S
    return means, covs


# ---- the ledger of exported names (tests/call_sequence_ref.ENTRY_POINTS; tests/test_call_sequences_host.py holds it to the header).
# The call reads the handle's kernel and q(v) and writes nothing the sweep keeps, so it is a reader; what stands behind the class is
# tests/test_gpu_predict_grad.py::test_nothing_the_sweep_keeps_is_written.
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_predict_grad", CR.READER)


register_entry_point()
