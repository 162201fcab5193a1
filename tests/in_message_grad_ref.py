"""NumPy restatement of the :in log-message with its gradient and Hessian with respect to the input (sgp_in_message_grad), on top of
tests/in_message_ref.py (make_case / make_shape_case / kernel_of / contraction), with the cases and the error bounds the host and
the GPU tests share.

Per point p of node t, k = K(Xu, x_p), s_t = sum_d mu_v^(d) (y_t' W)_d, S as in in_message_ref and A = tr(W) K_uu^-1 - S:
    logpdf = -1/2 tr(W) sigma2 + s_t'k + 1/2 k'A k,   q = s_t + A k,   grad = J'q,   hess = J'A J + sum_m q_m grad^2 k_m,
    k_m = sigma2 g(s_m), s_m = sum_d ((x_d - u_md) / ell_d)^2, z_md = (x_d - u_md) / ell_d^2,
    J_md = 2 sigma2 g'(s_m) z_md,   grad^2 k_m = sigma2 [4 g''(s_m) z_m z_m' + 2 g'(s_m) diag(1 / ell^2)].
The bounds follow the sibling's error model, one term per summand (B_m is the bracket, the size of what q_m is summed from):
    B_m             = |s_t|_m + tr(W) cond(K_uu) (|Kinv| |k|)_m + (|S| |k|)_m
    tol_grad[p,d]   = C eps sum_m |J_md| B_m
    tol_hess[p,d,e] = C eps [ tr(W) cond(K_uu) |J_d|'|Kinv||J_e| + |J_d|'|S||J_e| + sum_m B_m |grad^2 k_m[d,e]| ]
C = C_BOUND was settled on the CPU alone (tools/in_message_grad_rate.py --settle, recorded in profiles/in_message_grad.txt): the
restatement by two float64 routes -- the explicit inverse, and Cholesky solves -- against mpmath at 60 digits on the small cases
(MP_CASES).  The worst ratio at C = 1 is 5.4, at M = 1, where cond(K_uu) = 1 and the bound is a few roundings of one product;
with a factor 2 to spare the smallest round C is 20 (the sibling's 50 was the starting point).  The device's output never took
part in choosing it.

What the model does not carry is exp's own conditioning: k_m = sigma2 g(s_m) inherits the rounding of s_m times s_m / 2.  Where
some k_m is of the order of the others' sum this is far inside the cond(K_uu) term; it is all that is left at points so far from
every inducing input that the closure is flat (max_m k_m < 1e-12 sigma2, s_m / 2 > 27): the bounds are for points where the
message says something, and pendulum_batch's seed keeps the Newton iteration's end points there.

logpdf is compared at the sibling's bound (in_message_ref.vector_logpdf(want_bound=True))."""
import functools
import math

import numpy as np

from tests import in_message_ref as R

EPS = R.EPS
C_BOUND = 20.0
DIFFERENTIABLE = ("se", "matern32", "matern52")

# the shape cases of the GPU file (kwargs of in_message_ref.make_shape_case): the smallest that exercise each boundary.  Where many
# inducing inputs crowd a low-dimensional box (M = 129 in D = 3, M = 70 in D <= 2, M = 48 in D = 2) the jitter is 1e-3: at 1e-8
# cond(K_uu) is 1e10 .. 1e13 there and the bound, which carries it, would reject none of the host file's wrong references.
CROWDED_JITTER = 1e-3
GRAD_SHAPES = {}
for _M in (1, 63, 64, 65, 129):
    for _do in (1, 4):
        GRAD_SHAPES[f"M{_M}x{_do}"] = dict(M=_M, D=3, d_out=_do, family="se", sizes=[3, 1, 2], seed=700 + 10 * _do + _M,
                                           jitter=CROWDED_JITTER if _M > 100 else 1e-8)
for _D in (1, 2, 9, 32):
    for _iso in (False, True):
        GRAD_SHAPES[f"D{_D}{'iso' if _iso else ''}"] = dict(M=70, D=_D, d_out=2, family="se", sizes=[2, 3, 1], seed=800 + _D, iso=_iso,
                                                        jitter=CROWDED_JITTER if _D <= 2 else 1e-8)
for _f, _fam in enumerate(DIFFERENTIABLE):
    GRAD_SHAPES[f"{_fam}_coincident"] = dict(M=65, D=3, d_out=2, family=_fam, sizes=[7, 12, 5], seed=900 + _f, coincident=1)
GRAD_SHAPES["n1"] = dict(M=48, D=2, d_out=2, family="se", sizes=[1], seed=1001, jitter=CROWDED_JITTER)
GRAD_SHAPES["n64"] = dict(M=48, D=2, d_out=2, family="se", sizes=[40, 24], seed=1064, jitter=CROWDED_JITTER)
GRAD_SHAPES["n65"] = dict(M=48, D=2, d_out=2, family="se", sizes=[1, 64], seed=1065, jitter=CROWDED_JITTER)
GRAD_SHAPES["many"] = dict(M=48, D=6, d_out=4, family="se", sizes=[1 + t % 3 for t in range(1001)], seed=1100)
GRAD_SHAPES["limit4"] = dict(R.SHAPE_CASES["limit4"])
REFERENCE_CASES = ["a", "b", "c", "d", "f"]
# the cases small enough for mpmath (M <= 70; the points are thinned to MP_POINTS per case)
MP_CASES = ["a", "c", "f", "M1x1", "M1x4", "M63x4", "M65x1", "D1", "D2iso", "D9", "D32iso", "se_coincident", "matern32_coincident",
            "matern52_coincident", "n65"]
MP_POINTS = 6


def g_derivs(family, s):
    """(g, g', g'') of k = sigma2 g(s) at s = r^2.  Matern-3/2: g'' is infinite at r = 0 and multiplies z z' = 0 there; 0 is
    returned, the limit of the product."""
    s = np.asarray(s, dtype=np.float64)
    r = np.sqrt(s)
    if family == "se":
        e = np.exp(-0.5 * s)
        return e, -0.5 * e, 0.25 * e
    if family == "matern32":
        a = math.sqrt(3.0) * r
        e = np.exp(-a)
        with np.errstate(divide="ignore", invalid="ignore"):
            g2 = np.where(r > 0, 0.75 * math.sqrt(3.0) * e / np.where(r > 0, r, 1.0), 0.0)
        return (1.0 + a) * e, -1.5 * e, g2
    if family == "matern52":
        a = math.sqrt(5.0) * r
        e = np.exp(-a)
        return (1.0 + a + 5.0 * s / 3.0) * e, -(5.0 / 6.0) * (1.0 + a) * e, (25.0 / 12.0) * e
    raise ValueError(f"{family}: no gradient")


def get_case(name):
    """The inputs of a reference case (make_case) or of a shape case (make_shape_case)."""
    return R.make_case(name) if name in R.CASES else R.make_shape_case(**GRAD_SHAPES[name])


def panel(c, X=None):
    """k (n, M), J (n, M, D), Z (n, M, D), g' and g'' (n, M) of the case's points (or of X), from direct differences."""
    X = np.asarray(c["X"] if X is None else X, dtype=np.float64).reshape(-1, c["D"])
    ell = np.asarray(c["ell"], dtype=np.float64)
    diff = X[:, None, :] - c["Xu"][None, :, :]
    s = np.sum((diff / ell) ** 2, axis=2)
    Z = diff / ell ** 2
    g0, g1, g2 = g_derivs(c["family"], s)
    return c["sigma2"] * g0, 2.0 * c["sigma2"] * g1[:, :, None] * Z, Z, g1, g2


def node_of(c):
    return np.repeat(np.arange(len(c["start"]) - 1), np.diff(c["start"]))


def evaluate(c, route="inverse", fault=None, X=None, node=None):
    """(logpdf (n,), grad (n, D), hess (n, D, D)) of the case's points (or of X with their nodes) in float64.  route "inverse": A
    formed from the explicit inverse; "cholesky": every product with K_uu^-1 a pair of triangular solves.  fault: None, or one of
    the wrong references the bounds must reject -- "no_kernel_hessian" (drops sum q_m grad^2 k_m), "no_kinv" (drops the K_uu^-1
    half of A), "node0_y" (every node uses node 0's y)."""
    from scipy.linalg import cho_factor, cho_solve
    M, W, ell = c["M"], c["W"], np.asarray(c["ell"], dtype=np.float64)
    trW = float(np.trace(W)) if fault != "no_kinv" else 0.0
    node = node_of(c) if node is None else np.asarray(node)
    Kuu = R.kernel_of(c)(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(M)
    S, mus = R.contraction(c["mu_v"], c["Sigma_v"], W, M)
    yw = c["Y"] @ W
    if fault == "node0_y":
        yw = np.tile(yw[:1], (len(yw), 1))
    st = (mus @ yw.T).T[node]                                             # n x M
    k, J, Z, g1, g2 = panel(c, X)
    n, D = k.shape[0], c["D"]
    cols = np.concatenate([k[:, :, None], J], axis=2)                      # n x M x (1 + D)
    flat = cols.transpose(1, 0, 2).reshape(M, -1)                          # M x n (1 + D)
    if route == "inverse":
        A = trW * np.linalg.inv(Kuu) - S
        A = 0.5 * (A + A.T)
        U = A @ flat
    else:
        U = trW * cho_solve(cho_factor(Kuu, lower=True), flat) - S @ flat
    U = U.reshape(M, n, 1 + D).transpose(1, 0, 2)                          # n x M x (1 + D)
    q = st + U[:, :, 0]
    lp = -0.5 * trW * c["sigma2"] + np.sum(st * k, axis=1) + 0.5 * np.sum(k * U[:, :, 0], axis=1)
    grad = np.einsum("nmd,nm->nd", J, q)
    hess = np.einsum("nmd,nme->nde", J, U[:, :, 1:])
    if fault != "no_kernel_hessian":
        hess = hess + 4.0 * c["sigma2"] * np.einsum("nm,nmd,nme->nde", q * g2, Z, Z)
        hess = hess + 2.0 * c["sigma2"] * np.sum(q * g1, axis=1)[:, None, None] * np.diag(1.0 / ell ** 2)
    return lp, grad, 0.5 * (hess + hess.transpose(0, 2, 1))


def bounds(c, X=None, node=None, cst=C_BOUND):
    """(tol_grad (n, D), tol_hess (n, D, D)) of the module docstring."""
    M, W, ell = c["M"], c["W"], np.asarray(c["ell"], dtype=np.float64)
    trW = float(np.trace(W))
    node = node_of(c) if node is None else np.asarray(node)
    Kuu = R.kernel_of(c)(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(M)
    if M > R.VECTOR_ABOVE:
        from tests.test_envelope_host import spd_cond
        cond = spd_cond(Kuu)
    else:
        cond = float(np.linalg.cond(Kuu))
    aKinv = np.abs(np.linalg.inv(Kuu))
    S, mus = R.contraction(c["mu_v"], c["Sigma_v"], W, M)
    aS = np.abs(S)
    st = np.abs((mus @ (c["Y"] @ W).T).T[node])
    k, J, Z, g1, g2 = panel(c, X)
    ak, aJ = np.abs(k), np.abs(J)
    B = st + trW * cond * (ak @ aKinv) + ak @ aS                          # n x M
    tol_grad = cst * EPS * np.einsum("nmd,nm->nd", aJ, B)
    KJ = np.einsum("ml,nle->nme", aKinv, aJ)
    SJ = np.einsum("ml,nle->nme", aS, aJ)
    t = trW * cond * np.einsum("nmd,nme->nde", aJ, KJ) + np.einsum("nmd,nme->nde", aJ, SJ)
    t = t + 4.0 * c["sigma2"] * np.einsum("nm,nmd,nme->nde", B * np.abs(g2), np.abs(Z), np.abs(Z))
    t = t + 2.0 * c["sigma2"] * np.sum(B * np.abs(g1), axis=1)[:, None, None] * np.diag(1.0 / ell ** 2)
    return tol_grad, cst * EPS * t


def mp_evaluate(c, points):
    """(logpdf, grad, hess) of the listed points at 60 digits (mpmath), rounded once at the end: the exact values of the float64
    inputs.  g, g', g'' are restated here in mpmath."""
    import mpmath as mp
    M, D, d_out, fam = c["M"], c["D"], c["d_out"], c["family"]
    node = node_of(c)
    with mp.workdps(60):
        f = lambda v: mp.mpf(float(v))
        ell = [f(v) for v in c["ell"]]
        s2, jit = f(c["sigma2"]), f(c["jitter"])

        def g012(s):
            r = mp.sqrt(s)
            if fam == "se":
                e = mp.exp(-s / 2)
                return e, -e / 2, e / 4
            if fam == "matern32":
                a = mp.sqrt(3) * r
                e = mp.exp(-a)
                return (1 + a) * e, -3 * e / 2, (3 * mp.sqrt(3) / 4) * e / r if r > 0 else mp.mpf(0)
            a = mp.sqrt(5) * r
            e = mp.exp(-a)
            return (1 + a + 5 * s / 3) * e, -(mp.mpf(5) / 6) * (1 + a) * e, (mp.mpf(25) / 12) * e
        Xu = [[f(v) for v in row] for row in c["Xu"]]
        Kuu = mp.matrix(M, M)
        for i in range(M):
            for j in range(M):
                s = mp.fsum(((Xu[i][d] - Xu[j][d]) / ell[d]) ** 2 for d in range(D))
                Kuu[i, j] = s2 * g012(s)[0] + (jit if i == j else 0)
        Wm = [[f(c["W"][i, j]) for j in range(d_out)] for i in range(d_out)]
        trW = mp.fsum(Wm[i][i] for i in range(d_out))
        mu = [f(v) for v in c["mu_v"]]
        Sig = c["Sigma_v"]
        A = trW * mp.inverse(Kuu)
        for i in range(M):
            for j in range(M):
                acc = mp.mpf(0)
                for a in range(d_out):
                    for b in range(d_out):
                        sym = (f(Sig[a * M + i, b * M + j]) + f(Sig[a * M + j, b * M + i])) / 2     # contraction symmetrises S
                        mm = (mu[a * M + i] * mu[b * M + j] + mu[a * M + j] * mu[b * M + i]) / 2
                        acc += Wm[a][b] * (sym + mm)
                A[i, j] -= acc
        lp, grad, hess = [], [], []
        for p in points:
            t = node[p]
            yw = [mp.fsum(f(c["Y"][t, e]) * Wm[e][d] for e in range(d_out)) for d in range(d_out)]
            st = [mp.fsum(mu[d * M + m] * yw[d] for d in range(d_out)) for m in range(M)]
            x = [f(v) for v in c["X"][p]]
            k, g1, g2, Z = [], [], [], []
            for m in range(M):
                s = mp.fsum(((x[d] - Xu[m][d]) / ell[d]) ** 2 for d in range(D))
                a0, a1, a2 = g012(s)
                k.append(s2 * a0); g1.append(a1); g2.append(a2)
                Z.append([(x[d] - Xu[m][d]) / ell[d] ** 2 for d in range(D)])
            J = [[2 * s2 * g1[m] * Z[m][d] for m in range(M)] for d in range(D)]          # D x M
            Ak = [mp.fsum(A[m, l] * k[l] for l in range(M)) for m in range(M)]
            q = [st[m] + Ak[m] for m in range(M)]
            lp.append(float(-trW * s2 / 2 + mp.fsum(st[m] * k[m] for m in range(M)) + mp.fsum(k[m] * Ak[m] for m in range(M)) / 2))
            grad.append([float(mp.fsum(J[d][m] * q[m] for m in range(M))) for d in range(D)])
            AJ = [[mp.fsum(A[m, l] * J[e][l] for l in range(M)) for m in range(M)] for e in range(D)]
            c2 = 2 * s2 * mp.fsum(q[m] * g1[m] for m in range(M))
            H = np.empty((D, D))
            for d in range(D):
                for e in range(d, D):
                    v = mp.fsum(J[d][m] * AJ[e][m] for m in range(M)) + 4 * s2 * mp.fsum(q[m] * g2[m] * Z[m][d] * Z[m][e] for m in range(M))
                    if d == e:
                        v += c2 / ell[d] ** 2
                    H[d, e] = H[e, d] = float(v)
            hess.append(H)
    return np.array(lp), np.array(grad), np.array(hess)


def mp_points(c):
    """The points of a case that the mpmath comparison takes: MP_POINTS spread over the case, its first ten included where the
    case has coincident points (they are the first ten of node 1)."""
    n = len(c["X"])
    pts = set(np.linspace(0, n - 1, min(n, MP_POINTS)).astype(int).tolist())
    if c.get("sizes") == [7, 12, 5]:
        pts |= {7, 8, 12, 13}                                             # two on inducing inputs, two 1e-9 away
    return sorted(pts)


def worst(err, bound):
    """Worst error / bound (a zero bound admits a zero error only; a non-finite error is infinitely wrong)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the GPU tests compare against for one case, computed once per process, arrays read-only: the inputs, lp and its
    bound tol (the sibling's), grad, hess (the Cholesky route) and tol_grad, tol_hess."""
    c = dict(get_case(name))
    lp, grad, hess = evaluate(c, "cholesky")
    tg, th = bounds(c)
    v = R.vector_logpdf(c, want_bound=True)
    c.update(lp=lp, tol=v["tol"], grad=grad, hess=hess, tol_grad=tg, tol_hess=th)
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


def ratios(c, lp, grad, hess):
    """Worst error / bound of the three outputs against reference(name)."""
    out = dict(logpdf=worst(np.abs(lp - c["lp"]), c["tol"]), grad=worst(np.abs(grad - c["grad"]), c["tol_grad"]))
    if hess is not None:
        out["hess"] = worst(np.abs(hess - c["hess"]), c["tol_hess"])
    return out


# ------------------------------------------------------------------------------------------------
# the damped Newton iteration of multisgp.rule_in_laplace_batch, restated over the float64 restatement above
FLAT = 1e-12                                                             # max_m k_m / sigma2 below which the closure counts as flat


def pendulum_batch(T=300, seed=30):
    """A T-node batch on case a's model (M = 48, D = 2, d_out = 2) by case a's recipe: left means ~ U(-1.5, 1.5), left covariances
    0.05 (L L' / D + I), y ~ randn.  The seed is the first for which the damped Newton iteration on the float64 restatement
    (tests/test_in_message_grad_host.py) leaves at most 5 % of the nodes unconverged after 20 rounds AND ends no node where the
    closure is flat (max_m k_m < FLAT sigma2: about one start in a hundred runs off to such a plateau, where the gradient
    vanishes and the bounds' model has nothing to hold on to, see the module docstring)."""
    c = dict(R.make_case("a"))
    rng = np.random.default_rng(seed)
    D = c["D"]
    means = rng.uniform(-1.5, 1.5, (T, D))
    covs = np.empty((T, D, D))
    for t in range(T):
        L = rng.normal(size=(D, D))
        covs[t] = 0.05 * (L @ L.T / D + np.eye(D))
    c.update(means=means, covs=covs, Y=rng.normal(size=(T, c["d_out"])), nodes=T, X=means.copy(),
             start=np.arange(T + 1, dtype=np.int64))
    return c
