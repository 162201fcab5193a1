"""NumPy / SciPy restatement of the three forward point calls -- sgp_predict, sgp_predict_var and sgp_out_message -- with the
shape cases and the error bounds the host file (tests/test_predict_shapes_host.py) and the GPU file
(tests/test_gpu_predict_shapes.py) share.  Inputs are in_message_ref.make_shape_case's (ragged M and Q, iso / ARD lengthscales, a
non-diagonal W, Sigma_v = 0.01 I + 0.02 U U' / rank), the kernel is test_kernel_family_host.matern's.

Per test point, k = K(Xu, x), in float64 through Cholesky solves (no explicit inverse):
    mean[o]    = k' mu^(o)                      bound 50 eps |k|' |mu^(o)|                        (gpssm_ref.out_message_ref's, per point)
    qff        = sigma2 - |L_K^-1 k|^2          bound 50 eps cond(K_uu) sigma2
    form[i, j] = k' Sigma_v^(ij) k              bound 50 eps cond(Sigma_v) sqrt(form_ii form_jj)
    C          = form + qff I  (+ W^-1)
-- the error model and constants of tests/test_gpu_predict_var.py / tests/in_message_ref.py.  A diagonal entry of C carries both
terms; with the usual jitter of 1e-8 the first is 1e-6 .. 1e-4 absolute, the size of a dropped row of the form.  Two derived
comparisons do not carry it and are sharp whatever the jitter, one compares the noise flag:
    off-diagonal  C_ij, i != j                   bound  form term + 2 eps |C_ij|
    differences   C_ii - C_00 against form_ii - form_00 (the device adds one qff to every diagonal entry)
                                                 bound  50 eps cond(Sigma_v) (form_ii + form_00) + 4 eps (|C_ii| + |C_00|)
    noise         C_noise - C against W^-1       bound  2 spacing(|C_noise| + |W^-1|) + 4 eps max |W^-1|   (test_gpu_envelope's)
and, where the jitter is SHARP_JITTER, cond(K_uu + jitter I) <= 1e6 (sigma2 M / jitter bounds it: 1.04e5 at M = 129), so that the
diagonal itself is compared at 1e-8 or less.  The cases named ill_* keep the jitter 1e-8 and `limit` 1e-6: the ill-conditioned
route at the old bound.  W^-1 of the reference is the exact inverse of the float64 W (rational arithmetic), rounded once.

:out of node t: mean[t, o] = sum_s w_s k_s' mu^(o), bound 50 eps sum_s |w_s| |k_s|' |mu^(o)| (gpssm_ref's).

`evaluate(c, fault)` restates the faults a kernel on these paths could have (FAULTS); the host file shows that each moves a
compared output by more than 10 x its bound on every case it can occur in."""
import functools
from fractions import Fraction

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from tests import in_message_ref as R

EPS = R.EPS
TB = 64
SHARP_JITTER = 1e-3                       # in_message_grad_ref.CROWDED_JITTER
COND_KUU_MAX, COND_SIGMA_MAX, FORM_MIN = 1e6, 1e3, 1e-6
NODE_SIZES = [1, 64, 65, 129, 200, 3]
FAMILIES = R.FAMILIES
FAULTS = ["drop_ls_row", "drop_k_row", "unmasked_upper", "block_stride_mp", "mu_stride_mp", "drop_65th_point", "winv_diagonal"]

# name -> kwargs of in_message_ref.make_shape_case, plus group (the test that runs it); one node of ns points unless sizes are given
CASES = {}
for _M in (43, 65):
    for _do in (2, 3, 4):
        CASES[f"dout{_M}x{_do}"] = dict(group="dout", M=_M, D=3, d_out=_do, family="se", sizes=[70], seed=1100 + 10 * _do + _M)
for _M in (1, 63, 64, 129):
    for _do in (1, 3, 4):
        CASES[f"ragged{_M}x{_do}"] = dict(group="ragged", M=_M, D=3, d_out=_do, family="se", sizes=[65], seed=1200 + 10 * _do + _M)
for _f, _fam in enumerate(FAMILIES):
    for _do in (1, 2, 3, 4):
        CASES[f"{_fam}x{_do}"] = dict(group="family", M=65, D=9, d_out=_do, family=_fam, sizes=[70], seed=1300 + 10 * _f + _do,
                                      coincident=0)
for _D in (1, 2, 4, 8, 5, 32):
    for _iso in (False, True):
        CASES[f"dim{_D}{'iso' if _iso else ''}"] = dict(group="dims", M=70, D=_D, d_out=2, family="se", sizes=[257], seed=1400 + _D,
                                                        iso=_iso)
for _fam in ("se", "matern12"):
    for _do in (1, 4):
        CASES[f"blocks_{_fam}x{_do}"] = dict(group="blocks", M=48, D=2, d_out=_do, family=_fam, sizes=[513], seed=1500 + _do)
for _fam in ("se", "matern12"):
    CASES[f"nodes_{_fam}"] = dict(group="nodes", M=70, D=7, d_out=2, family=_fam, sizes=NODE_SIZES, seed=1600)
CASES["many"] = dict(group="many", M=48, D=6, d_out=4, family="se", sizes=[1 + t % 3 for t in range(1001)], seed=1700)
CASES["limit"] = dict(group="limit", M=1008, D=2, d_out=4, family="se", sizes=[70], seed=1800, jitter=1e-6)
CASES["ill_dout65x3"] = dict(CASES["dout65x3"], group="ill", jitter=1e-8)
CASES["ill_ragged129x4"] = dict(CASES["ragged129x4"], group="ill", jitter=1e-8)
CASES["ill_dim1"] = dict(CASES["dim1"], group="ill", jitter=1e-8)
for _k in CASES.values():
    _k.setdefault("jitter", SHARP_JITTER)
SHARP = [n for n, k in CASES.items() if k["jitter"] == SHARP_JITTER]
RAGGED_NS = (1, 64, 65)                   # one point, one full tile of k_predvar_multi, one point into the second workgroup
BLOCK_NS = (255, 256, 257, 513)           # k_predict's 256-thread blocks: one short of one, one, one into the second, into the third
MP_POINTS = 6


def group(name):
    return sorted(n for n, k in CASES.items() if k["group"] == name)


def make_case(name):
    """make_shape_case's inputs of a case.  M = 1: the points lie 0.6 lengthscales (per dimension, randn) about the one inducing
    input -- further out the one kernel value is all there is of the mean, its exponent's rounding (eps s / 2) outgrows the dot
    product's bound and the forms fall below FORM_MIN.  The `nodes` cases take weights ~ U(-0.5, 1.5) with every fifth of a
    longer node exactly 0 (a node's 65th point, index 64, keeps its weight)."""
    kw = {k: v for k, v in CASES[name].items() if k != "group"}
    c = R.make_shape_case(**kw)
    rng = np.random.default_rng(kw["seed"] + 5000)
    if c["M"] == 1:
        c["X"] = c["Xu"][0] + 0.6 * c["ell"] * rng.normal(size=c["X"].shape)
    if CASES[name]["group"] == "nodes":
        w = rng.uniform(-0.5, 1.5, len(c["X"]))
        for t in range(c["nodes"]):
            if c["sizes"][t] > 1:
                w[c["start"][t]:c["start"][t + 1]:5] = 0.0
        c["wts"] = w
    c["name"] = name
    return c


def exact_inverse(W):
    """The inverse of the float64 matrix W in rational arithmetic (Gauss-Jordan), each entry rounded once."""
    d = W.shape[0]
    a = [[Fraction(float(W[i, j])) for j in range(d)] + [Fraction(int(i == j)) for j in range(d)] for i in range(d)]
    for col in range(d):
        piv = max(range(col, d), key=lambda r: abs(a[r][col]))
        a[col], a[piv] = a[piv], a[col]
        inv = 1 / a[col][col]
        a[col] = [v * inv for v in a[col]]
        for r in range(d):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [v - f * u for v, u in zip(a[r], a[col])]
    return np.array([[float(a[i][d + j]) for j in range(d)] for i in range(d)])


def conditions(c):
    """(cond(K_uu + jitter I), cond(Sigma_v)): the SVD's up to in_message_ref.VECTOR_ABOVE, extreme eigenvalues above."""
    Kuu = R.kernel_of(c)(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(c["M"])
    if c["M"] > R.VECTOR_ABOVE:
        from tests.test_envelope_host import spd_cond
        return spd_cond(Kuu), spd_cond(np.asarray(c["Sigma_v"]))
    return float(np.linalg.cond(Kuu)), float(np.linalg.cond(c["Sigma_v"]))


def padded_mu(mu_v, M, d_out, stride):
    """(d_out, M): output o read at o * stride of mu_v padded with zeros -- stride = M is mu_v itself."""
    pad = np.zeros(max((M * d_out + TB - 1) // TB * TB, (d_out - 1) * stride + M))
    pad[:M * d_out] = mu_v
    return np.stack([pad[o * stride:o * stride + M] for o in range(d_out)])


def evaluate(c, fault=None):
    """dict(mean (n, d_out), qff (n,), form, C, C_noise (n, d_out, d_out), Winv, node_mean (T, d_out)) of a case in float64.
    fault: None, or one of FAULTS --
      drop_ls_row      the last row of L_S (Sigma_v = L_S L_S') takes no part in z_i = L_S[iM:(i+1)M, :]' k
      drop_k_row       the last row of k takes no part in the forms
      unmasked_upper   L_S with what the in-place factorisation leaves above its diagonal: Sigma_v's strict upper triangle
      block_stride_mp  the blocks of Sigma_v read at multiples of M_p (in_message_ref.padded_blocks)
      mu_stride_mp     mu^(o) read at o M_p of the zero-padded mu_v
      drop_65th_point  the 65th point of every node that has one left out of its sum
      winv_diagonal    1 / diag(W) for W^-1."""
    M, d_out, start = c["M"], c["d_out"], c["start"]
    Mp = (M + TB - 1) // TB * TB
    kern = R.kernel_of(c)
    Kuu = kern(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(M)
    K = kern(c["sigma2"], c["ell"], c["Xu"], c["X"])                            # M x n
    A = solve_triangular(cholesky(Kuu, lower=True), K, lower=True)
    qff = c["sigma2"] - np.sum(A * A, axis=0)
    mus = padded_mu(c["mu_v"], M, d_out, Mp if fault == "mu_stride_mp" else M)
    mean = K.T @ mus.T
    n = K.shape[1]
    Sig = np.asarray(c["Sigma_v"])
    form = np.empty((n, d_out, d_out))
    if fault in ("drop_ls_row", "unmasked_upper"):
        L = cholesky(Sig, lower=True)
        if fault == "drop_ls_row":
            L[-1, :] = 0.0
        else:
            L = L + np.triu(Sig, 1)
        Z = [L[i * M:(i + 1) * M, :].T @ K for i in range(d_out)]
        for i in range(d_out):
            for j in range(i, d_out):
                form[:, i, j] = form[:, j, i] = np.sum(Z[i] * Z[j], axis=0)
    else:
        if fault == "block_stride_mp":
            Sig = R.padded_blocks(Sig, M, d_out, Mp)
        Kf = K
        if fault == "drop_k_row":
            Kf = K.copy()
            Kf[-1, :] = 0.0
        for i in range(d_out):
            for j in range(i, d_out):
                form[:, i, j] = form[:, j, i] = np.sum(Kf * (Sig[i * M:(i + 1) * M, j * M:(j + 1) * M] @ Kf), axis=0)
    C = form + qff[:, None, None] * np.eye(d_out)[None]
    Winv = np.diag(1.0 / np.diag(c["W"])) if fault == "winv_diagonal" else exact_inverse(np.asarray(c["W"]))
    w = np.array(c["wts"])
    if fault == "drop_65th_point":
        for t in range(len(start) - 1):
            if start[t + 1] - start[t] > 64:
                w[start[t] + 64] = 0.0
    node_mean = np.stack([w[start[t]:start[t + 1]] @ mean[start[t]:start[t + 1]] for t in range(len(start) - 1)])
    return dict(mean=mean, qff=qff, form=form, C=C, C_noise=C + Winv[None], Winv=Winv, node_mean=node_mean, K=K, mus=mus)


def bounds(c, ref, cond_kuu, cond_sigma):
    """The bounds of the module docstring from the reference's own values: b_mean (n, d_out), b_qff, b_form (n, d_out, d_out),
    b_node (T, d_out)."""
    start, d_out = c["start"], c["d_out"]
    aK, amu = np.abs(ref["K"]), np.abs(ref["mus"])
    b_mean = 50 * EPS * aK.T @ amu.T
    diag = np.sqrt(np.einsum("sii->si", ref["form"]))
    b_form = 50 * EPS * cond_sigma * diag[:, :, None] * diag[:, None, :]
    aw = np.abs(c["wts"])
    b_node = np.stack([aw[start[t]:start[t + 1]] @ b_mean[start[t]:start[t + 1]] for t in range(len(start) - 1)])
    return dict(b_mean=b_mean, b_qff=50 * EPS * cond_kuu * c["sigma2"], b_form=b_form, b_node=b_node.reshape(-1, d_out))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests compare against for one case, computed once per process, arrays read-only: the inputs, evaluate()'s
    values, bounds()'s, cond_kuu and cond_sigma."""
    c = make_case(name)
    cond_kuu, cond_sigma = conditions(c)
    ref = evaluate(c)
    c.update(ref, cond_kuu=cond_kuu, cond_sigma=cond_sigma, **bounds(c, ref, cond_kuu, cond_sigma))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def worst(err, bound):
    """Worst error / bound (a zero bound admits a zero error only; a non-finite error is infinitely wrong)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.where(np.isfinite(err), err, np.inf)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


def mean_ratio(c, mean, rows=slice(None)):
    """Worst error / bound of per-point means (as sgp_predict, sgp_predict_var or sgp_out_message return them) over `rows`."""
    return worst(np.abs(np.reshape(mean, (-1, c["d_out"])) - c["mean"][rows]), c["b_mean"][rows])


def var_ratios(c, C, C_noise=None, rows=slice(None), truth=None):
    """Worst error / bound of each comparison of the module docstring over the points `rows`: diag, floor (-C_ii over its
    bound), and for d_out > 1 offdiag and diagdiff; noise with C_noise.  truth: (form, C, Winv) to compare against in place of
    the reference's (the host file's mpmath values); the bounds are always the reference's."""
    d = c["d_out"]
    form, Cr, Winv = (c["form"][rows], c["C"][rows], c["Winv"]) if truth is None else truth
    C = np.reshape(C, (-1, d, d))
    b_form = c["b_form"][rows]
    eye = np.eye(d, dtype=bool)
    b_C = b_form + c["b_qff"] * eye[None]
    out = dict(diag=worst(np.abs(C - Cr)[:, eye], b_C[:, eye]), floor=worst(np.maximum(-C[:, eye], 0.0), b_C[:, eye]))
    if d > 1:
        off = ~eye
        out["offdiag"] = worst(np.abs(C - Cr)[:, off], (b_form + 2 * EPS * np.abs(Cr))[:, off])
        dg, fg, bg = np.einsum("sii->si", C), np.einsum("sii->si", form), np.einsum("sii->si", b_form)
        cr = np.abs(np.einsum("sii->si", Cr))
        err = np.abs((dg[:, 1:] - dg[:, :1]) - (fg[:, 1:] - fg[:, :1]))
        out["diagdiff"] = worst(err, bg[:, 1:] + bg[:, :1] + 4 * EPS * (cr[:, 1:] + cr[:, :1]))
    if C_noise is not None:
        Cn = np.reshape(C_noise, (-1, d, d))
        bound = 2 * np.spacing(np.abs(Cn) + np.abs(c["Winv"])[None]) + 4 * EPS * np.abs(c["Winv"]).max()
        out["noise"] = worst(np.abs((Cn - C) - Winv[None]), bound)
    return out


def node_ratio(c, node_mean):
    return worst(np.abs(node_mean - c["node_mean"]), c["b_node"])


def sharp_conditions(c):
    """(cond(K_uu + jitter I), cond(Sigma_v), the smallest form_ii) of a reference."""
    return c["cond_kuu"], c["cond_sigma"], float(np.einsum("sii->si", c["form"]).min())


# ------------------------------------------------------------------------------------------------
# the same values at 60 digits
def mp_points(c):
    """The points the mpmath comparison takes: MP_POINTS spread over the case, and of a case with coincident points one on an
    inducing input and one 1e-9 away."""
    n = len(c["X"])
    pts = set(np.linspace(0, n - 1, min(n, MP_POINTS)).astype(int).tolist())
    if CASES[c["name"]].get("coincident") is not None:
        pts |= {1, 6}
    return sorted(pts)


def mp_evaluate(c, points):
    """(mean (p, d_out), qff (p,), form, C (p, d_out, d_out), Winv) of the listed points at 60 digits (mpmath), each rounded once
    at the end: the exact values of the float64 inputs.  The kernel families are restated here in mpmath."""
    import mpmath as mp
    M, D, d_out, fam = c["M"], c["D"], c["d_out"], c["family"]
    with mp.workdps(60):
        f = lambda v: mp.mpf(float(v))
        ell = [f(v) for v in c["ell"]]
        s2, jit = f(c["sigma2"]), f(c["jitter"])

        def kappa(s):
            r = mp.sqrt(s)
            if fam == "se":
                return mp.exp(-s / 2)
            if fam == "matern12":
                return mp.exp(-r)
            if fam == "matern32":
                return (1 + mp.sqrt(3) * r) * mp.exp(-mp.sqrt(3) * r)
            return (1 + mp.sqrt(5) * r + 5 * s / 3) * mp.exp(-mp.sqrt(5) * r)
        Xu = [[f(v) for v in row] for row in c["Xu"]]
        Kuu = mp.matrix(M, M)
        for i in range(M):
            for j in range(i + 1):
                s = mp.fsum(((Xu[i][d] - Xu[j][d]) / ell[d]) ** 2 for d in range(D))
                Kuu[i, j] = Kuu[j, i] = s2 * kappa(s) + (jit if i == j else 0)
        L = mp.cholesky(Kuu)
        mu = [[f(v) for v in c["mu_v"][o * M:(o + 1) * M]] for o in range(d_out)]
        Sig = c["Sigma_v"]
        Wm = mp.matrix(d_out, d_out)
        for i in range(d_out):
            for j in range(d_out):
                Wm[i, j] = f(c["W"][i, j])
        Wi = mp.inverse(Wm)
        Winv = np.array([[float(Wi[i, j]) for j in range(d_out)] for i in range(d_out)])
        mean, qff, form, C = [], [], [], []
        for p in points:
            x = [f(v) for v in c["X"][p]]
            k = [s2 * kappa(mp.fsum(((x[d] - Xu[m][d]) / ell[d]) ** 2 for d in range(D))) for m in range(M)]
            a = []
            for i in range(M):                                                # forward substitution L a = k
                a.append((k[i] - mp.fsum(L[i, j] * a[j] for j in range(i))) / L[i, i])
            q = s2 - mp.fsum(v * v for v in a)
            mean.append([float(mp.fdot(k, mu[o])) for o in range(d_out)])
            qff.append(float(q))
            F, Cp = np.empty((d_out, d_out)), np.empty((d_out, d_out))
            for i in range(d_out):
                for j in range(i, d_out):
                    rows = [mp.fdot(k, [f(v) for v in Sig[i * M + r, j * M:(j + 1) * M]]) for r in range(M)]
                    v = mp.fdot(k, rows)
                    F[i, j] = F[j, i] = float(v)
                    Cp[i, j] = Cp[j, i] = float(v + q if i == j else v)
            form.append(F)
            C.append(Cp)
    return np.array(mean).reshape(len(points), d_out), np.array(qff), np.array(form), np.array(C), Winv
