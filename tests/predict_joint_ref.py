"""NumPy / SciPy restatement of the joint predictive covariance (sgp_predict_joint) and of the posterior samples (sgp_sample_f), with
the cases and the error bounds the host file (tests/test_predict_joint_host.py) and the GPU files (tests/test_gpu_predict_joint*.py)
share.  Inputs are in_message_ref.make_shape_case's with one node of ns points (ragged M and Q, iso / ARD lengthscales, a
non-diagonal W, Sigma_v = 0.01 I + 0.02 U U' / rank); the kernel is test_kernel_family_host.matern's.

Row r = i ns + s is output i at point s.  With K = K(Xu, X*), A = L_K^-1 K through a Cholesky solve (no explicit inverse):
    qff(s, s')      = k(x_s, x_s') - A[:, s] . A[:, s']        bound 50 eps cond(K_uu) sigma2
    form_ij(s, s')  = K[:, s]' Sigma_v^(ij) K[:, s']           bound 50 eps cond(Sigma_v) sqrt(form_ii(s, s) form_jj(s', s'))
    cov[(i,s),(j,s')] = delta_ij qff(s, s') + form_ij(s, s')   bound: the sum of the two that enter
    noise           C_noise - C against delta_ss' W^-1         bound 2 spacing(|C_noise| + |W^-1|) + 4 eps max |W^-1|
-- the error model and constants of tests/predict_shapes_ref.py.  The jitter is SHARP_JITTER, so that cond(K_uu + jitter I) <= 1e6
and every entry, the off-block ones too, is compared at 1e-8 or less; the two cases named ill_* keep 1e-8.  W^-1 is the exact
inverse of the float64 W (rational arithmetic), rounded once.

Samples: with L = chol(cov + sample_jitter I), samples = vec(mean) + L eps.  The factor is held to the backward-error bound
    |L L' - (cov + s I)|_ij <= CHOL_C R eps (|L| |L'|)_ij
CHOL_C is 10 x the largest ratio SciPy's factor reaches on the sampling cases (SAMPLE_CASES, R <= 260) against a 60-digit product (the margin covers a blocked,
matrix-core summation order; measured by tests/test_predict_joint_host.py, recorded in profiles/predict_joint.txt), and the product
L eps to 50 eps |L| |eps|.

`evaluate(c, fault)` restates the faults a kernel on this path could have (FAULTS); the host file shows that each moves a compared
entry by more than 10 x its bound on every case where it can occur."""
import functools

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from tests import in_message_ref as R
from tests import predict_shapes_ref as PS

EPS = R.EPS
TB = 64
SHARP_JITTER = PS.SHARP_JITTER
COND_KUU_MAX = 1e6
FAMILIES = R.FAMILIES
# SciPy's largest |L L' - A|_ij / (R eps (|L| |L'|)_ij) over SAMPLE_CASES is 0.5302 (at R = 1: one square root;
# test_predict_joint_host.py measures it and holds this constant to it); 10 x that
CHOL_SCIPY_WORST = 0.5302
CHOL_C = 5.302
FAULTS = ["drop_k_row", "drop_65th_point", "unmirrored_upper", "tile_swapped", "kss_sigma2", "block_stride_mp", "noise_everywhere",
          "lc_upper"]

TILE_NS = (1, 63, 64, 65, 129)
TILE_M = (1, 63, 64, 65, 129)
CASES = {}
for _ns in TILE_NS:
    for _M in TILE_M:
        for _do in (1, 3):
            CASES[f"tile{_ns}x{_M}x{_do}"] = dict(group="tile", M=_M, D=3, d_out=_do, family="se", sizes=[_ns],
                                                  seed=2100 + 1000 * _do + 10 * _M + _ns)
for _f, _fam in enumerate(FAMILIES):
    for _do in (1, 2, 3, 4):
        CASES[f"{_fam}x{_do}"] = dict(group="family", M=65, D=9, d_out=_do, family=_fam, sizes=[70], seed=2300 + 10 * _f + _do)
for _D in (1, 5, 32):
    for _iso in (False, True):
        CASES[f"dim{_D}{'iso' if _iso else ''}"] = dict(group="dims", M=70, D=_D, d_out=2, family="se", sizes=[130], seed=2400 + _D,
                                                        iso=_iso)
CASES["limit"] = dict(group="limit", M=1008, D=2, d_out=4, family="se", sizes=[70], seed=2500)
CASES["dup"] = dict(group="dup", M=65, D=3, d_out=2, family="se", sizes=[70], seed=2600)
CASES["ill_family"] = dict(CASES["matern32x3"], group="ill", jitter=1e-8)
CASES["ill_tile"] = dict(CASES["tile129x129x3"], group="ill", jitter=1e-8)
for _ns in (130, 257):
    CASES[f"chunk{_ns}"] = dict(group="chunk", M=70, D=4, d_out=2, family="matern52", sizes=[_ns], seed=2700 + _ns)
for _k in CASES.values():
    _k.setdefault("jitter", SHARP_JITTER)
DUP_PAIR = (5, 40)                        # the case "dup": point 40 is point 5
# the cases the sampling tests run (R = ns d_out <= 260)
SAMPLE_CASES = ["tile1x63x1", "tile64x64x1", "tile65x1x3", "tile63x129x3", "matern12x2", "sex3", "dup"]
N_GENERAL = 7


def group(name):
    return sorted(n for n, k in CASES.items() if k["group"] == name)


def make_case(name):
    """make_shape_case's inputs of a case, one node of ns points.  M = 1: the points lie 0.6 lengthscales about the one inducing
    input (predict_shapes_ref.make_case's reason: further out the forms fall below what the bounds resolve)."""
    kw = {k: v for k, v in CASES[name].items() if k != "group"}
    c = R.make_shape_case(**kw)
    rng = np.random.default_rng(kw["seed"] + 5000)
    if c["M"] == 1:
        c["X"] = c["Xu"][0] + 0.6 * c["ell"] * rng.normal(size=c["X"].shape)
    if CASES[name]["group"] == "dup":
        c["X"][DUP_PAIR[1]] = c["X"][DUP_PAIR[0]]
    c["name"] = name
    return c


def sample_jitter(c):
    """What the sampling tests pass: 1e-9 sigma2 (train.sample_posterior's default), 1e-6 sigma2 with the duplicated point."""
    return (1e-6 if CASES.get(c["name"], {}).get("group") == "dup" else 1e-9) * c["sigma2"]


def block_sizes(ns, d_out):
    """The (first row, size) of the covariance's blocks in tile order: (output, point block of 64)."""
    return [(i * ns + a, min(TB, ns - a)) for i in range(d_out) for a in range(0, ns, TB)]


def evaluate(c, fault=None):
    """dict(mean (ns, d_out), qff (ns, ns), form (d_out, d_out, ns, ns), C, C_noise (R, R), Winv, K) of a case in float64.
    fault: None, or one of FAULTS --
      drop_k_row        the last row of K(Xu, X*) takes no part in z or the forms
      drop_65th_point   the 65th point (the first of the second point block) is not stored: its rows and columns stay zero
      unmirrored_upper  the tiles above the block diagonal are not written
      tile_swapped      a tile pair (a, b) of equally sized blocks written at (b, a) without transposing
      kss_sigma2        k(x_s, x_s') taken as sigma2 off the diagonal too
      block_stride_mp   the blocks of Sigma_v read at multiples of M_p (in_message_ref.padded_blocks)
      noise_everywhere  W^-1 added to every point pair, not only s == s'
      lc_upper          (samples only, see sample_reference) L_C read with what the factorisation leaves above its diagonal."""
    M, d_out = c["M"], c["d_out"]
    Mp = (M + TB - 1) // TB * TB
    kern = R.kernel_of(c)
    X = c["X"]
    ns = len(X)
    Kuu = kern(c["sigma2"], c["ell"], c["Xu"]) + c["jitter"] * np.eye(M)
    K = kern(c["sigma2"], c["ell"], c["Xu"], X)
    mus = PS.padded_mu(c["mu_v"], M, d_out, M)
    mean = K.T @ mus.T
    Kf = K
    if fault == "drop_k_row":
        Kf = K.copy()
        Kf[-1, :] = 0.0
    A = solve_triangular(cholesky(Kuu, lower=True), Kf, lower=True)
    Kss = np.full((ns, ns), c["sigma2"]) if fault == "kss_sigma2" else kern(c["sigma2"], c["ell"], X, X)
    Kss[np.diag_indices(ns)] = c["sigma2"]
    qff = Kss - A.T @ A
    Sig = np.asarray(c["Sigma_v"])
    if fault == "block_stride_mp":
        Sig = R.padded_blocks(Sig, M, d_out, Mp)
    form = np.empty((d_out, d_out, ns, ns))
    for i in range(d_out):
        for j in range(d_out):
            form[i, j] = Kf.T @ (Sig[i * M:(i + 1) * M, j * M:(j + 1) * M] @ Kf)
    C = form.transpose(0, 2, 1, 3).reshape(ns * d_out, ns * d_out).copy()
    for i in range(d_out):
        C[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns] += qff
    Winv = PS.exact_inverse(np.asarray(c["W"]))
    point_eye = np.ones((ns, ns)) if fault == "noise_everywhere" else np.eye(ns)
    C_noise = C + np.kron(Winv, point_eye)
    blocks = block_sizes(ns, d_out)
    for M_ in (C, C_noise):
        if fault == "drop_65th_point":
            for i in range(d_out if ns > TB else 0):
                M_[i * ns + TB, :] = 0.0
                M_[:, i * ns + TB] = 0.0
        elif fault == "unmirrored_upper":
            for bi, (r0, rs) in enumerate(blocks):
                for c0, cs in blocks[bi + 1:]:
                    M_[r0:r0 + rs, c0:c0 + cs] = 0.0
        elif fault == "tile_swapped":
            src = M_.copy()
            for bi, (r0, rs) in enumerate(blocks):
                for c0, cs in blocks[:bi]:
                    if rs == cs:
                        M_[r0:r0 + rs, c0:c0 + cs] = src[c0:c0 + cs, r0:r0 + rs]
                        M_[c0:c0 + cs, r0:r0 + rs] = src[r0:r0 + rs, c0:c0 + cs]
    return dict(mean=mean, qff=qff, form=form, C=C, C_noise=C_noise, Winv=Winv, K=K)


def fault_applies(c, fault):
    """Whether a fault can show in a case (the host file demands that it then does).  tile_swapped needs a tile that is not its
    own transpose: two full point blocks of one output, or two outputs' blocks of the same points -- whose tile k_s sigma_ij k_s'
    is symmetric when M = 1."""
    ns, d_out, M = len(c["X"]), c["d_out"], c["M"]
    return {"drop_k_row": True, "drop_65th_point": ns > TB, "unmirrored_upper": ns * d_out > min(ns, TB),
            "tile_swapped": (d_out > 1 and ns > 1 and M > 1) or ns >= 2 * TB, "kss_sigma2": ns > 1, "block_stride_mp": d_out > 1 and M % TB != 0,
            "noise_everywhere": ns > 1, "lc_upper": ns * d_out > 1}[fault]


def bounds(c, ref, cond_kuu, cond_sigma):
    """b_cov (R, R): 50 eps cond(Sigma_v) sqrt(form_ii(s, s) form_jj(s', s')) + delta_ij 50 eps cond(K_uu) sigma2; b_qff."""
    ns, d_out = len(c["X"]), c["d_out"]
    diag = np.sqrt(np.concatenate([np.diag(ref["form"][i, i]) for i in range(d_out)]))
    b_qff = 50 * EPS * cond_kuu * c["sigma2"]
    b_cov = 50 * EPS * cond_sigma * np.outer(diag, diag) + b_qff * np.kron(np.eye(d_out), np.ones((ns, ns)))
    return dict(b_cov=b_cov, b_qff=b_qff)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests compare against for one case, computed once per process, arrays read-only."""
    c = make_case(name)
    cond_kuu, cond_sigma = PS.conditions(c)
    ref = evaluate(c)
    c.update(ref, cond_kuu=cond_kuu, cond_sigma=cond_sigma, **bounds(c, ref, cond_kuu, cond_sigma))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


worst = PS.worst


def cov_ratio(c, cov, truth=None):
    """Worst error / bound over EVERY entry of the R x R covariance."""
    return worst(np.abs(np.asarray(cov) - (c["C"] if truth is None else truth)), c["b_cov"])


def noise_ratio(c, cov_noise, cov, truth=None):
    """Worst error / bound of C_noise - C against delta_ss' W^-1 (or `truth`: another restatement's difference)."""
    ns = len(c["X"])
    want = np.kron(c["Winv"], np.eye(ns)) if truth is None else truth
    big = np.kron(np.abs(c["Winv"]), np.ones((ns, ns)))
    bound = 2 * np.spacing(np.abs(cov_noise) + big) + 4 * EPS * np.abs(c["Winv"]).max()
    return worst(np.abs((np.asarray(cov_noise) - np.asarray(cov)) - want), bound)


def diag_blocks(cov, ns, d_out):
    """(ns, d_out, d_out): the blocks cov[(., s), (., s)] -- what sgp_predict_var returns per point."""
    idx = np.arange(d_out)[:, None] * ns + np.arange(ns)[None, :]              # [i][s]
    return cov[idx.T[:, :, None], idx.T[:, None, :]]


def diag_block_bounds(c):
    """(ns, d_out, d_out): b_cov on the diagonal blocks."""
    return diag_blocks(np.asarray(c["b_cov"]), len(c["X"]), c["d_out"])


# ------------------------------------------------------------------------------------------------
# samples
def chol_ratio(L, A):
    """Largest |L L' - A|_ij / (n eps (|L| |L'|)_ij) over the lower triangle (what a factorisation reads) of a lower factor L, the
    product taken in extended precision (the device check; the host file takes it at 60 digits)."""
    L = np.tril(L)
    n = len(L)
    Ll = L.astype(np.longdouble)
    err = np.abs(Ll @ Ll.T - np.asarray(A, dtype=np.longdouble)).astype(np.float64)
    low = np.tril_indices(n)
    return worst(err[low], (n * EPS * (np.abs(L) @ np.abs(L).T))[low])


def sample_reference(c, eps, cov=None, fault=None):
    """(L, vec(mean) + L eps) for eps (R, n): L = chol(cov + sample_jitter I) of the reference's cov (or the one given)."""
    A = np.array(c["C"] if cov is None else cov) + sample_jitter(c) * np.eye(len(c["C"]))
    L = cholesky(A, lower=True)
    Lu = L + np.triu(A, 1) if fault == "lc_upper" else L
    return L, c["mean"].T.reshape(-1)[:, None] + Lu @ eps


def general_eps(c, n=N_GENERAL):
    return np.random.default_rng(CASES[c["name"]]["seed"] + 9000).normal(size=(len(c["C"]), n))


# ------------------------------------------------------------------------------------------------
# the same values at 60 digits
def mp_entries(c, count=10):
    """The (r, r') the mpmath comparison takes: the corners, the diagonal's ends and entries spread over the matrix -- of a case
    with a duplicated point the pair itself."""
    n = len(c["C"])
    rng = np.random.default_rng(CASES[c["name"]]["seed"] + 7000)
    pairs = {(0, 0), (n - 1, 0), (n - 1, n - 1), (n // 2, n // 2)} | {tuple(p) for p in rng.integers(0, n, size=(count, 2))}
    if CASES[c["name"]]["group"] == "dup":
        pairs.add((DUP_PAIR[1], DUP_PAIR[0]))
    return sorted(pairs)


def mp_evaluate(c, pairs):
    """cov and W^-1-difference of the listed entries at 60 digits (mpmath), each rounded once at the end."""
    import mpmath as mp
    M, D, d_out, fam = c["M"], c["D"], c["d_out"], c["family"]
    ns = len(c["X"])
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

        def kfun(a, b):
            return s2 * kappa(mp.fsum(((a[d] - b[d]) / ell[d]) ** 2 for d in range(D)))
        Xu = [[f(v) for v in row] for row in c["Xu"]]
        Kuu = mp.matrix(M, M)
        for i in range(M):
            for j in range(i + 1):
                Kuu[i, j] = Kuu[j, i] = kfun(Xu[i], Xu[j]) + (jit if i == j else 0)
        L = mp.cholesky(Kuu)
        Sig = c["Sigma_v"]
        cache = {}

        def point(s):
            if s not in cache:
                x = [f(v) for v in c["X"][s]]
                k = [kfun(x, Xu[m]) for m in range(M)]
                a = []
                for i in range(M):
                    a.append((k[i] - mp.fsum(L[i, j] * a[j] for j in range(i))) / L[i, i])
                cache[s] = (x, k, a)
            return cache[s]
        out = []
        for r, rr in pairs:
            i, s, j, t = r // ns, r % ns, rr // ns, rr % ns
            xs, ks, as_ = point(s)
            xt, kt, at = point(t)
            rows = [mp.fdot(kt, [f(v) for v in Sig[i * M + m, j * M:(j + 1) * M]]) for m in range(M)]
            v = mp.fdot(ks, rows)
            if i == j:
                v += (s2 if s == t else kfun(xs, xt)) - mp.fdot(as_, at)
            out.append(float(v))
    return np.array(out)


def mp_chol_ratio(L, A):
    """Largest |L L' - A|_ij / (n eps (|L| |L'|)_ij) with the product of the float64 factor taken at 60 digits."""
    import mpmath as mp
    L = np.tril(L)
    n = len(L)
    scale = n * EPS * (np.abs(L) @ np.abs(L).T)
    worst_ratio = 0.0
    with mp.workdps(60):
        rows = [[mp.mpf(float(v)) for v in L[i, :i + 1]] for i in range(n)]
        for i in range(n):
            for j in range(i + 1):
                d = abs(mp.fdot(rows[i][:j + 1], rows[j]) - mp.mpf(float(A[i, j])))
                worst_ratio = max(worst_ratio, float(d) / scale[i, j])
    return worst_ratio


# ---- the ledger of exported names (tests/call_sequence_ref.ENTRY_POINTS; tests/test_call_sequences_host.py holds it to the header).
# Both calls read the handle's kernel and q(v) and write nothing the sweep keeps, so they are readers; what stands behind the class
# is tests/test_gpu_predict_joint.py::test_both_calls_change_nothing_of_the_handle.
def register_entry_points():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_predict_joint", CR.READER)
    CR.ENTRY_POINTS.setdefault("sgp_sample_f", CR.READER)


register_entry_points()
