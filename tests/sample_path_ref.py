"""NumPy / SciPy restatement of the pathwise (Matheron) posterior function samples (sgp_sample_path) through Cholesky solves, with the
cases and the error bound the host file (tests/test_sample_path_host.py) and the GPU file (tests/test_gpu_sample_path.py) share.
Inputs are in_message_ref.make_shape_case's (ragged M and Q, ARD lengthscales, Sigma_v = 0.01 I + 0.02 U U' / rank) with the jitter
SHARP_JITTER, so that cond(K_uu + jitter I) <= 1e6; the kernel is test_kernel_family_host.matern's.

With amp = sqrt(2 sigma2 / L), the arguments a_sl = phase_l + sum_d x_sd omega_dl / ell_d (inputs scaled by 1 / ell once, d ascending,
the sum started from phase_l), phi = amp cos(a), K = K_uu + jitter I = L_K L_K', Sigma_v = L_S L_S' and column c = (output i, sample j):
    v_j = mu_v + L_S eps_v[:, j]        T_c = K^-1 Phi_u w_c        C_c = v_j[iM:(i+1)M] - T_c
    f[s, i, j] = sum_l w_c[l] phi_l(x_s) + k(Xu, x_s)' C_c
Every entry has its own forward-error bound from the operand magnitudes, PATH_C eps times the sum of
    features   sum_l |w_l| amp (1 + (D + 2) (|phase_l| + sum_d |x_d omega_dl / ell_d|))     a cosine and its argument's roundings
    Gram       (D + 4) sum_m |k_sm| |C_m|                                                  the D-term distance and kappa
    draw       cond(Sigma_v) sum_m |k_sm| (|L_S| |eps_v|)_m                                the factor of Sigma_v
    solve      cond(K) sum_m |k_sm| |T_m|                                                  the two triangular solves
PATH_C is 20 x the worst ratio this restatement reaches against a 60-digit evaluation (mp_evaluate) over MP_CASES -- NumPy stays within
5 % of the bound; tests/test_sample_path_host.py measures it and holds the constant to it.

`evaluate(c, ..., fault=)` restates the faults a kernel on this path could have (FAULTS); the host file shows that each moves a
compared entry by more than 10 x its bound on every case where it can occur."""
import functools

import numpy as np
from scipy.linalg import cho_solve, cholesky

from tests import in_message_ref as R
from tests import predict_shapes_ref as PS

EPS = R.EPS
FAMILIES = R.FAMILIES
NU2 = {"matern12": 1, "matern32": 3, "matern52": 5}
# NumPy's worst error / (eps x the sum above) over MP_CASES, as tests/test_sample_path_host.py measures it, and 20 x that
PATH_NUMPY_WORST = 0.0475
PATH_C = 0.95
FAULTS = ["no_phase", "inv_ell_squared", "amp_no_2", "no_jitter", "no_mu", "eps_blocks_swapped"]

# the tile edges, a covering set: M, ns, L in {1, 5|63, 64, 65, 130|300|200}, J = d_out n_samples in {1, 3, 64, 65, 130}, D in
# {1, 2, 8, 9, 32}, every family
CASES = {}
for _k, (_M, _ns, _L, _do, _S, _D, _fam) in enumerate([
        (1, 1, 1, 1, 1, 1, "se"), (5, 63, 63, 3, 1, 2, "matern12"), (64, 64, 64, 4, 16, 8, "matern32"),
        (65, 65, 65, 1, 65, 9, "matern52"), (130, 300, 200, 2, 65, 32, "se"), (1, 300, 64, 2, 32, 8, "matern12"),
        (130, 1, 65, 3, 1, 1, "matern32"), (5, 64, 200, 1, 1, 32, "matern52"), (64, 65, 1, 1, 65, 2, "se"),
        (65, 63, 63, 4, 16, 9, "se")]):
    CASES[f"tile{_k}"] = dict(group="tile", M=_M, D=_D, d_out=_do, family=_fam, sizes=[_ns], seed=3100 + _k, L=_L, S=_S)
# the function property, the linear map, the state and refusal tests: 300 points, more than one chunk of 64 or 100
CASES["func"] = dict(group="func", M=70, D=3, d_out=2, family="matern52", sizes=[300], seed=3200, L=100, S=3)
CASES["uni"] = dict(group="func", M=48, D=2, d_out=1, family="se", sizes=[70], seed=3201, L=40, S=2)
# beyond SGP_JOINT_MAX_ROWS: ns d_out = 3 x 8192
CASES["large"] = dict(group="large", M=5, D=2, d_out=3, family="se", sizes=[8192], seed=3300, L=8, S=2)
for _c in CASES.values():
    _c.setdefault("jitter", PS.SHARP_JITTER)
MP_CASES = ["tile0", "tile1", "tile3", "tile8", "uni"]


def group(name):
    return sorted(n for n, k in CASES.items() if k["group"] == name)


def draw_features(family, D, L, rng):
    """(omega (D, L), phase (L,)): normals, divided by sqrt(chi2(2 nu) / (2 nu)) per feature for a Matern family; phase U[0, 2 pi)"""
    omega = rng.normal(size=(D, L))
    if family != "se":
        omega = omega / np.sqrt(rng.chisquare(NU2[family], L) / NU2[family])
    return omega, rng.uniform(0.0, 2.0 * np.pi, L)


def make_case(name):
    kw = {k: v for k, v in CASES[name].items() if k not in ("group", "L", "S")}
    c = R.make_shape_case(**kw)
    L, S = CASES[name]["L"], CASES[name]["S"]
    rng = np.random.default_rng(kw["seed"] + 5000)
    c["omega"], c["phase"] = draw_features(c["family"], c["D"], L, rng)
    c["feat_w"] = rng.normal(size=(L, c["d_out"], S))
    c["eps_v"] = rng.normal(size=(c["M"] * c["d_out"], S))
    c["name"], c["L"], c["S"] = name, L, S
    return c


def features(c, X, fault=None):
    """(phi (n, L), A (n, L)): the features at X and the magnitudes |phase_l| + sum_d |x_d omega_dl / ell_d| of their arguments"""
    ell = c["ell"] ** 2 if fault == "inv_ell_squared" else c["ell"]
    Xs = np.asarray(X, dtype=np.float64) / ell
    L = c["omega"].shape[1]
    t = np.zeros((len(Xs), L)) if fault == "no_phase" else np.broadcast_to(c["phase"], (len(Xs), L)).copy()
    A = np.broadcast_to(np.abs(c["phase"]), (len(Xs), L)).copy()
    for d in range(c["D"]):
        term = Xs[:, d:d + 1] * c["omega"][d][None, :]
        t = t + term
        A += np.abs(term)
    amp = np.sqrt((1.0 if fault == "amp_no_2" else 2.0) * c["sigma2"] / L)
    return amp * np.cos(t), A


def evaluate(c, X=None, feat_w=None, eps_v=None, fault=None, cond=None):
    """(f (n, d_out, S), bound (n, d_out, S)) at the points X (default: the case's) for the feature weights and normals given
    (default: the case's).  fault: None, or one of FAULTS --
      no_phase            the cosine's argument starts from 0
      inv_ell_squared     inputs scaled by 1 / ell^2
      amp_no_2            amplitude sqrt(sigma2 / L)
      no_jitter           the solve runs with K_uu, not K_uu + jitter I
      no_mu               v = L_S eps_v
      eps_blocks_swapped  output block i of eps_v read where block i + 1 (mod d_out) lies
    cond: (cond(K), cond(Sigma_v)) where the caller has them already."""
    M, D, d_out = c["M"], c["D"], c["d_out"]
    X = c["X"] if X is None else np.asarray(X, dtype=np.float64).reshape(-1, D)
    W = c["feat_w"] if feat_w is None else np.asarray(feat_w, dtype=np.float64)
    E = c["eps_v"] if eps_v is None else np.asarray(eps_v, dtype=np.float64)
    S, L = W.shape[2], W.shape[0]
    kern = R.kernel_of(c)
    Kuu = kern(c["sigma2"], c["ell"], c["Xu"])
    Kj = Kuu + c["jitter"] * np.eye(M)
    K = kern(c["sigma2"], c["ell"], c["Xu"], X)                          # M x n
    LS = cholesky(np.asarray(c["Sigma_v"]), lower=True)
    if fault == "eps_blocks_swapped":
        E = np.concatenate([E[((i + 1) % d_out) * M:((i + 1) % d_out + 1) * M] for i in range(d_out)])
    V = LS @ E + (0.0 if fault == "no_mu" else c["mu_v"][:, None])
    Vmag = np.abs(LS) @ np.abs(E)
    phi_u, _ = features(c, c["Xu"], fault)
    phi_s, A = features(c, X, fault)
    amp = np.sqrt(2.0 * c["sigma2"] / L)
    cond_k, cond_s = cond if cond is not None else PS.conditions(c)
    Lk = None if fault == "no_jitter" else cholesky(Kj, lower=True)
    f, bound = np.empty((len(X), d_out, S)), np.empty((len(X), d_out, S))
    per_term = amp * (1.0 + (D + 2) * A)                                 # n x L
    for i in range(d_out):
        B = phi_u @ W[:, i, :]
        T = np.linalg.solve(Kuu, B) if fault == "no_jitter" else cho_solve((Lk, True), B)
        C = V[i * M:(i + 1) * M] - T
        f[:, i, :] = phi_s @ W[:, i, :] + K.T @ C
        aK = np.abs(K.T)
        bound[:, i, :] = (per_term @ np.abs(W[:, i, :]) + (D + 4) * (aK @ np.abs(C)) + cond_s * (aK @ Vmag[i * M:(i + 1) * M])
                          + cond_k * (aK @ np.abs(T)))
    return f, PATH_C * EPS * bound


def fault_applies(c, fault):
    """Whether a fault can show in a case (the host file demands that it then does)"""
    return {"eps_blocks_swapped": c["d_out"] > 1, "inv_ell_squared": bool(np.any(c["ell"] != 1.0))}.get(fault, True)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests compare against for one case, computed once per process, arrays read-only."""
    c = make_case(name)
    c["cond"] = PS.conditions(c)
    c["f"], c["bound"] = evaluate(c, cond=c["cond"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


worst = PS.worst


def ratio(c, got, X=None, feat_w=None, eps_v=None, rows=None):
    """Worst error / bound over every entry of `got` (n, d_out, S) -- of the case's own reference, or of the inputs given (`rows`:
    the points of the case's X that `got` holds)."""
    if X is None and feat_w is None and eps_v is None:
        f, b = c["f"], c["bound"]
        if rows is not None:
            f, b = f[rows], b[rows]
    else:
        f, b = evaluate(c, c["X"][rows] if (X is None and rows is not None) else X, feat_w, eps_v, cond=c["cond"])
    return worst(np.abs(np.asarray(got) - f), b)


# ------------------------------------------------------------------------------------------------
# the same values at 60 digits
def mp_entries(c, count=6):
    n, d_out, S = len(c["X"]), c["d_out"], c["S"]
    rng = np.random.default_rng(CASES[c["name"]]["seed"] + 7000)
    picks = {(0, 0, 0), (n - 1, d_out - 1, S - 1)} | {(int(rng.integers(n)), int(rng.integers(d_out)), int(rng.integers(S)))
                                                     for _ in range(count)}
    return sorted(picks)


def mp_evaluate(c, entries):
    """f at the listed (s, i, j) at 60 digits (mpmath), each rounded once at the end"""
    import mpmath as mp
    M, D, d_out, fam, L = c["M"], c["D"], c["d_out"], c["family"], c["L"]
    with mp.workdps(60):
        f = lambda v: mp.mpf(float(v))
        ell = [f(v) for v in c["ell"]]
        s2, jit = f(c["sigma2"]), f(c["jitter"])
        amp = mp.sqrt(2 * s2 / L)

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
        om = [[f(c["omega"][d, l]) for d in range(D)] for l in range(L)]
        ph = [f(v) for v in c["phase"]]

        def phi(x):
            return [amp * mp.cos(ph[l] + mp.fsum(om[l][d] * x[d] / ell[d] for d in range(D))) for l in range(L)]
        Xu = [[f(v) for v in row] for row in c["Xu"]]
        Kuu = mp.matrix(M, M)
        for a in range(M):
            for b in range(a + 1):
                Kuu[a, b] = Kuu[b, a] = kfun(Xu[a], Xu[b]) + (jit if a == b else 0)
        phi_u = [phi(x) for x in Xu]
        Q = M * d_out
        Sig = mp.matrix(Q, Q)
        for a in range(Q):
            for b in range(Q):
                Sig[a, b] = f(c["Sigma_v"][a, b])
        LS = mp.cholesky(Sig)
        coef = {}

        def coefficients(i, j):
            if (i, j) not in coef:
                w = [f(v) for v in c["feat_w"][:, i, j]]
                e = [f(v) for v in c["eps_v"][:, j]]
                rhs = mp.matrix([mp.fdot(phi_u[m], w) for m in range(M)])
                T = mp.cholesky_solve(Kuu, rhs)
                v = [f(c["mu_v"][i * M + m]) + mp.fsum(LS[i * M + m, q] * e[q] for q in range(i * M + m + 1)) for m in range(M)]
                coef[(i, j)] = (w, [v[m] - T[m] for m in range(M)])
            return coef[(i, j)]
        out = []
        for s, i, j in entries:
            x = [f(v) for v in c["X"][s]]
            w, C = coefficients(i, j)
            out.append(float(mp.fdot(phi(x), w) + mp.fdot([kfun(x, Xu[m]) for m in range(M)], C)))
    return np.array(out)


# ---- the ledger of exported names (tests/call_sequence_ref.ENTRY_POINTS; tests/test_call_sequences_host.py holds it to the header).
# The call reads the handle's kernel and q(v) and writes nothing the sweep keeps, so it is a reader; what stands behind the class is
# tests/test_gpu_sample_path.py::test_nothing_the_sweep_keeps_is_written.
def register_entry_point():
    from tests import call_sequence_ref as CR
    CR.ENTRY_POINTS.setdefault("sgp_sample_path", CR.READER)


register_entry_point()
