"""The fixtures and error bounds of test_gpu_envelope.py (sweeps and factorisations up to the d_out * M = 4032 limit of a handle),
and, CPU only, the proof that those bounds can see a bug: each fault a subtly wrong factorisation chain could make -- one
rank-64 update of a late step dropped, one Kronecker output block of a ragged Lambda shifted by a row, one per-step log-det
slot lost -- moves a quantity the GPU test checks by at least 100 x the bound it checks it with, on the same fixtures.

Bounds (each from the computed condition number, as test_gpu_parity.kuu_tol / post_tol):
  - K_uu factor: kuu_tol(cond K_uu); posterior: post_tol(cond Lambda);
  - log-determinants: logdet_tol = n eps (cond(A) + sum_c |log L_cc^2|) -- first order, logdet(A + dA) - logdet(A) =
    tr(A^-1 dA) <= n |A^-1| |dA| with a backward error |dA| ~ eps |A|, plus the rounding of a sum of n logarithms.
"""
import functools
import math

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, eigh

from oracle import sgp_oracle as O
from tests import multi_theta_ref as R
from tests.test_gpu_parity import kuu_tol, post_tol

EPS = np.finfo(np.float64).eps
TB = 64                                 # tile size of the factorisation chains
LIMIT = 4032                            # d_out * M of sgp_create
LOG2PI = math.log(2.0 * math.pi)


def relF(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def spd_cond(A):
    """2-norm condition number of a symmetric positive definite matrix (extreme eigenvalues)."""
    lo = eigh(A, eigvals_only=True, subset_by_index=[0, 0], driver="evr")[0]
    hi = eigh(A, eigvals_only=True, subset_by_index=[len(A) - 1, len(A) - 1], driver="evr")[0]
    return float(hi / lo)


def logdet_tol(L, cond):
    """Bound on |logdet_dev - logdet_ref| of the SPD matrix with (reference) lower factor L and condition number cond."""
    n = L.shape[0]
    return n * EPS * (cond + float(np.sum(np.abs(2.0 * np.log(np.diag(L))))))


def step_logdets(L):
    """The factorisation chain's per-step slots: 2 sum log L_cc over the 64 pivots of each step."""
    d = 2.0 * np.log(np.diag(L))
    return np.array([d[j:j + TB].sum() for j in range(0, len(d), TB)])


# ------------------------------------------------------------------------------------------------
# UniSGP fixture: D = 8, inputs and inducing inputs uniform over the box (spread: cond(K_uu) ~ 1e4 at M = 4032), jitter 1e-6
UNI_D, UNI_S2, UNI_ELL, UNI_JIT, UNI_W, UNI_PRIOR = 8, 0.8, 1.2, 1e-6, 5.0, 50.0


def uni_inputs(N, M, seed=0):
    rng = np.random.default_rng(1000 * M + seed)
    Xu = rng.uniform(-1.745, 1.745, (M, UNI_D))
    rng = np.random.default_rng(7 * N + M + seed)
    X = rng.uniform(-1.745, 1.745, (N, UNI_D))
    y = np.sin(X.sum(axis=1) / 2.0) + 0.1 * rng.normal(size=N)
    return X, Xu, y


@functools.lru_cache(maxsize=None)
def uni_kuu(M):
    """K_uu (jitter included), its condition number and slogdet: a function of M alone (the inducing inputs are)."""
    _, Xu, _ = uni_inputs(1, M)
    K = O.kernelmatrix(UNI_S2, np.full(UNI_D, UNI_ELL), Xu) + UNI_JIT * np.eye(M)
    return K, spd_cond(K), float(np.linalg.slogdet(K)[1])


@functools.lru_cache(maxsize=None)
def uni_reference(N, M):
    """The oracle sweep of the UniSGP fixture and what the GPU checks need from it (cached: several tests share it)."""
    X, Xu, y = uni_inputs(N, M)
    ell = np.full(UNI_D, UNI_ELL)
    ref = O.vmp_sweep(Xu, X, y, None, UNI_S2, ell, UNI_W, jitter=UNI_JIT, Lambda0=np.eye(M) / UNI_PRIOR, xi0=np.zeros(M))
    Kuu, cond_K, ld_K = uni_kuu(M)
    Lam = np.eye(M) / UNI_PRIOR + UNI_W * ref.stats.Psi2
    cond_L = spd_cond(Lam)
    L_lam = cholesky(Lam, lower=True)
    return dict(ref=ref, Lam=Lam, L_lam=L_lam, cond_K=cond_K, cond_L=cond_L, logdet_K=ld_K,
                logdet_L=float(np.linalg.slogdet(Lam)[1]), tol_ldK=logdet_tol(ref.KuuL, cond_K),
                tol_ldL=logdet_tol(L_lam, cond_L))


# ------------------------------------------------------------------------------------------------
# MultiSGP fixture: T nodes with Gaussian inputs (srcubature: 9 weighted points each in D = 4), inducing inputs spread over the box
MULTI_DIN, MULTI_S2, MULTI_ELL, MULTI_JIT = 4, 0.8, 0.5, 1e-8


def multi_inputs(d_out, M, T, seed=0):
    rng = np.random.default_rng(100 * d_out + M + seed)
    Din = MULTI_DIN
    Xu = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(Din)], axis=1)
    means = rng.uniform(-1.7, 1.7, (T, Din))
    covs = [np.diag(rng.uniform(0.002, 0.03, Din)) for _ in range(T)]
    cub = [O.srcubature(means[t], covs[t]) for t in range(T)]
    pts = np.stack([c[0] for c in cub])                    # (T, S, Din)
    wts = np.stack([c[1] for c in cub])                    # (T, S)
    Y = np.sin(means @ rng.normal(size=(Din, d_out))) + 0.05 * rng.normal(size=(T, d_out))
    Sig_y = np.stack([np.diag(rng.uniform(0.01, 0.1, d_out)) for _ in range(T)])
    A = rng.normal(size=(d_out, d_out))
    W = 5.0 * (A @ A.T / d_out + np.eye(d_out))
    return dict(Xu=Xu, pts=pts, wts=wts, Y=Y, Sig_y=Sig_y, W=W, E_logdetW=float(np.linalg.slogdet(W)[1]) - 0.1, T=T)


def multi_prior(kind, Q, seed=0):
    """(Lambda0, xi0) of a prior form, plus what the device is given: ("isotropic", variance), ("precision", xi0, Lambda0)
    or ("meancov", mu0, Sigma0)."""
    rng = np.random.default_rng(Q + seed)
    if kind == "isotropic":
        return np.eye(Q) / UNI_PRIOR, np.zeros(Q), ("isotropic", UNI_PRIOR)
    A = rng.normal(size=(Q, Q))
    S = A @ A.T / Q + 0.5 * np.eye(Q)                                   # eigenvalues in [0.5, 4.5]
    v = 0.3 * rng.normal(size=Q)
    if kind == "precision":
        return S, v, ("precision", v, S)
    Lam0 = O.cholinv(S)
    return Lam0, Lam0 @ v, ("meancov", v, S)


def multi_energy(ms, mu, Sig, W, E_logdetW, Kinv):
    """sum over the nodes of multi_average_energy, from the summed statistics (no per-node loop)."""
    d = W.shape[0]
    M = ms.Psi2.shape[0]
    Rv = Sig + np.outer(mu, mu)
    bw = (ms.B @ W).T.reshape(-1)                                       # vec(B W), output-major
    return (ms.n * (0.5 * d * LOG2PI - 0.5 * E_logdetW) + 0.5 * np.trace(W @ ms.Ryy)
            + 0.5 * np.trace(W) * (ms.s_kk - np.sum(Kinv * ms.Psi2)) - float(mu @ bw)
            + 0.5 * np.sum(ms.Psi2 * R.sum_rv_wbar(Rv, W, M)))


@functools.lru_cache(maxsize=None)
def multi_reference(d_out, M, T, prior, gauss_out):
    """Oracle of one MultiSGP sweep, and of the sweep after carry_posterior on the same data (summed statistics only)."""
    f = multi_inputs(d_out, M, T)
    Q = d_out * M
    ell = np.full(MULTI_DIN, MULTI_ELL)
    ms = O.multi_suff_stats(f["Xu"], f["pts"], f["wts"], f["Y"], f["Sig_y"] if gauss_out else None, MULTI_S2, ell)
    Lam0, xi0, dev_prior = multi_prior(prior, Q)
    W = f["W"]
    mu, Sig = O.multi_v_update(ms, W, Lam0, xi0)
    Kuu = O.kernelmatrix(MULTI_S2, ell, f["Xu"]) + MULTI_JIT * np.eye(M)
    Kinv = O.cholinv(Kuu)
    Lam = Lam0 + np.kron(W, ms.Psi2)
    xi = xi0 + (ms.B @ W).T.reshape(-1)
    L_lam = cholesky(Lam, lower=True)
    cond_K, cond_L = spd_cond(Kuu), spd_cond(Lam)
    mu2, Sig2 = O.multi_v_update(ms, W, Lam, xi)                        # prior <- posterior, same data again
    Lam2 = Lam + np.kron(W, ms.Psi2)
    return dict(f=f, ms=ms, Lam0=Lam0, xi0=xi0, dev_prior=dev_prior, mu=mu, Sig=Sig, Kuu=Kuu, Lam=Lam, L_lam=L_lam,
                S_w=O.multi_w_update(ms, mu, Sig, Kinv), energy=multi_energy(ms, mu, Sig, W, f["E_logdetW"], Kinv),
                cond_K=cond_K, cond_L=cond_L, logdet_K=float(np.linalg.slogdet(Kuu)[1]),
                logdet_L=float(np.linalg.slogdet(Lam)[1]), tol_ldK=logdet_tol(cholesky(Kuu, lower=True), cond_K),
                tol_ldL=logdet_tol(L_lam, cond_L), mu2=mu2, Sig2=Sig2, cond_L2=spd_cond(Lam2),
                logdet_L2=float(np.linalg.slogdet(Lam2)[1]))


def reversed_padded(Lam, Qp):
    """The matrix the Lambda chain factors: Lambda padded with identity to Qp, in index-reversed order (P Lambda P)."""
    Q = Lam.shape[0]
    A = np.eye(Qp)
    A[:Q, :Q] = Lam
    return A[::-1, ::-1].copy()


# ------------------------------------------------------------------------------------------------
def test_summed_multi_energy_is_the_per_node_sum():
    """multi_energy (used at the limit, where the per-node loop would cost minutes) against the oracle's per-node
    multi_average_energy on a small fixture."""
    d_out, M, T = 3, 20, 30
    f = multi_inputs(d_out, M, T, seed=1)
    ell = np.full(MULTI_DIN, MULTI_ELL)
    ms = O.multi_suff_stats(f["Xu"], f["pts"], f["wts"], f["Y"], f["Sig_y"], MULTI_S2, ell)
    Lam0, xi0, _ = multi_prior("precision", d_out * M)
    mu, Sig = O.multi_v_update(ms, f["W"], Lam0, xi0)
    Kinv = O.cholinv(O.kernelmatrix(MULTI_S2, ell, f["Xu"]) + MULTI_JIT * np.eye(M))
    loop = sum(O.multi_average_energy(*O.psi_statistics(f["Xu"], f["pts"][t], f["wts"][t], MULTI_S2, ell), f["Y"][t],
                                      f["Sig_y"][t], mu, Sig, f["W"], f["E_logdetW"], Kinv) for t in range(T))
    assert math.isclose(multi_energy(ms, mu, Sig, f["W"], f["E_logdetW"], Kinv), loop, rel_tol=1e-10)


def test_fixtures_are_well_conditioned():
    """cond(K_uu) stays well under 1e10 at every size the GPU file sweeps, so the bounds are tight."""
    for M in (2049, 3001, 4032):
        assert uni_kuu(M)[1] < 1e7, (M, uni_kuu(M)[1])
    for d_out, M in ((2, 2016), (3, 1344), (4, 1008), (4, 1000)):
        f = multi_inputs(d_out, M, 2)
        K = O.kernelmatrix(MULTI_S2, np.full(MULTI_DIN, MULTI_ELL), f["Xu"]) + MULTI_JIT * np.eye(M)
        assert spd_cond(K) < 1e8, (d_out, M)


def _drop_update(A, L, j, i=None):
    """The factor a chain computes when step j skips the rank-64 update of tile (i, i) (default: the step's diagonal tile) by
    panel j - 1: the Cholesky factor of A with L_{i,j-1} L_{i,j-1}^T added back to that tile (the earlier panels are unchanged)."""
    i = j if i is None else i
    r, p = slice(TB * i, TB * (i + 1)), slice(TB * (j - 1), TB * j)
    E = np.zeros_like(A)
    E[r, r] = L[r, p] @ L[r, p].T
    return cholesky(A + E, lower=True)


@pytest.mark.parametrize("step", [33, 47, 62])
def test_a_dropped_late_update_is_seen(step):
    """M = 4032 (63 steps): one rank-64 update of step j >= 33 dropped in the K_uu chain moves the K_uu factor and logdet_kuu,
    in the Lambda chain mu_v and logdet_lambda, by >= 100 x the bounds of test_gpu_envelope.test_unisgp_sweep_at_the_limit."""
    N, M = 3000, 4032
    r = uni_reference(N, M)
    Kuu = uni_kuu(M)[0]
    LK = r["ref"].KuuL
    LK_bad = _drop_update(Kuu, LK, step)
    assert relF(LK_bad, LK) > 100 * kuu_tol(r["cond_K"]), (relF(LK_bad, LK), kuu_tol(r["cond_K"]))
    ld_bad = 2.0 * np.log(np.diag(LK_bad)).sum()
    assert abs(ld_bad - r["logdet_K"]) > 100 * r["tol_ldK"], (ld_bad - r["logdet_K"], r["tol_ldK"])
    # the Lambda chain factors P Lambda P
    A = reversed_padded(r["Lam"], M)
    LA = cholesky(A, lower=True)
    LA_bad = _drop_update(A, LA, step)
    xi = UNI_W * r["ref"].stats.b[:, 0]
    mu_bad = cho_solve((LA_bad, True), xi[::-1])[::-1]
    tol = post_tol(r["cond_L"])
    assert relF(mu_bad, r["ref"].mu_v) > 100 * tol, (relF(mu_bad, r["ref"].mu_v), tol)
    ldl_bad = 2.0 * np.log(np.diag(LA_bad)).sum()
    assert abs(ldl_bad - r["logdet_L"]) > 100 * r["tol_ldL"], (ldl_bad - r["logdet_L"], r["tol_ldL"])


def test_a_dropped_logdet_slot_is_seen():
    """Each per-step log-det slot of either chain, left out of the sum, moves logdet_kuu / logdet_lambda by >= 100 x the bound,
    at the UniSGP limit and in the ragged MultiSGP case (whose first Lambda step is half padding)."""
    r = uni_reference(3000, 4032)
    slots_K = step_logdets(r["ref"].KuuL)
    slots_L = step_logdets(cholesky(reversed_padded(r["Lam"], 4032), lower=True))
    assert len(slots_K) == len(slots_L) == 63
    assert np.abs(slots_K).min() > 100 * r["tol_ldK"], (np.abs(slots_K).min(), r["tol_ldK"])
    assert np.abs(slots_L).min() > 100 * r["tol_ldL"], (np.abs(slots_L).min(), r["tol_ldL"])
    m = multi_reference(4, 1000, *MULTI_RAGGED)
    slots = step_logdets(cholesky(reversed_padded(m["Lam"], 4032), lower=True))
    assert len(slots) == 63
    assert np.abs(slots).min() > 100 * m["tol_ldL"], (np.abs(slots).min(), m["tol_ldL"])


MULTI_RAGGED = (420, "isotropic", False)          # (T, prior, Gaussian q_out) of the (d_out, M) = (4, 1000) case


@pytest.mark.parametrize("a,b", [(0, 0), (1, 2), (3, 3), (0, 3)])
def test_a_mis_mapped_kronecker_block_is_seen(a, b):
    """(d_out, M) = (4, 1000): Q = 4000 in Qp = 4032, so no output block starts on a tile boundary.  Block (a, b) of W (x) Psi2
    formed one row off (psi of row i - 1 at row i; the upper triangle of Lambda read -- the lower one of P Lambda P, as the chain
    does) moves mu_v or makes
    Lambda indefinite (info != 0, which the GPU test also checks) -- by >= 100 x post_tol."""
    m = multi_reference(4, 1000, *MULTI_RAGGED)
    M, W, Psi2 = 1000, m["f"]["W"], m["ms"].Psi2
    Lam = m["Lam"].copy()
    rows, cols = slice(a * M, (a + 1) * M), slice(b * M, (b + 1) * M)
    Lam[rows, cols] += W[a, b] * (np.roll(Psi2, 1, axis=0) - Psi2)
    Lam = np.triu(Lam) + np.triu(Lam, 1).T
    xi = m["xi0"] + (m["ms"].B @ W).T.reshape(-1)
    try:
        mu_bad = cho_solve((cholesky(Lam, lower=True), True), xi)
    except np.linalg.LinAlgError:
        mu_bad = None                                                    # not positive definite: info_lambda != 0
    tol = post_tol(m["cond_L"])
    assert mu_bad is None or relF(mu_bad, m["mu"]) > 100 * tol, (relF(mu_bad, m["mu"]), tol)
