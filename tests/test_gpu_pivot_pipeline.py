"""The pivot run of the Cholesky step kernel's 64 x 64 factorisation (potf2_tile, the `wave == cb` branch) is software-pipelined:
column k + 1 is fetched through the LDS crossbar BEFORE update k and corrected on the receiving lane, the row broadcast is one
64-bit DPP move, and pivot k is no longer copied aside per pivot but read back from the diagonal of the unnormalised column behind
the run.  Every entry is still defined by the same operations on the same operands -- only which lane performs a duplicate of
an update changed -- so every case here must reproduce, BITWISE, what the library computed before the change
(tests/golden/pivot_pipeline_*.npz, recorded by tools/record_pivot_pipeline_golden.py with that library in place).

Shapes: N = 300 points (no multiple of anything the statistics kernels tile by), D = 2, and
    M = 16, 17, 48, 64   one tile: partial, odd and full blocks of 16 pivots, n_valid inside a block
    M = 65, 80           a second tile that is nearly empty
    M = 128, 200         several steps, twins, deferred formation
each in the plain and in the overlapped order, plus sgp_potrf on a matrix of its own at the same M.  Arrays are kept for M <= 80,
SHA-256 digests of the full arrays for every case.
A non-positive pivot at columns 0, 1, 15, 16, 31, 47, 63 and 64 (first, second and last pivot of a run, every block of 16, the
second tile) must report the recorded column: the tested number now comes from the fetched-ahead, corrected column, and the
failure ballot reads it from the diagonal lanes.  An ill-conditioned K_uu (cond ~ 1e9) must stay bitwise the recording: the fetch-ahead relies on the
block staying bitwise symmetric, which is what keeps such a factorisation accurate."""
import hashlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, D = 300, 2
S2, ELL, JITTER, PRIOR_VAR, W = 0.9, np.array([0.3, 0.25]), 1e-6, 50.0, 300.0
SIZES = (16, 17, 48, 64, 65, 80, 128, 200)
KEEP_ARRAYS_UP_TO = 80
MODES = {
    "plain": dict(env={"SGP_OVERLAP": "0"}),
    "overlap": dict(env={"SGP_EARLY_FORM": "1"}, cols=True),
}
CASES = [(M, mode) for M in SIZES for mode in MODES]
BAD_COLUMNS = (0, 1, 15, 16, 31, 47, 63, 64)
M_BAD = 80                                                  # two tile columns: column 64 is the second tile's first pivot
# smooth kernel over the same box, small jitter: K_uu is numerically of low rank, cond = lambda_max / ~jitter
ILL_ELL, ILL_JITTER = np.array([3.0, 2.5]), 5e-8
ILL_SIZES = (64, 128)
ILL_CASES = [(M, mode) for M in ILL_SIZES for mode in MODES]
ENV_KEYS = ("SGP_OVERLAP", "SGP_OVERLAP_COLS", "SGP_EARLY_FORM")


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"pivot_pipeline_{name}.npz")


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def inputs(M, tag):
    rng = np.random.default_rng(zlib.crc32(f"pivot/{M}/{tag}".encode()))
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    return dict(X=X, Xu=Xu, Y=y, M=M)


def spd_matrix(M, tag):
    """A well-conditioned SPD matrix of its own for sgp_potrf (not a kernel matrix: dense, no structure)."""
    rng = np.random.default_rng(zlib.crc32(f"pivot/potrf/{M}/{tag}".encode()))
    B = rng.normal(size=(M, M + 3))
    return B @ B.T / M + 0.5 * np.eye(M)


def cond_kuu(Xu, ell, jitter):
    """2-norm condition number of the SE K_uu + jitter I (host, for the fixture's sanity check only)."""
    Z = Xu / ell
    d2 = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2)
    ev = np.linalg.eigvalsh(S2 * np.exp(-0.5 * d2) + jitter * np.eye(Xu.shape[0]))
    return float(ev[-1] / ev[0])


def set_env(M, mode, setenv):
    m = MODES[mode]
    for k in ENV_KEYS:
        setenv(k, None)
    for k, v in m["env"].items():
        setenv(k, v)
    if m.get("cols"):
        ncol = (M + 63) // 64
        setenv("SGP_OVERLAP_COLS", ",".join(str(c) for c in range(1, ncol)) if ncol > 1 else "1")


def run_sweeps(G, d, ell, jitter, want_chol=False):
    """Three sweeps on one handle; returns (plan, the snapshot of each sweep)."""
    snaps = []
    with G.SGPDevice(N, d["M"], D) as dev:
        dev.set_inducing(d["Xu"])
        dev.set_data(d["X"], d["Y"])
        dev.set_kernel(S2, ell, jitter)
        dev.set_prior_isotropic(PRIOR_VAR)
        dev.set_noise([[W]])
        plan = dev.overlap_plan()
        for _ in range(3):
            dev.sweep()
            mu, Sig, Uv = dev.posterior()
            sc = dev.scalars()
            assert sc.info_kuu == 0 and sc.info_lambda == 0
            snap = dict(mu_v=mu, Sigma_v=Sig, Uv=Uv, logdet_kuu=np.array([sc.logdet_kuu]),
                        logdet_lambda=np.array([sc.logdet_lambda]), energy=np.array([sc.energy]))
            if want_chol:
                snap["kuu_chol"] = dev.kuu_chol()
            snaps.append(snap)
    return plan, snaps


def run_case(G, M, mode, setenv):
    set_env(M, mode, setenv)
    d = inputs(M, mode)
    plan, snaps = run_sweeps(G, d, ELL, JITTER)
    return d, plan, snaps


def run_ill_case(G, M, mode, setenv):
    set_env(M, mode, setenv)
    d = inputs(M, f"ill/{mode}")
    plan, snaps = run_sweeps(G, d, ILL_ELL, ILL_JITTER, want_chol=True)
    return d, plan, snaps


def record(d, plan, snap):
    """What is kept of a case: digests of everything, the arrays themselves (Sigma's lower, Uv's upper triangle) for small M."""
    Q = snap["mu_v"].size
    out = {f"sha_{k}": sha(v) for k, v in snap.items()}
    out["sha_inputs"] = sha(np.concatenate([d["X"].ravel(), d["Xu"].ravel(), np.ravel(d["Y"])]))
    out["form_steps"] = np.array([g["form_step"] for g in plan], dtype=np.int64)
    for k in ("logdet_kuu", "logdet_lambda", "energy"):
        out[k] = snap[k]
    if Q <= KEEP_ARRAYS_UP_TO:
        out["mu_v"] = snap["mu_v"]
        out["Sigma_v_tril"] = snap["Sigma_v"][np.tril_indices(Q)]
        out["Uv_triu"] = snap["Uv"][np.triu_indices(Q)]
    return out


def record_potrf(A, L):
    out = {"sha_A": sha(A), "sha_L": sha(L)}
    if A.shape[0] <= KEEP_ARRAYS_UP_TO:
        out["L_tril"] = L[np.tril_indices(A.shape[0])]
    return out


def potrf_info(G, A):
    """(info of the PosDefException sgp_potrf raises, or 0 if it does not raise)"""
    try:
        G.potrf(A)
    except G.PosDefException as e:
        return int(e.info)
    return 0


def bad_matrix(c):
    A = spd_matrix(M_BAD, "bad")
    A[c, c] = -3.0
    return A


def sweep_info(G, c, setenv):
    """info of a plain-order sweep whose prior precision has a large negative entry at (c, c)"""
    set_env(M_BAD, "plain", setenv)
    d = inputs(M_BAD, "bad")
    with G.SGPDevice(N, M_BAD, D) as dev:
        dev.set_inducing(d["Xu"])
        dev.set_data(d["X"], d["Y"])
        dev.set_kernel(S2, ELL, JITTER)
        L0 = np.eye(M_BAD) / PRIOR_VAR
        L0[c, c] = -1e9
        dev.set_prior_precision(np.zeros(M_BAD), L0)
        dev.set_noise([[W]])
        dev.sweep()
        try:
            dev.posterior()
        except G.PosDefException as e:
            return int(e.info)
    return 0


def _setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def _compare(got, gold, prefix):
    assert np.array_equal(got["sha_inputs"], gold[f"{prefix}/sha_inputs"]), "the fixture was recorded for other inputs"
    for k, v in got.items():
        assert np.array_equal(v, gold[f"{prefix}/{k}"]), f"{k} differs from the recorded sweep"


def _same_run_to_run(snaps):
    for s in snaps[1:]:
        for k in s:
            assert np.array_equal(s[k], snaps[0][k]), f"{k} differs between two sweeps of one handle"


@pytest.mark.parametrize("M,mode", CASES, ids=[f"m{M}-{mode}" for M, mode in CASES])
def test_sweep_is_bitwise_the_recorded_one(G, M, mode, monkeypatch):
    d, plan, snaps = run_case(G, M, mode, _setenv(monkeypatch))
    _compare(record(d, plan, snaps[0]), np.load(golden_path(f"m{M}")), mode)
    _same_run_to_run(snaps)
    assert np.all(np.isfinite(snaps[0]["mu_v"])) and np.isfinite(snaps[0]["logdet_lambda"][0])


@pytest.mark.parametrize("M", SIZES, ids=[f"m{M}" for M in SIZES])
def test_potrf_is_bitwise_the_recorded_one(G, M):
    A = spd_matrix(M, "potrf")
    L = G.potrf(A)
    gold = np.load(golden_path(f"m{M}"))
    got = record_potrf(A, L)
    assert np.array_equal(got["sha_A"], gold["potrf/sha_A"]), "the fixture was recorded for another matrix"
    for k, v in got.items():
        assert np.array_equal(v, gold[f"potrf/{k}"]), f"{k} differs from the recorded factor"
    assert np.array_equal(G.potrf(A), L)
    assert np.all(np.isfinite(L)) and np.all(np.triu(L, 1) == 0.0)


@pytest.mark.parametrize("c", BAD_COLUMNS, ids=[f"col{c}" for c in BAD_COLUMNS])
def test_non_positive_pivot_reports_the_recorded_column(G, c, monkeypatch):
    gold = np.load(golden_path("indefinite"))
    want_potrf, want_sweep = int(gold[f"potrf/col{c}"][0]), int(gold[f"sweep/col{c}"][0])
    assert want_potrf == c + 1 and want_sweep > 0, "the fixture must hold the failing column (LAPACK: column + 1)"
    assert potrf_info(G, bad_matrix(c)) == want_potrf
    assert sweep_info(G, c, _setenv(monkeypatch)) == want_sweep


@pytest.mark.parametrize("M,mode", ILL_CASES, ids=[f"m{M}-{mode}" for M, mode in ILL_CASES])
def test_ill_conditioned_kuu_is_bitwise_the_recorded_one(G, M, mode, monkeypatch):
    d, plan, snaps = run_ill_case(G, M, mode, _setenv(monkeypatch))
    gold = np.load(golden_path("illcond"))
    cond = cond_kuu(d["Xu"], ILL_ELL, ILL_JITTER)
    assert 1e8 < cond < 1e10, f"cond(K_uu) = {cond:.3g}: the case is meant to be ill-conditioned (~1e9)"
    _compare(record(d, plan, snaps[0]), gold, f"m{M}/{mode}")
    _same_run_to_run(snaps)
    assert np.all(np.isfinite(snaps[0]["kuu_chol"])) and np.isfinite(snaps[0]["logdet_kuu"][0])
