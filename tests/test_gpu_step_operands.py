"""The Cholesky step kernel's MFMA runs (k_potrf_step: the own rank-64 update of the solve group, trsm_update, the K-slices of X X^T) read their
LDS operands a k-step ahead of the products.  Only the reads moved: the products and their order per accumulator are the same, so
every case here must reproduce, BITWISE, what the library computed before the change (tests/golden/step_operands_*.npz, recorded by
tools/record_step_operands_golden.py with that library in place).

Shapes: the smallest at which each changed path runs -- N = 300 points (no multiple of anything the statistics kernels tile by),
D = 2, and
    M = 64   one tile column: the diagonal workgroup only (diag_inv, mma_left)
    M = 128  two: one panel block and its twins, fsyrk with all four K-slices
    M = 130  three (padded): n_valid inside a tile, an own update with j > 0, the trsm_update column blocks 1-3
    M = 256  four: a step with both twins and further panel blocks
each in the plain order, with SGP_OVERLAP_COLS and SGP_EARLY_FORM = 1 / 0 (the library overlaps only where its planner takes the
SYRK to fill the chip; the plan it reports is part of the fixture), with point weights, and with d_out = 2 (the MultiSGP chain,
Q = 2 M).  Arrays are kept for Q <= 128 (the triangle that carries them), SHA-256 digests of the full arrays for every case.
A Lambda that is not positive definite must report the same column as before."""
import hashlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, D = 300, 2
S2, ELL, JITTER, PRIOR_VAR, W = 0.9, np.array([0.3, 0.25]), 1e-6, 50.0, 300.0
SIZES = (64, 128, 130, 256)
# env: what the case sets; cols is filled in per M (every tile-column boundary but the first group's own)
MODES = {
    "plain": dict(env={"SGP_OVERLAP": "0"}),
    "overlap_early": dict(env={"SGP_EARLY_FORM": "1"}, cols=True),
    "overlap_late": dict(env={"SGP_EARLY_FORM": "0"}, cols=True),
    "weights": dict(env={}, weights=True),
    "dout2": dict(env={}, d_out=2),
}
CASES = [(M, mode) for M in SIZES for mode in MODES]
# (name, M, what makes Lambda indefinite): a prior precision with one negative diagonal entry in the second tile column of either
# order; the negative noise precision of test_gpu_parity at this file's shapes
INDEFINITE = [("prior_m130", 130, "prior"), ("prior_m256", 256, "prior"), ("noise_m130", 130, "noise")]


def golden_path(M):
    return os.path.join(GOLDEN_DIR, f"step_operands_m{M}.npz")


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def inputs(M, mode):
    m = MODES[mode]
    Do = m.get("d_out", 1)
    rng = np.random.default_rng(zlib.crc32(f"{M}/{mode}".encode()))
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    d = dict(X=X, Xu=Xu, Y=y, wts=None, Do=Do, M=M)
    if m.get("weights"):
        d["wts"] = rng.uniform(0.2, 1.0, N)
    if Do > 1:
        T, S = N // 5, 5                                  # 60 nodes of five weighted points each, two outputs
        wts = rng.uniform(0.5, 1.5, (T, S))
        A = rng.normal(size=(Do, Do))
        d.update(T=T, S=S, wts=(wts / wts.sum(axis=1, keepdims=True)).reshape(-1),
                 Ynode=np.stack([y[::S], np.cos(X[::S, 0])], axis=1),
                 Sig_y=np.stack([np.diag(rng.uniform(0.01, 0.1, Do)) for _ in range(T)]),
                 W=A @ A.T + Do * np.eye(Do), xi0=0.01 * rng.normal(size=Do * M))
        d["E_logdetW"] = float(np.linalg.slogdet(d["W"])[1]) - 0.1
    return d


def open_device(G, d):
    dev = G.SGPDevice(N, d["M"], D, d_out=d["Do"])
    dev.set_inducing(d["Xu"])
    if d["Do"] == 1:
        dev.set_data(d["X"], d["Y"], None, d["wts"])
        dev.set_kernel(S2, ELL, JITTER)
        dev.set_prior_isotropic(PRIOR_VAR)
        dev.set_noise([[W]])
    else:
        dev.set_data(d["X"], np.repeat(d["Ynode"], d["S"], axis=0), None, d["wts"], n_nodes=d["T"])
        dev.set_output_cov_sum(d["Sig_y"].sum(axis=0))
        dev.set_kernel(S2, ELL, JITTER)
        dev.set_prior_precision(d["xi0"], np.eye(d["Do"] * d["M"]) / 10.0)
        dev.set_noise(d["W"], d["E_logdetW"])
    return dev


def set_env(M, mode, setenv):
    m = MODES[mode]
    for k in ("SGP_OVERLAP", "SGP_OVERLAP_COLS", "SGP_EARLY_FORM"):
        setenv(k, None)
    for k, v in m["env"].items():
        setenv(k, v)
    if m.get("cols"):
        ncol = (M + 63) // 64
        setenv("SGP_OVERLAP_COLS", ",".join(str(c) for c in range(1, ncol)) if ncol > 1 else "1")


def run_case(G, M, mode, setenv):
    """Three sweeps on one handle; returns (inputs, plan, the snapshot of each sweep)."""
    set_env(M, mode, setenv)
    d = inputs(M, mode)
    snaps = []
    with open_device(G, d) as dev:
        plan = dev.overlap_plan()
        for _ in range(3):
            dev.sweep()
            mu, Sig, Uv = dev.posterior()
            sc = dev.scalars()
            assert sc.info_kuu == 0 and sc.info_lambda == 0
            snaps.append(dict(mu_v=mu, Sigma_v=Sig, Uv=Uv, logdet_kuu=np.array([sc.logdet_kuu]),
                              logdet_lambda=np.array([sc.logdet_lambda])))
    return d, plan, snaps


def record(d, plan, snap):
    """What is kept of a case: digests of everything, the arrays themselves (Sigma's lower, Uv's upper triangle) for Q <= 128."""
    Q = snap["mu_v"].size
    out = {f"sha_{k}": sha(v) for k, v in snap.items()}
    out["sha_inputs"] = sha(np.concatenate([d["X"].ravel(), d["Xu"].ravel(), np.ravel(d["Y"])]))
    out["form_steps"] = np.array([g["form_step"] for g in plan], dtype=np.int64)
    out["logdet_kuu"], out["logdet_lambda"] = snap["logdet_kuu"], snap["logdet_lambda"]
    if Q <= 128:
        out["mu_v"] = snap["mu_v"]
        out["Sigma_v_tril"] = snap["Sigma_v"][np.tril_indices(Q)]
        out["Uv_triu"] = snap["Uv"][np.triu_indices(Q)]
    return out


def run_indefinite(G, M, kind, setenv):
    """(info of the PosDefException the posterior getter raises, or 0 if it does not raise)"""
    for k in ("SGP_OVERLAP", "SGP_OVERLAP_COLS", "SGP_EARLY_FORM"):
        setenv(k, None)
    d = inputs(M, "plain")
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(d["Xu"])
        dev.set_data(d["X"], d["Y"])
        dev.set_kernel(S2, ELL, JITTER)
        if kind == "prior":
            L0 = np.eye(M) / PRIOR_VAR
            L0[M // 2, M // 2] = -1e9
            dev.set_prior_precision(np.zeros(M), L0)
            dev.set_noise([[W]])
        else:
            dev.set_prior_isotropic(PRIOR_VAR)
            dev.set_noise([[-W]], 0.0)
        dev.sweep()
        try:
            dev.posterior()
        except G.PosDefException as e:
            return int(e.info)
    return 0


def _setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


@pytest.mark.parametrize("M,mode", CASES, ids=[f"m{M}-{mode}" for M, mode in CASES])
def test_sweep_is_bitwise_the_recorded_one(G, M, mode, monkeypatch):
    d, plan, snaps = run_case(G, M, mode, _setenv(monkeypatch))
    gold = np.load(golden_path(M))
    got = record(d, plan, snaps[0])
    assert np.array_equal(got["sha_inputs"], gold[f"{mode}/sha_inputs"]), "the fixture was recorded for other inputs"
    for k, v in got.items():
        assert np.array_equal(v, gold[f"{mode}/{k}"]), f"{k} differs from the recorded sweep"
    for s in snaps[1:]:                                                   # run to run
        for k in s:
            assert np.array_equal(s[k], snaps[0][k]), f"{k} differs between two sweeps of one handle"
    assert np.all(np.isfinite(snaps[0]["mu_v"])) and np.isfinite(snaps[0]["logdet_lambda"][0])


@pytest.mark.parametrize("name,M,kind", INDEFINITE, ids=[c[0] for c in INDEFINITE])
def test_non_positive_pivot_reports_the_recorded_column(G, name, M, kind, monkeypatch):
    info = run_indefinite(G, M, kind, _setenv(monkeypatch))
    want = int(np.load(golden_path(M))[f"indefinite/{name}"][0])
    assert want > 0, "the fixture must hold a failing column"
    assert info == want
