"""Masked statistics groups formed one step early (k_potrf_step, late_form): tile column c of P Lambda P with form step f >= 1 takes
Lambda0 + w Psi2 in from the trailing-update workgroups of step f - 1, behind their own rank-64 update, instead of from the panel and
diagonal workgroups of step f (the planner's choice per group; forced here for every group with SGP_EARLY_FORM=1).  The sums are the same term by term, so every case here must reproduce, BITWISE, what the library
computed before the change (tests/golden/early_formation.npz, recorded by tools/record_early_formation_golden.py with that
library in place), agree with the CPU oracle at the parity tests' bound, and keep the resident-statistics sweep, a repeated sweep
and the hand-off status as they were.

Shapes: N = 10 000 points (the smallest count at which the SYRK is taken to fill the chip, so that an overlapped plan exists),
D = 2, the groupings forced through SGP_OVERLAP_COLS and asserted through overlap_plan()."""
import os
import zlib

import numpy as np
import pytest

from oracle import sgp_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "early_formation.npz")
N, D = 10000, 2
S2, ELL, JITTER, PRIOR_VAR = 0.9, np.array([0.3, 0.25]), 1e-6, 50.0

# cols: SGP_OVERLAP_COLS; form: the form steps overlap_plan() must report ([] = no overlapped plan: MultiSGP sweeps in the plain order)
CASES = {
    "m192_cut1": dict(M=192, cols="1", form=[0, 1], w=300.0),                    # f = 1: step 0 stores the group's tiles
    "m192_cut2": dict(M=192, cols="2", form=[0, 2], w=300.0),
    "m256_cut12": dict(M=256, cols="1,2", form=[0, 1, 2], w=300.0),              # groups formed in consecutive steps
    "m256_cut13": dict(M=256, cols="1,3", form=[0, 1, 3], w=300.0),
    "m200_cut13": dict(M=200, cols="1,3", form=[0, 1, 3], w=300.0),              # padding inside the last tile column
    "m192_cut2_weights": dict(M=192, cols="2", form=[0, 2], w=120.0, weights=True),
    "multi_q256": dict(M=128, cols="1,2", form=[], d_out=2),                     # d_out = 2, Q = 256
}
ROWS = lambda Q: [0, Q // 2, Q - 1]


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def relF(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def post_tol(cond_L):
    """tests/test_gpu_parity.py's bound on the posterior: the north star's 1e-5, or cond(Lambda) * eps where that is tighter."""
    return min(1e-5, max(1e-9, 20 * np.finfo(float).eps * cond_L))


def inputs(name):
    c = CASES[name]
    M, Do = c["M"], c.get("d_out", 1)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    d = dict(X=X, Xu=Xu, Y=y, wts=None, Do=Do, M=M)
    if c.get("weights"):
        d["wts"] = rng.uniform(0.2, 1.0, N)
    if Do > 1:
        # 2 000 nodes of five weighted points each (the layout of a cubature rule), two outputs
        T, S = N // 5, 5
        wts = rng.uniform(0.5, 1.5, (T, S))
        d.update(T=T, S=S, wts=(wts / wts.sum(axis=1, keepdims=True)).reshape(-1),
                 Ynode=np.stack([y[::S], np.cos(X[::S, 0])], axis=1),
                 Sig_y=np.stack([np.diag(rng.uniform(0.01, 0.1, Do)) for _ in range(T)]))
        A = rng.normal(size=(Do, Do))
        d["W"] = A @ A.T + Do * np.eye(Do)
        d["E_logdetW"] = float(np.linalg.slogdet(d["W"])[1]) - 0.1
        d["xi0"] = 0.01 * rng.normal(size=Do * M)
    return d


def open_device(G, name, d, reuse_stats=False):
    c = CASES[name]
    dev = G.SGPDevice(N, c["M"], D, d_out=d["Do"], reuse_stats=reuse_stats)
    dev.set_inducing(d["Xu"])
    if d["Do"] == 1:
        dev.set_data(d["X"], d["Y"], None, d["wts"])
        dev.set_kernel(S2, ELL, JITTER)
        dev.set_prior_isotropic(PRIOR_VAR)
        dev.set_noise([[c["w"]]])
    else:
        dev.set_data(d["X"], np.repeat(d["Ynode"], d["S"], axis=0), None, d["wts"], n_nodes=d["T"])
        dev.set_output_cov_sum(d["Sig_y"].sum(axis=0))
        dev.set_kernel(S2, ELL, JITTER)
        dev.set_prior_precision(d["xi0"], np.eye(d["Do"] * c["M"]) / 10.0)
        dev.set_noise(d["W"], d["E_logdetW"])
    return dev


def snapshot(dev):
    """What a sweep leaves behind, raw.  The getters refuse (SGPError) when a bounded device-word wait gave up: reading them IS the
    check that the hand-off status word is clear."""
    mu, Sig, Uv = dev.posterior()
    sc = np.empty(8)
    dev._check(dev._lib.sgp_get_scalars(dev._h, sc.ctypes.data_as(dev._lib.sgp_get_scalars.argtypes[1])), "sgp_get_scalars")
    return dict(mu=mu, Sigma=Sig, Uv=Uv, scalars=sc)


def digest(snap, d):
    """The part of a snapshot that is kept as a fixture: mu, the scalars, three rows and a checksum of Sigma and of Uv; and a
    checksum of the inputs, so that a fixture recorded for other inputs is told apart from a wrong result."""
    Q = snap["mu"].size
    crc = lambda a: np.array([zlib.crc32(np.ascontiguousarray(a).tobytes())], dtype=np.int64)
    return dict(mu=snap["mu"], scalars=snap["scalars"], Sigma_rows=snap["Sigma"][ROWS(Q)], Uv_rows=snap["Uv"][ROWS(Q)],
                Sigma_crc=crc(snap["Sigma"]), Uv_crc=crc(snap["Uv"]),
                inputs_crc=crc(np.concatenate([d["X"].ravel(), d["Xu"].ravel(), np.ravel(d["Y"])])))


def run_case(G, name, monkeypatch=None):
    """Full sweep twice on one handle, full + resident-statistics sweep on a second one (SGP_FLAG_REUSE_STATS)."""
    c = CASES[name]
    # (SGP_EARLY_FORM=1: every masked group is added early, also where the planner's model would leave it to its form step)
    for k, v in (("SGP_OVERLAP_COLS", c["cols"]), ("SGP_EARLY_FORM", "1")):
        if monkeypatch is not None:
            monkeypatch.setenv(k, v)
        else:
            os.environ[k] = v
    d = inputs(name)
    with open_device(G, name, d) as a, open_device(G, name, d, reuse_stats=True) as b:
        plans = [a.overlap_plan(), b.overlap_plan()]
        a.sweep()
        first = snapshot(a)
        a.sweep()
        second = snapshot(a)
        b.sweep()
        full = snapshot(b)
        kind_next = b.sweep_kind()[0]
        b.sweep()
        kind_last = b.sweep_kind()[1]
        resident = snapshot(b)
    return d, plans, first, second, full, resident, (kind_next, kind_last)


def assert_bitwise(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} differs (max |diff| {np.max(np.abs(a[k] - b[k])):.3e})"


def oracle_check(name, d, snap):
    c = CASES[name]
    M, mu, Sig, Uv, sc = c["M"], snap["mu"], snap["Sigma"], snap["Uv"], snap["scalars"]
    if d["Do"] == 1:
        st = O.suff_stats(d["Xu"], d["X"], d["Y"], None, S2, ELL, omega=d["wts"])
        ref = O.vmp_sweep(d["Xu"], d["X"], d["Y"], None, S2, ELL, c["w"], jitter=JITTER, Lambda0=np.eye(M) / PRIOR_VAR,
                          xi0=np.zeros(M), stats=st)
        tol = post_tol(np.linalg.cond(np.eye(M) / PRIOR_VAR + c["w"] * st.Psi2))
        errs = dict(mu=relF(mu, ref.mu_v), Sigma=relF(Sig, ref.Sigma_v), Uv=relF(Uv, ref.Uv))
        print(f"{name}: tol {tol:.3g}", {k: f"{v:.3g}" for k, v in errs.items()}, "energy", sc[2], ref.energy, "I2", sc[1], ref.sum_I2)
        assert all(v < tol for v in errs.values()), (errs, tol)
        # (the energy carries w / 2 times sum I1 = s_kk - tr(Kuu^-1 Psi2), which cancels: cond(K_uu) * eps * s_kk, the bound of
        # test_gpu_psi_sweep and test_gpu_dims)
        Kuu = O.kernelmatrix(S2, ELL, d["Xu"]) + JITTER * np.eye(M)
        tol_I1 = 50 * np.finfo(float).eps * np.linalg.cond(Kuu) * st.s_kk
        print(f"{name}: energy bound", max(1e-7, tol) * abs(ref.energy) + 0.5 * c["w"] * tol_I1)
        assert abs(sc[2] - ref.energy) <= max(1e-7, tol) * abs(ref.energy) + 0.5 * c["w"] * tol_I1
    else:
        T, S, W = d["T"], d["S"], d["W"]
        pts, wts = d["X"].reshape(T, S, D), d["wts"].reshape(T, S)
        ms = O.multi_suff_stats(d["Xu"], pts, wts, d["Ynode"], d["Sig_y"], S2, ELL)
        mu_ref, Sig_ref = O.multi_v_update(ms, W, np.eye(2 * M) / 10.0, d["xi0"])
        errs = dict(mu=relF(mu, mu_ref), Sigma=relF(Sig, Sig_ref))
        print(f"{name}:", {k: f"{v:.3g}" for k, v in errs.items()})
        assert errs["mu"] < 1e-8 and errs["Sigma"] < 1e-8, errs          # (test_multisgp_sweep_matches_oracle's bounds)
        np.testing.assert_allclose(Uv.T @ Uv, Sig_ref + np.outer(mu_ref, mu_ref), rtol=1e-7, atol=1e-10)
        Kuu = O.kernelmatrix(S2, ELL, d["Xu"]) + JITTER * np.eye(M)
        Kinv = O.cholinv(Kuu)
        U_ref = 0.0
        for t in range(T):
            P0, P1, P2 = O.psi_statistics(d["Xu"], pts[t], wts[t], S2, ELL)
            U_ref += O.multi_average_energy(P0, P1, P2, d["Ynode"][t], d["Sig_y"][t], mu_ref, Sig_ref, W, d["E_logdetW"], Kinv)
        tol_I1 = 50 * np.finfo(float).eps * np.linalg.cond(Kuu) * S2 * T
        print(f"{name}: energy", sc[2], U_ref, "bound", 1e-7 * abs(U_ref) + 0.5 * np.trace(W) * tol_I1)
        assert abs(sc[2] - U_ref) <= 1e-7 * abs(U_ref) + 0.5 * np.trace(W) * tol_I1


@pytest.mark.parametrize("name", list(CASES))
def test_early_formed_groups_reproduce_the_recorded_sweep(G, name, monkeypatch):
    d, plans, first, second, full, resident, kinds = run_case(G, name, monkeypatch)
    for plan in plans:                                                   # the case is what it says before anything is trusted
        assert [g["form_step"] for g in plan] == CASES[name]["form"], plan
        assert all(g["masked"] == (1 if i else 0) for i, g in enumerate(plan))
    # 1. bitwise what the library computed before the groups were formed early
    gold = np.load(GOLDEN)
    got = digest(first, d)
    assert np.array_equal(got["inputs_crc"], gold[f"{name}/inputs_crc"]), "the fixture was recorded for other inputs"
    for k, v in got.items():
        assert np.array_equal(v, gold[f"{name}/{k}"]), f"{k} differs from the recorded sweep"
    # 2. the CPU oracle, at the parity tests' bound
    oracle_check(name, d, first)
    # 3. the sweep over resident statistics forms at the same places: bitwise the full sweep
    assert kinds == (2, 2), kinds                                        # (SGP_SWEEP_REUSED)
    assert_bitwise(full, first, "full sweep of the second handle")
    assert_bitwise(resident, full, "resident-statistics sweep")
    # 4. run to run
    assert_bitwise(second, first, "second sweep")
    # 5. the hand-off status word is clear: every getter above answered (snapshot), and the factorisations went through
    assert first["scalars"][3] == 0 and first["scalars"][4] == 0


def test_early_formed_group_behind_an_allreduce_hook(G, monkeypatch):
    """Data-sharded, on one GPU (as test_overlapped_sweep_with_one_reduce_per_statistics_group): the masked group comes back from
    its reduce through an event, which the stream now waits for in front of the step whose trailing workgroups add the group --
    step f - 1 -- and no kernel polls for the collective.  Cut {1}: f = 1, the wait sits in front of step 0."""
    torch = pytest.importorskip("torch")
    from gaussianprocessnode_amd.distributed import device_tensor
    M, w, cut = 192, 300.0, N
    monkeypatch.setenv("SGP_OVERLAP_COLS", "1")
    monkeypatch.setenv("SGP_EARLY_FORM", "1")
    rng = np.random.default_rng(77)
    X = rng.uniform(-1.745, 1.745, (2 * N, D))
    Xu = X[rng.permutation(2 * N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=2 * N)

    def make(sl):
        dev = G.SGPDevice(N, M, D)
        dev.set_inducing(Xu); dev.set_data(X[sl], y[sl]); dev.set_kernel(S2, ELL, JITTER)
        dev.set_prior_isotropic(PRIOR_VAR); dev.set_noise([[w]])
        return dev
    other, mine = make(slice(cut, 2 * N)), make(slice(0, cut))
    captured, streams = [], []

    def capture(ptr, n, stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            captured.append(device_tensor(ptr, n).clone())
        streams.append(stream)
    other.set_allreduce(capture)
    plan = other.overlap_plan()
    assert [g["form_step"] for g in plan] == [0, 1], plan
    other.sweep()
    torch.cuda.synchronize()
    assert len(captured) == 2 and len(set(streams)) == 2                  # one reduce per group, each on its group's stream
    calls = []

    def hook(ptr, n, stream):
        k = len(calls) % 2
        calls.append(n)
        with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            device_tensor(ptr, n).add_(captured[k])
    mine.set_allreduce(hook)
    assert [g["form_step"] for g in mine.overlap_plan()] == [0, 1]
    outs = []
    for _ in range(2):
        mine.sweep()
        outs.append(mine.posterior())
    sc = mine.scalars()                                                   # (refuses if a bounded wait gave up)
    mine.close(); other.close()
    assert calls == [c.numel() for c in captured] * 2
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    ref = O.vmp_sweep(Xu, X, y, None, S2, ELL, w, jitter=JITTER, Lambda0=np.eye(M) / PRIOR_VAR, xi0=np.zeros(M))
    tol = post_tol(np.linalg.cond(np.eye(M) / PRIOR_VAR + w * ref.stats.Psi2))
    mu, Sig, Uv = outs[0]
    errs = dict(mu=relF(mu, ref.mu_v), Sigma=relF(Sig, ref.Sigma_v), Uv=relF(Uv, ref.Uv))
    print(f"sharded: tol {tol:.3g}", {k: f"{v:.3g}" for k, v in errs.items()})
    assert all(v < tol for v in errs.values()), (errs, tol)
    Kuu = O.kernelmatrix(S2, ELL, Xu) + JITTER * np.eye(M)
    tol_I1 = 50 * np.finfo(float).eps * np.linalg.cond(Kuu) * ref.stats.s_kk          # (see oracle_check)
    assert abs(sc.energy - ref.energy) <= max(1e-7, tol) * abs(ref.energy) + 0.5 * w * tol_I1
