"""Every launch plan of a sweep (sweep_plan, sweep_local_impl in csrc/sgp_api.hip), on purpose: caller streams, several live
handles, and the sizes on each side of gate_side, the word join's grid bound and the overlapped order (tests/sweep_plans.py).

Each test asserts the plan bits the library recorded (SGPDevice.sweep_plan) and then the results, two ways: against the CPU oracle
with the suite's bounds (post_tol(cond Lambda) on the posterior, cond(K_uu) eps s_kk on sum I1: tests/test_gpu_parity.py,
tests/test_gpu_early_formation.py; 1e-8 for d_out > 1: test_multisgp_sweep_matches_oracle), and BITWISE against the same state swept
alone -- one live handle, the library's own stream, SGP_OVERLAP=0 at create where the compared plan cannot overlap.  Events instead
of device words, a second handle, another host order of the enqueues change how the launches wait for each other, never what they
compute.

Ordering is made visible: before a sweep on a caller's stream a few milliseconds of unrelated torch work are enqueued on that stream
(sized once with torch events, against nothing in the library), and nothing synchronises between the sweep and the reader under
test.  Consecutive sweeps run at states whose oracle posteriors differ by 1e-3 or more (tests/test_sweep_plans_host.py)."""
import gc
import math

import numpy as np
import pytest

from tests import sweep_plans as P

pytestmark = pytest.mark.gpu

BUSY_MS = 5.0                      # the unrelated work in front of a caller-stream sweep, at least
TWINS = {}


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Busy:
    """`busy(stream)`: enqueue >= BUSY_MS of matrix products on `stream`.  Sized once from a timed run of the same products."""

    def __init__(self, torch):
        self.torch = torch
        self.x = torch.randn(4096, 4096, device="cuda")
        self.y = torch.empty_like(self.x)
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            for _ in range(3):
                torch.mm(self.x, self.x, out=self.y)
            e0.record(s)
            for _ in range(8):
                torch.mm(self.x, self.x, out=self.y)
            e1.record(s)
        e1.synchronize()
        per = e0.elapsed_time(e1) / 8
        self.reps = max(1, math.ceil(BUSY_MS / per))
        with torch.cuda.stream(s):
            e0.record(s)
            self(s)
            e1.record(s)
        e1.synchronize()
        self.ms = e0.elapsed_time(e1)
        print(f"busy: {self.reps} products of 4096^2 fp32, {self.ms:.2f} ms measured ({per:.3f} ms each)")
        assert self.ms >= 0.5 * BUSY_MS

    def __call__(self, stream):
        with self.torch.cuda.stream(stream):
            for _ in range(self.reps):
                self.torch.mm(self.x, self.x, out=self.y)


@pytest.fixture(scope="module")
def busy(torch):
    return Busy(torch)


@pytest.fixture
def streams(torch):
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    yield s
    torch.cuda.synchronize()


def live_handles():
    from gaussianprocessnode_amd import device
    gc.collect()
    return sum(1 for d in list(device._live) if d._h.value)


def make(G, mp, st, *, overlap=None, reuse=False):
    """a handle configured for `st`; overlap: None = only the case that is there for the overlapped order may overlap"""
    d = P.inputs(st.name, st.variant)
    overlap = P.CASES[st.name]["overlapped"] if overlap is None else overlap
    with mp.context() as m:
        if overlap:
            m.delenv("SGP_OVERLAP", raising=False)
        else:
            m.setenv("SGP_OVERLAP", "0")                   # (read once, by sgp_create)
        dev = G.SGPDevice(d["N"], d["M"], d["D"], d_out=d["Do"], reuse_stats=reuse, keep_kuf=d["Do"] == 1)
    P.configure(dev, st)
    return dev


def snap(dev):
    """What a sweep leaves behind, raw.  The getters refuse (SGPError) when a bounded device-word wait gave up."""
    mu, Sig, Uv = dev.posterior()
    sc = np.empty(8)
    dev._check(dev._lib.sgp_get_scalars(dev._h, sc.ctypes.data_as(dev._lib.sgp_get_scalars.argtypes[1])), "sgp_get_scalars")
    return dict(mu=mu, Sigma=Sig, Uv=Uv, scalars=sc)


def assert_bitwise(a, b, where):
    for k in b:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), f"{where}: {k} differs (max |diff| {np.max(np.abs(x - y)):.3e})"


def show(where, dev_or_bits, **figures):
    bits = dev_or_bits if isinstance(dev_or_bits, frozenset) else dev_or_bits.sweep_plan()
    print(f"plan {where}: [{' '.join(sorted(bits)) or '-'}]", " ".join(f"{k}={v:.3g}" for k, v in figures.items()))
    return bits


def check_oracle(st, s, where, carried=0):
    """the suite's bounds, nothing new; returns the largest error / bound"""
    o = P.oracle(st, carried)
    d = P.inputs(st.name)
    if d["Do"] == 1:
        tol = P.post_tol(o["cond_lambda"])
        errs = dict(mu=P.relF(s["mu"], o["mu"]), Sigma=P.relF(s["Sigma"], o["Sigma"]), Uv=P.relF(s["Uv"], o["Uv"]))
        e_energy = abs(s["scalars"][2] - o["energy"]) / (max(1e-7, tol) * abs(o["energy"]) + 0.5 * o["w"] * o["tol_I1"])
        e_I1 = abs(s["scalars"][0] - o["sum_I1"]) / (o["tol_I1"] + 1e-12)
        worst = max(max(errs.values()) / tol, e_energy, e_I1)
        print(f"oracle {where}: tol {tol:.3g}", {k: f"{v:.3g}" for k, v in errs.items()}, f"energy/bound {e_energy:.3g} I1/bound {e_I1:.3g}")
        assert all(v < tol for v in errs.values()), (where, errs, tol)
        assert e_energy <= 1 and e_I1 <= 1, (where, e_energy, e_I1)
        assert s["scalars"][3] == 0 and s["scalars"][4] == 0
    else:
        errs = dict(mu=P.relF(s["mu"], o["mu"]), Sigma=P.relF(s["Sigma"], o["Sigma"]))
        worst = max(errs.values()) / 1e-8
        print(f"oracle {where}:", {k: f"{v:.3g}" for k, v in errs.items()})
        assert errs["mu"] < 1e-8 and errs["Sigma"] < 1e-8, (where, errs)
    return worst


XS_SEED = 99


def query_points(d):
    rng = np.random.default_rng(XS_SEED)
    Xs = rng.uniform(-1.7, 1.7, (130, d["D"]))
    return Xs, np.arange(0, 131, 5), rng.normal(size=(26, d["Do"]))


READERS = {
    "posterior": lambda dev, d, t: dict(zip(("mu", "Sigma", "Uv"), dev.posterior())),
    "scalars": lambda dev, d, t: dict(scalars=snap(dev)["scalars"]),
    "stats": lambda dev, d, t: dict(zip(("Psi2", "B", "sc"), dev.stats())),
    "kuu_chol": lambda dev, d, t: dict(L=dev.kuu_chol()),
    "wishart_invscale": lambda dev, d, t: dict(S=dev.wishart_invscale()),
    "w_stats": lambda dev, d, t: dict(zip(("I1", "I2"), dev.w_stats())),
    "w_stats_stream": lambda dev, d, t: dict(zip(("I1", "I2"), dev.w_stats(t.cuda_stream))),
    "predict": lambda dev, d, t: dict(mean=dev.predict(query_points(d)[0])),
    "predict_var": lambda dev, d, t: dict(zip(("mean", "var"), dev.predict_var(query_points(d)[0]))),
    "in_message": lambda dev, d, t: dict(logpdf=dev.in_message(query_points(d)[0], query_points(d)[1], query_points(d)[2])),
    "out_message": lambda dev, d, t: dict(mean=dev.out_message(query_points(d)[0], query_points(d)[1])),
    "theta_objective": lambda dev, d, t: dict(zip(("value", "grad"), dev.theta_objective(want_grad=True))),
}
TWIN_READER = {"w_stats_stream": "w_stats"}                  # (alone, the same call on the library's own stream)


def twin(G, mp, cus, st, *, overlap=False, readers=()):
    """`st` swept alone: a new handle, no other alive, the library's own stream.  Shared between the tests; not to be written to."""
    key = (st, overlap)
    have = TWINS.get(key)
    if have is None or any("reader:" + r not in have for r in readers):
        assert live_handles() == 0, "a twin must be the only live handle (its plan takes the word join where the size allows)"
        d = P.inputs(st.name, st.variant)
        with make(G, mp, st, overlap=overlap) as dev:
            over = bool(dev.overlap_plan())
            dev.sweep()
            bits = dev.sweep_plan()
            assert bits == P.expected_bits(st.name, cus, overlapped=over), (st, bits)
            assert over == (overlap and P.CASES[st.name]["overlapped"]), (st, dev.overlap_plan())
            have = dict(snap(dev), bits=bits)
            for r in readers:
                have["reader:" + r] = READERS[TWIN_READER.get(r, r)](dev, d, None)
        if key in TWINS:
            have = {**TWINS[key], **have}
        TWINS[key] = have
    return have


def sweep_on(dev, busy, stream):
    """a sweep on `stream` (None: the library's own), the stream kept busy in front of it"""
    if stream is None:
        dev.sweep()
    else:
        busy(stream)
        dev.sweep(stream.cuda_stream)


# ---- (a) readers behind a sweep on a caller's stream ----------------------------------------------------------------------------
@pytest.mark.parametrize("reader", list(READERS))
def test_reader_right_after_a_sweep_on_a_callers_stream(G, torch, cus, busy, streams, monkeypatch, reader):
    name = "multi" if reader == "wishart_invscale" else "gated"
    d = P.inputs(name)
    old, new = P.step(name, 0), P.step(name, 1)
    alone = twin(G, monkeypatch, cus, new, readers=(reader,))
    t = streams[0]
    with make(G, monkeypatch, old) as dev:
        dev.sweep()                                        # (what a reader that did not wait would see: the results at `old`)
        P.set_kernel(dev, new)
        P.set_noise(dev, new)
        sweep_on(dev, busy, t)
        bits = dev.sweep_plan()
        got = READERS[reader](dev, d, t)                   # no synchronisation in between
        assert bits == P.expected_bits(name, cus, stream=True), bits
        assert_bitwise(got, alone["reader:" + reader], f"{reader} behind sweep(tstream)")
        worst = check_oracle(new, snap(dev), f"{name}/{reader}")
        o = P.oracle(new)
        if reader == "stats":
            assert P.relF(got["Psi2"], o["Psi2"]) < 1e-13 and P.relF(got["B"], o["B"]) < 1e-13
        if reader == "kuu_chol":
            assert P.relF(got["L"], o["KuuL"]) < max(1e-13, 0.05 * np.finfo(float).eps * o["cond_kuu"])
        if reader == "wishart_invscale":
            ref = o["wishart"]
            assert np.max(np.abs(got["S"] - ref)) <= 1e-7 * np.max(np.abs(ref)) + o["tol_I1"]
        if reader == "predict":
            from oracle import sgp_oracle as O
            ref = O.predict_mean(P.inducing_of(new), query_points(d)[0], o["mu"], *P.kernel_of(new))
            assert P.relF(got["mean"], ref) < max(1e-7, P.post_tol(o["cond_lambda"]))
        show(f"(a) {name} sweep(tstream) then {reader}", bits, err_over_bound=worst)


def test_sweep_kind_right_after_a_sweep_on_a_callers_stream(G, torch, cus, busy, streams, monkeypatch):
    st = P.step("gated", 1)
    alone = twin(G, monkeypatch, cus, st)
    with make(G, monkeypatch, st, reuse=True) as dev:
        sweep_on(dev, busy, streams[0])
        bits = dev.sweep_plan()
        assert dev.sweep_kind() == (2, 0)                  # next REUSED (it waits for the sweep and checks its status), last FULL
        assert bits == P.expected_bits("gated", cus, stream=True)
        assert_bitwise(snap(dev), {k: alone[k] for k in ("mu", "Sigma", "Uv", "scalars")}, "sweep_kind behind sweep(tstream)")
        show("(a) gated sweep(tstream) then sweep_kind", bits)


@pytest.mark.parametrize("carry_on_stream", [False, True], ids=["carry_own_then_sweep_tstream", "carry_tstream_then_sweep_own"])
def test_carry_posterior_across_streams(G, torch, cus, busy, streams, monkeypatch, carry_on_stream):
    """sweep(tstream), then carry_posterior() followed by sweep(tstream), or carry_posterior(tstream) followed by sweep(): nothing
    waited for in between.  The second sweep's prior has taken the first one's statistics in exactly once (the oracle with that
    prior), bitwise as on one stream."""
    st = P.step("gated", 2)
    t = streams[0]
    assert live_handles() == 0
    with make(G, monkeypatch, st, overlap=False) as dev:
        dev.sweep()
        dev.carry_posterior()
        dev.sweep()
        alone = snap(dev)
    with make(G, monkeypatch, st) as dev:
        first, second = t, (None if carry_on_stream else t)
        sweep_on(dev, busy, first)
        b1 = dev.sweep_plan()
        if carry_on_stream:
            busy(t)
        dev.carry_posterior(t.cuda_stream if carry_on_stream else 0)
        sweep_on(dev, busy, second)
        b2 = dev.sweep_plan()
        got = snap(dev)
    assert ("events" in b1) == (first is not None) and ("events" in b2) == (second is not None)
    worst = check_oracle(st, got, "carry across streams", carried=1)
    assert_bitwise(got, alone, "sweep, carry, sweep across streams")
    show(f"(a) gated carry on {'tstream' if carry_on_stream else 'own'}, second sweep", b2, err_over_bound=worst)


# ---- (b) setters under a queued sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ungated", "gated"])
def test_setters_under_a_queued_sweep_leave_it_its_own_parameters(G, torch, cus, busy, streams, monkeypatch, name):
    """A sweep queued behind busy work on a caller's stream reads the pinned parameter block, the prior, the targets and the inducing
    inputs WHEN IT RUNS: every setter must wait for it first.  After each setter the queued sweep's statistics, read from a buffer the
    caller bound (sgp_bind_stats), and its posterior, where the getters still hand it out (they refuse once the inducing inputs have
    changed), are those of the parameters before the call; the next sweep's are those after it."""
    s0 = P.step(name, 0)
    chain = [("set_kernel", s0._replace(kern=1)), ("set_noise", s0._replace(kern=1, noise=1)),
             ("set_prior_isotropic", s0._replace(kern=1, noise=1, prior="iso5")),
             ("set_prior_precision", s0._replace(kern=1, noise=1, prior="dense")),
             ("set_targets", s0._replace(kern=1, noise=1, prior="dense", targets=2)),
             ("set_inducing", s0._replace(kern=1, noise=1, prior="dense", targets=2, xu=1))]
    twins = [twin(G, monkeypatch, cus, st, readers=("stats",)) for st in [s0] + [c[1] for c in chain]]
    t = streams[0]
    M = P.inputs(name)["M"]
    with make(G, monkeypatch, s0) as dev:
        _, count, Mp = dev.stats_layout()
        buf = torch.zeros(count, dtype=torch.float64, device="cuda")
        dev.bind_stats(buf.data_ptr())
        for i, (setter, st) in enumerate(chain):
            sweep_on(dev, busy, t)
            bits = dev.sweep_plan()
            if setter == "set_kernel": P.set_kernel(dev, st)
            elif setter == "set_noise": P.set_noise(dev, st)
            elif setter == "set_targets": dev.set_targets(P.targets_of(st))
            elif setter == "set_inducing": dev.set_inducing(P.inducing_of(st))
            else: P.set_prior(dev, st)
            assert bits == P.expected_bits(name, cus, stream=True)
            raw = buf.cpu().numpy()
            bound = dict(Psi2=raw[:Mp * Mp].reshape(Mp, Mp)[:M, :M], B=raw[Mp * Mp:Mp * Mp + M].reshape(M, 1),
                         sc=raw[Mp * Mp + Mp:Mp * Mp + Mp + 8])
            assert_bitwise(bound, twins[i]["reader:stats"], f"the bound statistics of the sweep queued under {setter}")
            try:
                got = snap(dev)
            except G.SGPError as e:
                assert setter == "set_inducing" and "no finished sweep" in str(e), (setter, e)
            else:
                assert_bitwise(got, {k: twins[i][k] for k in ("mu", "Sigma", "Uv", "scalars")}, f"queued sweep under {setter}")
        sweep_on(dev, busy, t)
        last = snap(dev)
        assert_bitwise(last, {k: twins[-1][k] for k in ("mu", "Sigma", "Uv", "scalars")}, "the sweep after the last setter")
    worst = max(check_oracle(st, tw, f"{name}/{i}") for i, (st, tw) in enumerate(zip([s0] + [c[1] for c in chain], twins))
                if name == "ungated" or i in (0, len(chain)))
    show(f"(b) {name} setters under sweep(tstream)", bits, err_over_bound=worst)


# ---- (c) one handle alternating between its own and callers' streams ------------------------------------------------------------
@pytest.mark.parametrize("name", ["gated", "overlapped", "nojoin"])
def test_alternating_streams_on_one_handle(G, torch, cus, busy, streams, monkeypatch, name):
    t1, t2 = streams
    order = [None, t1, None, t2, t2, None]
    over = P.CASES[name]["overlapped"]
    twins = [twin(G, monkeypatch, cus, P.step(name, k), overlap=over and s is None) for k, s in enumerate(order)]
    worst = 0.0
    with make(G, monkeypatch, P.step(name, 0)) as dev:
        assert bool(dev.overlap_plan()) == over, "the case that is there for the overlapped order does not overlap on this device"
        for k, s in enumerate(order):
            st = P.step(name, k)
            P.set_kernel(dev, st)
            P.set_noise(dev, st)
            sweep_on(dev, busy, s)
            bits = dev.sweep_plan()
            got = snap(dev)
            assert bits == P.expected_bits(name, cus, stream=s is not None, overlapped=over), (k, bits)
            assert bits == twins[k]["bits"] or s is not None
            assert_bitwise(got, {q: twins[k][q] for q in ("mu", "Sigma", "Uv", "scalars")}, f"{name} sweep {k}")
            worst = max(worst, check_oracle(st, got, f"{name}/{k}"))
            show(f"(c) {name} sweep {k} on {'own' if s is None else 't1' if s is t1 else 't2'}", bits)
    print(f"(c) {name}: max error / bound {worst:.3g}")


# ---- (d) two-phase sweeps, the halves on the same and on different streams ------------------------------------------------------
PAIRS = {"t1_t1": (0, 0), "own_own": (None, None), "own_t1": (None, 0), "t1_own": (0, None), "t1_t2_event": (0, 1)}


@pytest.mark.parametrize("name,pair", [("gated", p) for p in PAIRS] + [("overlapped", "own_t1"), ("ungated", "own_t1"), ("multi", "t1_own")])
def test_two_phase_sweep_with_the_halves_on_any_streams(G, torch, cus, busy, streams, monkeypatch, name, pair):
    """sgp_sweep_local and sgp_sweep_finish may be given different streams (include/sgp_hip.h): the finish is ordered behind the
    local half by the library.  Bitwise the one-shot sweep alone."""
    old, new = P.step(name, 0), P.step(name, 1)
    alone = twin(G, monkeypatch, cus, new)
    sl, sf = (None if i is None else streams[i] for i in PAIRS[pair])
    with make(G, monkeypatch, old) as dev:
        dev.sweep()
        P.set_kernel(dev, new)
        P.set_noise(dev, new)
        if sl is not None:
            busy(sl)
        dev.sweep_local(0 if sl is None else sl.cuda_stream)
        bits = dev.sweep_plan()
        if pair == "t1_t2_event":
            ev = torch.cuda.Event()
            ev.record(sl)
            sf.wait_event(ev)
        elif sf is not None and sf is not sl:
            busy(sf)
        dev.sweep_finish(0 if sf is None else sf.cuda_stream)
        assert dev.sweep_plan() == bits                    # (recorded at plan time)
        got = snap(dev)
        assert bits == P.expected_bits(name, cus, stream=sl is not None, whole=False), bits
        assert_bitwise(got, {q: alone[q] for q in ("mu", "Sigma", "Uv", "scalars")}, f"two-phase {pair}")
        worst = check_oracle(new, got, f"{name}/{pair}")
        # ... and the next sweep, on the library's own stream, finds the handle in order
        nxt = P.step(name, 2)
        P.set_kernel(dev, nxt)
        P.set_noise(dev, nxt)
        dev.sweep()
        check_oracle(nxt, snap(dev), f"{name}/{pair} next")
        show(f"(d) {name} local {pair}", bits, err_over_bound=worst)


def test_two_phase_exact_psi_sweep_on_a_callers_stream(G, torch, busy, streams, monkeypatch):
    from oracle import sgp_oracle as O
    from tests import psi_stats_ref as R
    from tests.test_gpu_psi_sweep import JIT, S2, problem, setup
    M, D, T = 80, 2, 150
    Xu, ell, mean, S, Y, W = problem(1, M, D, T)
    t = streams[0]
    res = []
    assert live_handles() == 0
    for s in (None, t):
        with G.SGPDevice(T, M, D) as dev:
            setup(dev, Xu, ell, W)
            if s is not None:
                busy(s)
            dev.sweep_local_psi(mean, S, Y[:, 0], None, 0 if s is None else s.cuda_stream)
            bits = dev.sweep_plan()
            dev.sweep_finish(0 if s is None else s.cuda_stream)
            res.append(dict(snap(dev), **dict(zip(("Psi2", "B", "sc"), dev.stats()))))
            assert ("events" in bits) == (s is not None) and "gate_side" not in bits
    assert_bitwise(res[1], res[0], "sweep_local_psi(tstream) + sweep_finish(tstream)")
    uni, _ = R.exact_suff_stats(Xu, S2, ell, mean, S, Y)
    assert np.max(np.abs(res[1]["Psi2"] - uni.Psi2)) < 1e-13 * np.max(np.abs(uni.Psi2))
    Lam0 = np.eye(M) / 10.0
    ref = O.vmp_sweep(Xu, None, None, None, S2, ell, W[0, 0], jitter=JIT, Lambda0=Lam0, xi0=np.zeros(M), stats=uni)
    tol = P.post_tol(np.linalg.cond(Lam0 + W[0, 0] * uni.Psi2))
    errs = dict(mu=P.relF(res[1]["mu"], ref.mu_v), Sigma=P.relF(res[1]["Sigma"], ref.Sigma_v), Uv=P.relF(res[1]["Uv"], ref.Uv))
    assert all(v < tol for v in errs.values()), (errs, tol)
    show("(d) exact-Psi local + finish on tstream", bits, err_over_bound=max(errs.values()) / tol)


# ---- (e) sweeps over the resident statistics on a caller's stream ---------------------------------------------------------------
@pytest.mark.parametrize("full_on_stream", [False, True], ids=["full_own_resident_tstream", "full_tstream_resident_own"])
def test_resident_sweeps_across_streams(G, torch, cus, busy, streams, monkeypatch, full_on_stream):
    s0 = P.step("gated", 0)
    s1, s2 = s0._replace(targets=2), s0._replace(targets=2, noise=1)
    twins = [twin(G, monkeypatch, cus, st) for st in (s0, s1, s2)]
    t = streams[0]
    sfull, sres = (t, None) if full_on_stream else (None, t)
    with make(G, monkeypatch, s0, reuse=True, overlap=False) as dev:
        sweep_on(dev, busy, sfull)
        assert "resident" not in dev.sweep_plan()
        dev.set_targets(P.targets_of(s1))
        sweep_on(dev, busy, sres)
        b1, got1 = dev.sweep_plan(), snap(dev)
        assert dev.sweep_kind()[1] == 1                    # TARGETS
        P.set_noise(dev, s2)
        sweep_on(dev, busy, sres)
        b2, got2 = dev.sweep_plan(), snap(dev)
        assert dev.sweep_kind()[1] == 2                    # REUSED
    for b in (b1, b2):
        assert "resident" in b and ("events" in b) == (sres is not None) and not b & {"join_word", "kuu_interleaved", "overlapped"}
    assert_bitwise(got1, {q: twins[1][q] for q in got1}, "TARGETS sweep")
    assert_bitwise(got2, {q: twins[2][q] for q in got2}, "REUSED sweep")
    worst = max(check_oracle(s1, got1, "targets"), check_oracle(s2, got2, "reused"))
    show(f"(e) gated resident sweeps, full on {'tstream' if full_on_stream else 'own'}", b2, err_over_bound=worst)


# ---- (f) live handles -----------------------------------------------------------------------------------------------------------
def test_a_second_live_handle_turns_the_word_join_off_and_its_close_turns_it_on(G, torch, cus, monkeypatch):
    st = P.step("gated", 0)
    alone = twin(G, monkeypatch, cus, st)
    want = {q: alone[q] for q in ("mu", "Sigma", "Uv", "scalars")}
    assert "join_word" in alone["bits"] or cus < 248
    with make(G, monkeypatch, st) as a:
        idle = make(G, monkeypatch, P.step("ungated", 0))
        a.sweep()
        b2 = a.sweep_plan()
        assert b2 == P.expected_bits("gated", cus, live=2) and "join_word" not in b2
        assert_bitwise(snap(a), want, "a second handle alive")
        idle.close()
        a.sweep()
        assert a.sweep_plan() == alone["bits"]
        assert_bitwise(snap(a), want, "the second handle closed")
        for bad in (dict(n_max=10, m=4, d=40), dict(n_max=10, m=4, d=1, d_out=9), dict(n_max=0, m=4, d=1)):
            with pytest.raises(G.SGPError):
                G.SGPDevice(**bad)
        with pytest.raises(G.SGPError):
            G.SGPDevice(10, 4, 1, persistent_chain=True)   # (refused behind the device checks, still in front of the count)
        a.sweep()
        assert a.sweep_plan() == alone["bits"], "a failed sgp_create changed the live-handle count"
        assert_bitwise(snap(a), want, "after failed creates")
        show("(f) gated, idle second handle", b2)
        show("(f) gated, second handle closed / failed creates", a)


@pytest.mark.parametrize("name", ["ungated", "gated"])
@pytest.mark.parametrize("b_on_stream", [False, True], ids=["both_own", "b_on_tstream"])
def test_two_handles_with_sweeps_queued_at_the_same_time(G, torch, cus, busy, streams, monkeypatch, name, b_on_stream):
    sa, sb = P.step(name, 0), P.step(name, 1, variant=1)
    ta, tb = twin(G, monkeypatch, cus, sa), twin(G, monkeypatch, cus, sb)
    t = streams[0] if b_on_stream else None
    with make(G, monkeypatch, sa) as a, make(G, monkeypatch, sb) as b:
        for _ in range(2):
            a.sweep()
            sweep_on(b, busy, t)
        ba, bb = a.sweep_plan(), b.sweep_plan()
        ga, gb = snap(a), snap(b)
    assert ba == P.expected_bits(name, cus, live=2) and bb == P.expected_bits(name, cus, live=2, stream=b_on_stream)
    assert_bitwise(ga, {q: ta[q] for q in ga}, "handle a")
    assert_bitwise(gb, {q: tb[q] for q in gb}, "handle b")
    worst = max(check_oracle(sa, ga, f"{name}/a"), check_oracle(sb, gb, f"{name}/b"))
    show(f"(f) {name} a.sweep b.sweep a.sweep b.sweep, a", ba, err_over_bound=worst)
    show(f"(f) {name} ... b{' on tstream' if b_on_stream else ''}", bb)


# ---- (g) sgp_time_kernel on a caller's stream, then a sweep ---------------------------------------------------------------------
def test_time_kernel_on_a_callers_stream_then_a_sweep(G, torch, cus, streams, monkeypatch):
    from gaussianprocessnode_amd import _lib
    st = P.step("gated", 0)
    alone = twin(G, monkeypatch, cus, st)
    with make(G, monkeypatch, st, reuse=True) as dev:
        dev.sweep()
        for which in (_lib.SGP_T_GRAM, _lib.SGP_T_SYRK):
            assert dev.time_kernel(which, iters=2, stream=streams[0].cuda_stream) > 0.0
        assert dev.sweep_kind()[0] == 0                    # FULL: the timed launches rewrote K_uf and the partial sums
        dev.sweep()
        bits = dev.sweep_plan()
        assert dev.sweep_kind()[1] == 0 and "resident" not in bits
        got = snap(dev)
    assert_bitwise(got, {q: alone[q] for q in got}, "sweep after time_kernel(tstream)")
    show("(g) gated time_kernel(tstream) then sweep", bits, err_over_bound=check_oracle(st, got, "after time_kernel"))
