"""The cases of tests/test_gpu_sweep_plans.py: one problem on each side of every threshold from which sweep_plan and sweep_local_impl
(csrc/sgp_api.hip) choose how a sweep's launches meet, and the parameter sets its consecutive sweeps run at (helper, no tests;
imported by the GPU suite and by tests/test_sweep_plans_host.py, which holds the table to the constants of the source).

The plan follows from three facts.  The stream: a caller's stream turns the hand-off into events and rules out the overlapped order
and the interleaved K_uu chain.  The live handles of the process: a second one turns the Sigma launch's word join into an event
wait.  The size: gate_side (points x lower tiles >= GATE_MIN), the word join's grid bound (TQ (TQ + 1) / 2 * 4 + TQ^2 <= CUs -
JOIN_RESERVED_CUS) and the overlap planner.  Shapes are the smallest on each side of each threshold on a 256-CU device; the GPU tests
assert the bits the library reports (SGPDevice.sweep_plan), so nothing here is taken on trust.

Consecutive sweeps of a sequence run at consecutive rows of STEPS (kernel amplitude, lengthscales and noise precision all move), so
that a reader that saw the previous sweep's results misses every tolerance by orders of magnitude (MIN_STEP_DIFFERENCE).
"""
import collections
import functools
import zlib

import numpy as np

from oracle import sgp_oracle as O

TILE = 64
GATE_MIN = 10000                   # points x lower tiles from which the SYRK is taken to fill the chip (set_point_count)
JOIN_RESERVED_CUS = 40             # CUs the Sigma launch must leave free for a late K_uu chain before it may poll the join word
REFERENCE_CUS = 256                # the device the shapes were chosen for (MI355X)
PRIOR_VAR = 50.0
MIN_STEP_DIFFERENCE = 1e-3         # relative Frobenius distance between the oracle posteriors of consecutive STEPS, at least
COND_KUU_MAX, COND_LAMBDA_MAX = 1e10, 1e9

# name -> shape.  `expect`: the size-dependent bits on REFERENCE_CUS compute units for a whole sweep on the library's own stream with
# one live handle (the GPU test recomputes them from the device's CU count); `overlapped` is the planner's choice and is read from
# overlap_plan() there.
CASES = {
    "ungated": dict(N=1500, M=48, D=2, ell=(0.5, 0.4), jitter=1e-8, w=40.0, gate_side=False, join_word=True, overlapped=False),
    "gated": dict(N=5000, M=512, D=8, ell=tuple(np.linspace(1.5, 3.0, 8)), jitter=1e-8, w=100.0, gate_side=True, join_word=True,
                  overlapped=False),
    "nojoin": dict(N=3000, M=576, D=3, ell=(0.45, 0.4, 0.35), jitter=1e-6, w=60.0, gate_side=True, join_word=False,
                   overlapped=False),
    "overlapped": dict(N=10000, M=512, D=8, ell=tuple(np.linspace(1.5, 3.0, 8)), jitter=1e-8, w=100.0, gate_side=True,
                       join_word=True, overlapped=True),
    # d_out = 2: 300 nodes of five weighted points each (the layout of a cubature rule); MultiSGP sweeps never take the word join
    "multi": dict(N=1500, M=48, D=2, d_out=2, nodes=300, ell=(0.5, 0.4), jitter=1e-8, gate_side=False, join_word=False,
                  overlapped=False),
}
# (sigma2, factor on every lengthscale, factor on the noise precision) of the k-th sweep of a sequence
STEPS = ((0.9, 1.0, 1.0), (1.1, 0.93, 1.6), (0.75, 1.04, 0.6), (1.0, 0.9, 2.2), (0.85, 0.97, 0.8), (1.2, 0.88, 1.3))


def geometry(N, M, d_out=1, cus=REFERENCE_CUS):
    """What the plan's size-dependent bits follow from, restated from set_point_count and sweep_local_impl: (lower tiles, points x
    lower tiles, the Sigma launch's grid, gate_side, whether the grid bound allows the word join)."""
    T, TQ = -(-M // TILE), -(-(M * d_out) // TILE)
    ntiles = T * (T + 1) // 2
    grid = TQ * (TQ + 1) // 2 * 4 + TQ * TQ
    return dict(T=T, TQ=TQ, ntiles=ntiles, work=N * ntiles, grid=grid, gate_side=N * ntiles >= GATE_MIN,
                join_fits=grid <= cus - JOIN_RESERVED_CUS)


def expected_bits(name, cus, *, stream=False, live=1, whole=True, overlapped=None, hook=False):
    """The set of plan bits (names of gaussianprocessnode_amd._lib.PLAN_BITS) a FULL sweep of case `name` must report on `cus`
    compute units: `stream`: on a caller's stream; `live`: handles alive in the process; `whole`: sgp_sweep (not sgp_sweep_local);
    `overlapped`: what overlap_plan() said for the handle (None: the table's entry)."""
    c = CASES[name]
    g = geometry(c["N"], c["M"], c.get("d_out", 1), cus)
    events = stream or hook
    over = (c["overlapped"] if overlapped is None else overlapped) and whole and not stream
    stats_first = g["gate_side"] and not hook
    bits = set()
    if over: bits.add("overlapped")
    if events: bits.add("events")
    if c.get("d_out", 1) == 1 and not events and g["join_fits"] and live <= 1: bits.add("join_word")
    if whole and stats_first and not events: bits.add("kuu_interleaved")
    if stats_first: bits.add("stats_first")
    if g["gate_side"]: bits.add("gate_side")
    return frozenset(bits)


@functools.lru_cache(maxsize=None)
def inputs(name, variant=0):
    """The case's inputs (arrays not to be written to).  `variant`: another draw of the same shape (a second handle's data).  Y2: other
    targets for the same inputs (set_targets)."""
    c = CASES[name]
    N, M, D, Do = c["N"], c["M"], c["D"], c.get("d_out", 1)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{variant}".encode()))
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    y2 = np.cos(X[:, 0] - X[:, -1]) + 0.1 * rng.normal(size=N)
    y2 = (y2 - y2.mean()) / y2.std()
    d = dict(name=name, N=N, M=M, D=D, Do=Do, X=X, Xu=Xu, Y=y, Y2=y2, wts=None, ell=np.array(c["ell"]), jitter=c["jitter"])
    if Do > 1:
        T = c["nodes"]
        S = N // T
        wts = rng.uniform(0.5, 1.5, (T, S))
        A = rng.normal(size=(Do, Do))
        d.update(T=T, S=S, wts=(wts / wts.sum(axis=1, keepdims=True)).reshape(-1),
                 Ynode=np.stack([y[::S], np.cos(X[::S, 0])], axis=1),
                 Ynode2=np.stack([y2[::S], np.sin(X[::S, 1])], axis=1),
                 Sig_y=np.stack([np.diag(rng.uniform(0.01, 0.1, Do)) for _ in range(T)]),
                 W=A @ A.T + Do * np.eye(Do), xi0=0.01 * rng.normal(size=Do * M))
    return d


# What a handle is configured with: the case, the rows of STEPS its kernel and its noise come from, the prior ("iso": isotropic
# PRIOR_VAR; "iso5": isotropic 5; "dense": a dense precision and a non-zero weighted mean; d_out > 1 always has its own dense prior),
# which targets (1 | 2), which inducing inputs (0: the case's; 1: those of another draw) and which draw of the data.
State = collections.namedtuple("State", "name kern noise prior targets xu variant", defaults=(0, 0, "iso", 1, 0, 0))


def step(name, k, **kw):
    """the state of the k-th sweep of a sequence: kernel and noise both from STEPS[k]"""
    return State(name, k % len(STEPS), k % len(STEPS), **kw)


def kernel_of(st):
    return STEPS[st.kern][0], inputs(st.name)["ell"] * STEPS[st.kern][1]


def noise_of(st):
    d = inputs(st.name)
    return CASES[st.name]["w"] * STEPS[st.noise][2] if d["Do"] == 1 else d["W"] * STEPS[st.noise][2]


def inducing_of(st):
    return inputs(st.name, st.variant if st.xu == 0 else 7)["Xu"]


@functools.lru_cache(maxsize=None)
def prior_of(st):
    """(xi0, Lambda0) of the state's prior, natural form"""
    d = inputs(st.name, st.variant)
    Q = d["Do"] * d["M"]
    if d["Do"] > 1:
        return d["xi0"], np.eye(Q) / 10.0
    if st.prior == "dense":
        rng = np.random.default_rng(Q)
        A = rng.normal(size=(Q, 8))
        return 0.05 * rng.normal(size=Q), np.eye(Q) / PRIOR_VAR + 0.02 * A @ A.T
    return np.zeros(Q), np.eye(Q) / (5.0 if st.prior == "iso5" else PRIOR_VAR)


def set_kernel(dev, st):
    s2, ell = kernel_of(st)
    dev.set_kernel(s2, ell, inputs(st.name)["jitter"])


def set_noise(dev, st):
    w = noise_of(st)
    dev.set_noise([[w]] if np.ndim(w) == 0 else w)


def set_prior(dev, st):
    xi0, L0 = prior_of(st)
    if inputs(st.name)["Do"] == 1 and st.prior != "dense":
        dev.set_prior_isotropic(1.0 / L0[0, 0])
    else:
        dev.set_prior_precision(xi0, L0)


def targets_of(st):
    d = inputs(st.name, st.variant)
    if d["Do"] == 1:
        return d["Y"] if st.targets == 1 else d["Y2"]
    return np.repeat(d["Ynode"] if st.targets == 1 else d["Ynode2"], d["S"], axis=0)


def configure(dev, st):
    """Everything a new handle needs to sweep at `st` (the setters upload; nothing is enqueued)."""
    d = inputs(st.name, st.variant)
    dev.set_inducing(inducing_of(st))
    if d["Do"] == 1:
        dev.set_data(d["X"], targets_of(st))
    else:
        dev.set_data(d["X"], targets_of(st), None, d["wts"], n_nodes=d["T"])
        dev.set_output_cov_sum(d["Sig_y"].sum(axis=0))
    set_prior(dev, st)
    set_kernel(dev, st)
    set_noise(dev, st)


@functools.lru_cache(maxsize=None)
def oracle(st, carried=0):
    """The CPU oracle's sweep at `st`: dict(mu, Sigma, cond_kuu, cond_lambda) and, d_out = 1, Uv, energy, sum_I1, sum_I2, KuuL, Psi2, B,
    w, tol_I1.  `carried`: the sweep follows that many sweep + carry_posterior pairs at the same state (the prior has taken the
    statistics in that often).  Computed once per state and shared; not to be written to."""
    d = inputs(st.name, st.variant)
    (s2, ell), noise, Xu, M = kernel_of(st), noise_of(st), inducing_of(st), d["M"]
    xi0, L0 = prior_of(st)
    Kuu = O.kernelmatrix(s2, ell, Xu) + d["jitter"] * np.eye(M)
    out = dict(cond_kuu=float(np.linalg.cond(Kuu)))
    if d["Do"] == 1:
        st_ = O.suff_stats(Xu, d["X"], targets_of(st), None, s2, ell)
        L0, xi0 = L0 + carried * noise * st_.Psi2, xi0 + carried * noise * st_.b[:, 0]
        ref = O.vmp_sweep(Xu, d["X"], targets_of(st), None, s2, ell, noise, jitter=d["jitter"], Lambda0=L0, xi0=xi0, stats=st_)
        out.update(mu=ref.mu_v, Sigma=ref.Sigma_v, Uv=ref.Uv, energy=ref.energy, sum_I1=ref.sum_I1, sum_I2=ref.sum_I2, w=noise,
                   KuuL=ref.KuuL, Psi2=st_.Psi2, B=st_.b, cond_lambda=float(np.linalg.cond(L0 + noise * st_.Psi2)))
        # sum I1 = s_kk - tr(Kuu^-1 Psi2) cancels: cond(K_uu) eps s_kk (tests/test_gpu_parity.py, tests/test_gpu_early_formation.py)
        out["tol_I1"] = 50 * np.finfo(float).eps * out["cond_kuu"] * st_.s_kk
    else:
        T, S = d["T"], d["S"]
        Yn = d["Ynode"] if st.targets == 1 else d["Ynode2"]
        ms = O.multi_suff_stats(Xu, d["X"].reshape(T, S, d["D"]), d["wts"].reshape(T, S), Yn, d["Sig_y"], s2, ell)
        L0, xi0 = L0 + carried * np.kron(noise, ms.Psi2), xi0 + carried * (ms.B @ noise).T.reshape(-1)
        mu, Sig = O.multi_v_update(ms, noise, L0, xi0)
        Kinv = O.cholinv(Kuu)
        out.update(mu=mu, Sigma=Sig, cond_lambda=float(np.linalg.cond(L0 + np.kron(noise, ms.Psi2))),
                   wishart=O.multi_w_update(ms, mu, Sig, Kinv), tol_I1=50 * np.finfo(float).eps * out["cond_kuu"] * ms.s_kk)
    return out


def post_tol(cond_L):
    """tests/test_gpu_parity.py's bound on the posterior: the north star's 1e-5, or cond(Lambda) * eps where that is tighter."""
    return min(1e-5, max(1e-9, 20 * np.finfo(float).eps * cond_L))


def relF(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
