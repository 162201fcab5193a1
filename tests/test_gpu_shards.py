"""Data-sharded sweeps over UNEVEN shards, simulated in one process on one GPU: one handle per rank, each holding its
`shard_bounds` slice, with an all-reduce hook installed.  `shard_bounds` gives the first N mod world ranks one extra point, so
the ranks of one run hold different point counts -- and every rank must still issue the same sequence of collectives (the
overlapped order reduces once per statistics group, include/sgp_hip.h sgp_set_allreduce).  A plan mismatch fails an assert
here; nothing launches mismatched collectives across processes."""
import math

import numpy as np
import pytest

from gaussianprocessnode_amd.distributed import shard_bounds
from oracle import sgp_oracle as O
from tests.test_gpu_parity import post_tol, relF

pytestmark = pytest.mark.gpu

# What decides the collectives of an overlapped sweep: the groups' tile columns (and so the piece sizes), which stream runs them
# and which chain step forms them.  The point chunking of each group's SYRK ("chunks", "points_per_chunk") is the rank's own.
SHARED = ("col_begin", "col_end", "tiles", "masked", "cus", "form_step")


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def n_max_of(N, world):
    """The handle size every rank of a run uses: the largest shard, ceil(N / world)."""
    return -(-N // world)


def contract(plan):
    return [tuple(g[k] for k in SHARED) for g in plan]


def rank_plans(dev, X, world, hook_first=True):
    """overlap_plan() of every rank of `world`, each rank's shard of X loaded into the hooked handle `dev` in turn."""
    plans = []
    for r in range(world):
        lo, hi = shard_bounds(len(X), world, r)
        if not hook_first:
            dev.set_allreduce(None)
        dev.set_data(X[lo:hi], np.zeros(hi - lo))
        if not hook_first:
            dev.set_allreduce(lambda ptr, n, stream: None)
        plans.append(contract(dev.overlap_plan()))
    return plans


# (world, N, M): the cases a re-implementation of the planner flagged -- M = 512: 9793 / 9792 points, M = 256: 8193 / 8192 --
# and three ranks at the north-star size
PLAN_CASES = [(2, 19585, 512), (2, 16385, 256), (3, 20000, 512)]


@pytest.mark.parametrize("world,N,M", PLAN_CASES, ids=[f"w{w}-N{N}-M{M}" for w, N, M in PLAN_CASES])
def test_ranks_agree_on_the_overlap_plan(G, world, N, M):
    D = 2
    X = np.random.default_rng(N).uniform(-1.7, 1.7, (N, D))
    devs = [G.SGPDevice(n_max_of(N, world), M, D) for _ in range(world)]
    try:
        plans = []
        for r, dev in enumerate(devs):
            lo, hi = shard_bounds(N, world, r)
            dev.set_allreduce(lambda ptr, n, stream: None)
            dev.set_data(X[lo:hi], np.zeros(hi - lo))
            plans.append(contract(dev.overlap_plan()))
        assert all(p == plans[0] for p in plans), plans
        # the hook installed after the data: the same plan
        again = G.SGPDevice(n_max_of(N, world), M, D)
        with again:
            assert rank_plans(again, X, world, hook_first=False) == plans
    finally:
        for d in devs:
            d.close()


@pytest.mark.parametrize("world,N,M", PLAN_CASES, ids=[f"w{w}-N{N}-M{M}" for w, N, M in PLAN_CASES])
def test_ranks_agree_on_the_overlap_plan_across_a_scan_of_N(G, world, N, M):
    """200 consecutive totals around each case, every rank's handle sized by the rule (n_max = ceil(N / world)); one handle per
    n_max holds each rank's shard in turn."""
    D = 2
    X = np.random.default_rng(7).uniform(-1.7, 1.7, (N + 100, D))
    devs, bad = {}, []
    try:
        for n_tot in range(N - 100, N + 100):
            nm = n_max_of(n_tot, world)
            if nm not in devs:
                for d in devs.values():
                    d.close()
                devs = {nm: G.SGPDevice(nm, M, D)}
                devs[nm].set_allreduce(lambda ptr, n, stream: None)
            plans = rank_plans(devs[nm], X[:n_tot], world)
            if any(p != plans[0] for p in plans):
                bad.append((n_tot, plans))
    finally:
        for d in devs.values():
            d.close()
    assert not bad, f"{len(bad)} totals with rank-dependent plans, first: {bad[0]}"


@pytest.mark.parametrize("n_max", [1, 6667], ids=["sized-for-N", "sized-for-a-larger-run"])
def test_ranks_agree_on_the_overlap_plan_with_an_empty_shard(G, n_max):
    """Three ranks, two points: one shard is empty.  Handles sized for this N, and handles sized for a larger run (a host-paced
    run's last, small minibatch), where the plan is the overlapped one and the empty rank must follow it too."""
    world, N, M, D = 3, 2, 512, 2
    X = np.random.default_rng(3).uniform(-1.7, 1.7, (N, D))
    with G.SGPDevice(n_max, M, D) as dev:
        dev.set_allreduce(lambda ptr, n, stream: None)
        plans = rank_plans(dev, X, world)
    assert [shard_bounds(N, world, r)[1] - shard_bounds(N, world, r)[0] for r in range(world)] == [1, 1, 0]
    assert all(p == plans[0] for p in plans), plans


def _sharded_run(G, world, N, M, D, n_max, w=200.0, seed=41):
    """One sharded sweep and theta objective, simulated (tests/sharded_ref.py, `simulate`): pass 1 captures every rank's pieces (local
    statistics), pass 2 sweeps every rank with a hook that adds the other ranks' pieces -- what a sum-all-reduce leaves in the
    buffer -- so that every rank holds the whole posterior; then the 33-double gradient payloads the same way.  Returns the ranks'
    hook call sizes and rank 0's results."""
    pytest.importorskip("torch")
    from tests.sharded_ref import simulate
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.745, 1.745, (N, D))
    Xu = (X if N >= M else rng.uniform(-1.745, 1.745, (M, D)))[:M].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    s2, ell = 0.9, np.linspace(1.5, 3.0, D)
    plans = [None] * world

    def make(r):
        lo, hi = shard_bounds(N, world, r)
        d = G.SGPDevice(n_max, M, D)
        d.set_inducing(Xu); d.set_data(X[lo:hi], y[lo:hi]); d.set_kernel(s2, ell, 0.0)
        d.set_prior_isotropic(50.0); d.set_noise([[w]])
        return d

    def apply(r, d, op, second):
        if op == "sweep":
            d.sweep()
            if not second:
                plans[r] = contract(d.overlap_plan())
            return dict(post=d.posterior(), stats=d.stats(), scalars=d.scalars()) if second else None
        val, grad = d.theta_objective(want_grad=True)
        return dict(val=val, grad=grad)

    swept, objective = simulate(world, make, ["sweep", "objective"], apply)
    first = swept["results"][0]
    out = dict(plans=plans, calls1=swept["captured"], calls2=swept["calls"], gcalls=objective["calls"],
               posts=[r["post"] for r in swept["results"]], val=objective["results"][0]["val"],
               grad=objective["results"][0]["grad"], stats=first["stats"], scalars=first["scalars"])
    return out, (X, Xu, y, s2, ell, w)


# (world, N, M, n_max): the two uneven cases of the plan contract at the north-star M, and an empty rank in the overlapped order
SWEEP_CASES = [(2, 19585, 512, None), (3, 20000, 512, None), (3, 2, 512, 6667)]


@pytest.mark.parametrize("world,N,M,n_max", SWEEP_CASES, ids=["w2-N19585", "w3-N20000", "w3-N2-empty-rank"])
def test_uneven_shards_sweep_to_the_whole_data_posterior(G, world, N, M, n_max):
    D = 8
    n_max = n_max or n_max_of(N, world)
    r, (X, Xu, y, s2, ell, w) = _sharded_run(G, world, N, M, D, n_max)
    # every rank: the same plan and the same sequence of collectives, sweep after sweep
    assert all(p == r["plans"][0] for p in r["plans"]), r["plans"]
    assert all(c == r["calls1"][0] for c in r["calls1"]), r["calls1"]
    assert r["calls2"] == r["calls1"], (r["calls1"], r["calls2"])
    assert all(c == [33] for c in r["gcalls"]), r["gcalls"]
    assert len(r["calls1"][0]) == max(1, len(r["plans"][0]))
    if n_max > 1000:
        assert len(r["plans"][0]) == 2, r["plans"][0]          # these sizes run the overlapped order: one collective per group
    ref = O.vmp_sweep(Xu, X, y, None, s2, ell, w, jitter=0.0, Lambda0=np.eye(M) / 50.0, xi0=np.zeros(M))
    Psi2, B, scal = r["stats"]
    assert relF(Psi2, ref.stats.Psi2) < 1e-13 and np.array_equal(Psi2, Psi2.T)
    assert relF(B, np.reshape(ref.stats.b, B.shape)) < 1e-13
    assert scal[2] == N and scal[1] == N and math.isclose(scal[0], ref.stats.s_yy[0, 0], rel_tol=1e-13)
    cond_L = np.linalg.cond(np.eye(M) / 50.0 + w * ref.stats.Psi2)
    tol = post_tol(cond_L)
    for mu, Sig, Uv in r["posts"]:                             # every rank holds the whole-data posterior
        assert relF(mu, ref.mu_v) < tol and relF(Sig, ref.Sigma_v) < tol and relF(Uv, ref.Uv) < tol
    sc = r["scalars"]
    Kuu = O.kernelmatrix(s2, ell, Xu)
    tol_I1 = 50 * np.finfo(float).eps * np.linalg.cond(Kuu) * ref.stats.s_kk + 1e-12
    assert abs(sc.sum_I1 - ref.sum_I1) <= tol_I1
    assert abs(sc.energy - ref.energy) <= max(1e-7, tol) * abs(ref.energy) + 0.5 * w * tol_I1
    # the gradient: the ranks' 33-double data halves summed through the hook, against central differences of the oracle's
    # objective over the whole data at rank 0's q(v)
    mu0, _, Uv0 = r["posts"][0]
    p0 = np.concatenate([[s2], ell])
    f = lambda p: O.theta_objective(Xu, X, y, p[0], p[1:], mu0, Uv0, w)
    g_ref = np.array([(f(p0 + 1e-6 * e) - f(p0 - 1e-6 * e)) / 2e-6 for e in np.eye(1 + D)])
    assert math.isclose(r["val"], f(p0), rel_tol=1e-8, abs_tol=0.5 * w * tol_I1), (r["val"], f(p0))
    np.testing.assert_allclose(r["grad"], g_ref, rtol=5e-5, atol=1e-6 * np.abs(g_ref).max())
