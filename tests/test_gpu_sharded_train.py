"""Data-sharded device-paced training (sgp_train_step with an all-reduce hook installed) on two or three simulated ranks with
uneven and empty slices, against the whole-minibatch reference of tests/train_step_ref.py, through the comparison and at the
tolerances of the single-rank suite (train_step_ref.compare_outputs; nothing is widened: a sharded sum differs from the single-rank
one in its order alone).  The ranks are one handle each behind distributed.ShardedDevice; the sum-all-reduce is the replay of
tests/sharded_train_ref.py (every pass starts the run again, sums the collectives below its frontier and records the next group's
true local pieces: steps + learning steps + 1 passes).  tests/test_sharded_train_host.py shows on the CPU that the same driver over
NumPy ranks reproduces the reference and that a Gamma shape counting the local slice, an unsummed gradient payload, a dropped slot
beyond D = 3, a skipped collective on an empty rank and a local s_yy are each seen.

case                world  steps  what its shards reach
m12_d1_iso_m32      3      5      85/85/85, 86/85/85, 21 each, 29 each, then a window of 1 point: two EMPTY ranks on a step without
                                  learning; reset_prior on a later step; Matern-3/2
m65_d32_ard_se      2      3      all 33 gradient slots (D = 32, ARD); third window 1 point with reset_prior and learning: rank 1 is
                                  EMPTY on a learning step; 2 tile rows
m65_d5_iso_m12      2      2      129/128 and 37/36; Matern-1/2, one lengthscale: summed over the dimensions after the reduce
w1000_m130_d3_se    3      2      SGP_OVERLAP=1, 3 tile rows, 334/333/333 and 86/85/85 (see its test for what the library plans)
g1                  2      2      Probit, 129/128 and 71/71: q(w)'s shape and rate from the reduced statistics
g1e-4               3      3      Probit, vz = 1e4 on the first step, 67/67/66; last step without learning
mixed               3      2      Probit, mean / covariance prior; 7 points at x = FAR in 3/2/2, then 257 with both tails of r
g1_empty            3      2      Probit, first window 2 points in 1/1/0: an EMPTY rank on a learning Probit step (no forward
                                  message launch, k_probit_window with n = 0, no data half), then 67/67/66; run twice, bitwise

Every test prints its RATIO lines, every rank's slice length per step and the pass count (profiles/sharded_train.txt)."""
import numpy as np
import pytest

from tests import sharded_ref as SR
from tests import sharded_train_ref as ST
from tests import train_step_ref as TS
from tests.test_gpu_parity import relF
from tests.test_gpu_train_step import device_run

pytestmark = pytest.mark.gpu

# name -> (world, steps; None: the whole schedule)
CASES = {
    "m12_d1_iso_m32": (3, None),
    "m65_d32_ard_se": (2, 3),
    "m65_d5_iso_m12": (2, 2),
    "g1": (2, None),
    "g1e-4": (3, None),
    "mixed": (3, None),
    "g1_empty": (3, None),
}
EMPTY = ("g1_empty", "m12_d1_iso_m32", "m65_d32_ard_se")          # some rank holds no point of some step's window


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def check_run(name, world, nsteps, run, stats_counts=None):
    """Everything asserted of one replayed run (module docstring; the bounds are train_step_ref's and sharded_ref.STAT_TOL)."""
    case = ST.truncated(TS.get_case(name), nsteps)
    sched = case["sched"]
    M = case["Xu"].shape[0]
    res = run["results"]
    # the shards the case is there for, and the passes
    want_slices = ST.slices_of(sched, world)
    print(f"SLICES {name} world {world} n_max {run['n_max']}: " + " | ".join("/".join(str(v) for v in s) for s in want_slices)
          + f"; passes {run['passes']}")
    for r in range(world):
        assert run["slices"][r] == [s[r] for s in want_slices], r
    assert run["passes"] == len(sched) + sum(1 for s in sched if s[2]) + 1
    if name in EMPTY:
        assert any(0 in s for s in want_slices)
    # the documented collectives, per step, on every rank -- the empty ones included
    want = ST.step_counts(sched, SR.plain_counts(M) if stats_counts is None else stats_counts)
    for r in range(world):
        assert ST.split_steps(run["calls"][r], want) == want, (r, run["calls"][r])
    # every rank against the whole-minibatch reference
    for r, got in enumerate(res):
        ratios = TS.compare_outputs(name, got, nsteps)
        print(f"RATIO {name} world {world} rank {r}: " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()))
        assert all(v < 1.0 for v in ratios.values()), (r, ratios)
    # everything behind a collective is replicated arithmetic on identical bits: the ranks agree bitwise
    for r, got in enumerate(res[1:], 1):
        for k in ("theta", "steps", "skipped", "gamma", "mu", "Sigma"):
            assert ST.same_bits(got.get(k), res[0].get(k)), (r, k)
    # the last step's summed statistics piece: S_N is the whole window's length; Psi2 and B are the whole window's at the
    # reference's theta of that step, to the summation bound plus what the reference's theta tolerance lets them move by
    Psi2_ref, B_ref, n, allow_P, allow_B = ST.last_window_stats(name, nsteps)
    first = len(run["calls"][0]) - len(want[-1])
    if stats_counts is None:                                   # (one piece holds the whole buffer; grouped pieces are only counted)
        Psi2, B, sc = SR.unpack_exchange(run["summed"][0][first], M)
        tol_P, tol_B = SR.STAT_TOL + allow_P, SR.STAT_TOL + allow_B
        eP, eB = relF(Psi2, Psi2_ref), relF(B[:, 0], B_ref)
        print(f"RATIO {name} world {world} last window's summed statistics: S_N {sc[2]:g} of {n}, Psi2 {eP / tol_P:.3g} "
              f"(relF {eP:.3g}, bound {tol_P:.3g}), B {eB / tol_B:.3g} (relF {eB:.3g}, bound {tol_B:.3g})")
        assert sc[2] == n == sched[-1][1]
        assert eP < tol_P and eB < tol_B
    for r in range(1, world):                                  # the same sums on every rank
        assert all(np.array_equal(a, b) for a, b in zip(run["summed"][r], run["summed"][0])), r
    return res


@pytest.mark.parametrize("name", [n for n in CASES if n != "g1_empty"])
def test_sharded_runs_match_the_whole_minibatch_reference(G, name):
    world, nsteps = CASES[name]
    run = ST.device_replay(G, device_run, name, world, nsteps, overlap=0)
    assert all(p == [] for plans in run["plans"] for p in plans)
    check_run(name, world, nsteps, run)


def test_an_empty_rank_on_a_learning_probit_step_and_the_run_again(G):
    """g1_empty on three ranks: rank 2 holds no point of the first window and goes through the same collectives as its peers; the
    run a second time (new handles) is bitwise the first in every output of every rank."""
    world, nsteps = CASES["g1_empty"]
    a = ST.device_replay(G, device_run, "g1_empty", world, nsteps, overlap=0)
    res = check_run("g1_empty", world, nsteps, a)
    assert a["slices"][2][0] == 0 and a["calls"][2] == a["calls"][0]
    b = ST.device_replay(G, device_run, "g1_empty", world, nsteps, overlap=0)
    for r in range(world):
        assert set(res[r]) == set(b["results"][r])
        for k in res[r]:
            assert ST.same_bits(res[r][k], b["results"][r][k]), (r, k)
        assert all(np.array_equal(x, y) for x, y in zip(a["summed"][r], b["summed"][r]))


def test_overlap_forced_training_steps_keep_the_plain_order(G):
    """w1000_m130_d3_se (3 tile rows, 334/333/333 then 86/85/85) on handles created under SGP_OVERLAP=1.  With the hook installed
    and n_max = 334 the idle handle plans a grouped sweep (overlap_plan() is non-empty: two groups, the same on every rank), but a
    training step's sweep is never grouped: inside the run overlap_plan() is [] on every rank and step -- the library plans the
    plain order for sgp_train_step (sweep_plan and plan_overlap both leave a run out) -- so every step's statistics travel as
    ONE piece, sharded_ref.plain_counts, and that is what is asserted.  The planner is left as it is.  What the hooked run does
    exercise here: the events between the streams (the evDone record that ends a step and the K_uu chain's wait for it)."""
    name, world, nsteps = "w1000_m130_d3_se", 3, 2
    run = ST.device_replay(G, device_run, name, world, nsteps, overlap=1)
    idle, inside = run["plans_idle"], run["plans"]
    print(f"PLAN {name} n_max {run['n_max']}: idle handle {idle[0]}; inside the run {inside[0]}")
    assert all(p == idle[0] for p in idle)
    assert all(plans == inside[0] for plans in inside)
    M = TS.get_case(name)["Xu"].shape[0]
    if any(inside[0]):
        assert all(p == inside[0][0] for p in inside[0])
        check_run(name, world, nsteps, run, stats_counts=SR.planned_counts(inside[0][0], M))
    else:
        check_run(name, world, nsteps, run)
