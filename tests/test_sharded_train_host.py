"""The replay all-reduce of tests/sharded_train_ref.py on the CPU, no GPU: driven with a NumPy rank in place of SGPDevice it
reproduces train_step_ref's whole-minibatch run for one, two and three ranks; each listed fault of a rank drives an output of the
comparison tests/test_gpu_sharded_train.py asserts (train_step_ref.compare_outputs) to >= 1e3 tolerances or is caught by one of the
driver's own asserts; and the pass count and the frontier's advances are what the schedule says."""
import math

import numpy as np
import pytest

from tests import sharded_ref as SR
from tests import sharded_train_ref as ST
from tests import train_step_ref as TS


def worst(ratios):
    k = max(ratios, key=ratios.get)
    return k, float(ratios[k])


def compared(name, world, nsteps=None, **fault):
    """compare_outputs of every rank of a replayed NumPy run, and the Replay."""
    results, rp = ST.host_replay(name, world, nsteps, **fault)
    return [TS.compare_outputs(name, got, nsteps) for got in results], results, rp


# ------------------------------------------------------------------------------------------------
# 1. the replayed run is the whole-minibatch run

# (m12_d1_iso_m32: a later reset_prior and a last window of 1 point without learning, two empty ranks of three; m65_d5_iso_m12: one
# lengthscale over five dimensions, folded after the reduce; g1_empty: Probit with an empty rank on a learning step)
CLEAN = [("m12_d1_iso_m32", None), ("m65_d5_iso_m12", 2), ("g1_empty", None)]


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name,nsteps", CLEAN)
def test_replayed_numpy_ranks_reproduce_the_whole_minibatch_run(name, nsteps, world):
    ratios, results, rp = compared(name, world, nsteps)
    sched = ST.truncated(TS.get_case(name), nsteps)["sched"]
    for r, rat in enumerate(ratios):
        print(f"RATIO host {name} world {world} rank {r}: " + ", ".join(f"{q} {v:.3g}" for q, v in rat.items()))
        assert all(v < 1.0 for v in rat.values()), (r, rat)
    # every rank ends with the same bits: everything behind a collective is replicated arithmetic
    for got in results[1:]:
        for k in ("theta", "mu", "Sigma", "gamma", "steps", "skipped"):
            assert ST.same_bits(got[k], results[0][k]), k
    M = TS.get_case(name)["Xu"].shape[0]
    want = ST.step_counts(sched, SR.plain_counts(M))
    for r in range(world):
        assert ST.split_steps(rp.calls[r], want) == want
    assert rp.passes == len(sched) + sum(1 for s in sched if s[2]) + 1
    # the last step's summed statistics piece counts the whole window
    last = len(rp.counts) - len(want[-1])
    _, _, sc = SR.unpack_exchange(rp.summed_numpy()[0][last], M)
    assert sc[2] == sched[-1][1]
    if world == 3 and name != "m65_d5_iso_m12":
        assert any(0 in s for s in ST.slices_of(sched, world))              # an empty rank went through the same collectives


# ------------------------------------------------------------------------------------------------
# 2. the cases see a faulty rank

# fault -> (case, world, steps, which ranks carry it)
FAULT_CASE = {
    "gamma_counts_local_slice": ("g1", 2, None, None),
    "grad_payload_unsummed": ("m12_d1_iso_m32", 3, None, None),
    "grad_slot_dropped": ("m65_d32_ard_se", 2, 3, None),                    # slot 32, the last of D = 32
    "syy_from_local_slice": ("g1", 2, None, None),
}


@pytest.mark.parametrize("fault", sorted(FAULT_CASE))
def test_gpu_cases_see_a_faulty_rank(fault):
    """Each mutation of the NumPy rank moves a compared output of its GPU case by >= 1e3 x that output's tolerance on some rank (an
    exactly compared one: by anything at all)."""
    name, world, nsteps, who = FAULT_CASE[fault]
    ratios, _, _ = compared(name, world, nsteps, fault=fault, slot=32, faulty_ranks=who)
    top = max((worst(rat) for rat in ratios), key=lambda kv: kv[1])
    print(f"fault {fault}: case {name} on {world} ranks, {top[0]} moves by {top[1]:.3g} x its tolerance")
    assert top[1] >= 1e3, ratios
    assert set(FAULT_CASE) | {"empty_rank_skips_grad"} == set(ST.RANK_FAULTS)


@pytest.mark.parametrize("name,world,nsteps", [("g1_empty", 3, None), ("m65_d32_ard_se", 2, 3), ("m12_d1_iso_m32", 3, None)])
def test_a_rank_that_skips_its_gradient_collective_is_caught_by_the_driver(name, world, nsteps):
    """An empty rank that leaves out the gradient's collective (a deadlock on real hardware) issues another sequence of counts
    than its peers: the driver's assert, in the first pass.  m12_d1_iso_m32's empty slices fall on a step without learning, where
    there is no gradient collective to skip: that run stays clean."""
    sched = ST.truncated(TS.get_case(name), nsteps)["sched"]
    hit = any(learn and 0 in s for s, (_, _, learn, _) in zip(ST.slices_of(sched, world), sched))
    assert hit == (name != "m12_d1_iso_m32")
    if hit:
        with pytest.raises(AssertionError, match="issued|doubles where"):
            ST.host_replay(name, world, nsteps, fault="empty_rank_skips_grad")
    else:
        ratios, _, _ = compared(name, world, nsteps, fault="empty_rank_skips_grad")
        assert all(v < 1.0 for rat in ratios for v in rat.values())


# ------------------------------------------------------------------------------------------------
# 3. the driver itself: passes, frontiers, and replay against a lock-step all-reduce

class ToyRank:
    """A rank whose every piece depends on every earlier sum: per step a sweep of `pieces` collectives (their contents depend on
    the state, not on each other), then -- learning steps -- one collective whose content depends on that sweep's sums."""

    def __init__(self, r, pieces, jitter=None):
        self.r, self.pieces, self.hook, self.jitter = r, pieces, None, jitter
        self.begin()

    def begin(self):
        self.x = 1.0 + 0.25 * self.r

    def step(self, k, learn, reduce):
        bufs = [np.array([math.sin(self.x + k + j), self.x * (j + 1), float(self.r == j)]) for j in range(self.pieces)]
        if self.jitter is not None:
            bufs[0][0] += next(self.jitter)
        for b in bufs:
            reduce(self.r, b)
        s = sum(float(np.sum(b)) for b in bufs)
        self.x = math.cos(self.x) + 0.1 * s
        if learn:
            g = np.array([self.x * s + self.r, 1.0])
            reduce(self.r, g)
            self.x -= 0.01 * g[0] / g[1]


SCHED = [(0, 5, True, True), (5, 4, False, False), (0, 7, True, False), (9, 1, False, False), (2, 3, True, False)]


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("world", [1, 3])
def test_replay_is_a_lockstep_allreduce_and_its_passes_are_the_schedules(world, pieces):
    groups = ST.groups_of(SCHED, pieces)
    assert groups == [g for _, _, learn, _ in SCHED for g in ([pieces, 1] if learn else [pieces])]
    assert len(groups) == 5 + 3 and sum(groups) == 5 * pieces + 3
    assert ST.step_counts(SCHED, [7] * pieces) == [[7] * pieces + ([33] if s[2] else []) for s in SCHED]
    # lock step: all ranks advance together, every collective summed on the spot
    ranks = [ToyRank(r, pieces) for r in range(world)]
    for k, (_, _, learn, _) in enumerate(SCHED):
        # (ToyRank.step restated with every rank's step cut at its collectives)
        states = [rk.x for rk in ranks]
        bufs = [[np.array([math.sin(x + k + j), x * (j + 1), float(r == j)]) for j in range(pieces)] for r, x in enumerate(states)]
        tot = [sum(b[j] for b in bufs) for j in range(pieces)]
        s = sum(float(np.sum(t)) for t in tot)
        for r, rk in enumerate(ranks):
            rk.x = math.cos(rk.x) + 0.1 * s
        if learn:
            g = sum(np.array([rk.x * s + rk.r, 1.0]) for rk in ranks)
            for rk in ranks:
                rk.x -= 0.01 * g[0] / g[1]
    want = [rk.x for rk in ranks]
    # replay
    rp = ST.Replay(world, groups, ST.NumpyBuffers())
    toys = [ToyRank(r, pieces) for r in range(world)]
    hooks = [rp.hook(r) for r in range(world)]

    def run_rank(r):
        toys[r].begin()
        for k, (_, _, learn, _) in enumerate(SCHED):
            toys[r].step(k, learn, lambda q, b: hooks[q](b, b.size, None))
        return toys[r].x
    got = rp.run(run_rank)
    assert rp.passes == len(groups) + 1 == 9
    assert rp.frontiers == [0] + list(np.cumsum(groups)) and rp.frontiers[-1] == rp.total == len(rp.counts)
    assert np.allclose(got, want, rtol=1e-14, atol=0.0)                            # (sums in rank order on both sides)
    assert all(len(s) == rp.total for s in rp.summed)
    for k in range(rp.total):                                                       # the same sum on every rank
        assert all(np.array_equal(rp.summed[r][k], rp.summed[0][k]) for r in range(world))


def test_a_rank_that_does_not_repeat_itself_is_caught_by_the_driver():
    """Replay rests on repeatability: a piece that differs in its last bit from the one recorded for it fails the bitwise check."""
    import itertools
    rp = ST.Replay(2, ST.groups_of(SCHED, 1), ST.NumpyBuffers())
    drift = (1e-16 * i for i in itertools.count())
    toys = [ToyRank(0, 1), ToyRank(1, 1, jitter=drift)]
    hooks = [rp.hook(r) for r in range(2)]

    def run_rank(r):
        toys[r].begin()
        for k, (_, _, learn, _) in enumerate(SCHED):
            toys[r].step(k, learn, lambda q, b: hooks[q](b, b.size, None))
    with pytest.raises(AssertionError, match="not the one it recorded"):
        rp.run(run_rank)


def test_schedules_of_the_gpu_cases_reach_the_stated_shards():
    """What tests/test_gpu_sharded_train.py's table says about its shards, from shard_bounds."""
    S = lambda name, world, nsteps=None: ST.slices_of(ST.truncated(TS.get_case(name), nsteps)["sched"], world)
    assert S("m12_d1_iso_m32", 3) == [[85, 85, 85], [86, 85, 85], [21, 21, 21], [29, 29, 29], [1, 0, 0]]
    assert S("m65_d32_ard_se", 2, 3) == [[128, 128], [71, 71], [1, 0]]
    assert S("m65_d5_iso_m12", 2, 2) == [[129, 128], [37, 36]]
    assert S("w1000_m130_d3_se", 3, 2) == [[334, 333, 333], [86, 85, 85]]
    assert S("g1", 2) == [[129, 128], [71, 71]]
    assert S("g1e-4", 3) == [[67, 67, 66], [67, 67, 66], [21, 21, 21]]
    assert S("mixed", 3) == [[3, 2, 2], [86, 86, 85]]
    assert S("g1_empty", 3) == [[1, 1, 0], [67, 67, 66]]
    assert ST.n_max_of(TS.get_case("g1_empty")["sched"], 3) == 67 and ST.n_max_of(TS.get_case("w1000_m130_d3_se")["sched"][:2], 3) == 334
