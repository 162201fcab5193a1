"""Data-sharded TRAINING runs simulated in one process (helper, no tests): the replay all-reduce that
tests/test_gpu_sharded_train.py and tests/test_sharded_train_host.py share, and the NumPy rank the host file drives it with.

tests/sharded_ref.py sums every operation in two passes -- capture, then add.  A training run cannot be summed that way: theta, the
AdaMax state, q(v) and q(w) live on the device from step to step, so a step's local contribution is only the true one once every
collective before it has been summed.  The run is therefore REPLAYED: every pass starts every rank from scratch (`train_begin`
again) and runs the whole schedule; the hook of a pass with frontier f replaces the buffer of call k < f by the sum of all ranks'
recorded pieces of call k -- added in rank order from a clone, as sharded_ref.Rank does, the same bits on every rank -- and only
clones the piece of a call k >= f.  What a rank hands the hook at the frontier is then its true local contribution (everything it
depends on was summed); those pieces are recorded and the frontier advances by one GROUP: the pieces of one sweep (they do not
depend on each other), or the gradient's 33 doubles (they depend on that sweep's summed statistics and come a pass later).  A
schedule of s steps of which l learn has s + l groups and takes s + l + 1 passes, 2 s + 1 when every step learns; the last pass
sums every call, its results are the run's, and it keeps a copy of every summed piece.  What a pass computes behind its frontier
is local-only and is ignored.

The ranks run one after another in one process: no threads, nothing waits for another rank, nothing can block.  Replay rests on
repeatability, which is asserted rather than assumed: a rank's own piece of every call k < f must be, bitwise, the one recorded
for it in the earlier pass; and every rank must issue the same sequence of counts as every other rank and as in every earlier
pass (an empty rank included: a rank that leaves out a collective is a deadlock on real hardware).
"""
from __future__ import annotations

import contextlib

import numpy as np
from scipy.linalg import cholesky

from gaussianprocessnode_amd.distributed import ShardedDevice, shard_bounds
from oracle import sgp_oracle as O
from tests import sharded_ref as SR
from tests import train_step_ref as TS

GRAD_SLOTS = SR.GRAD_SLOTS


# ---------------------------------------------------------------------------------------------------------------------------
# the schedule's collectives
# ---------------------------------------------------------------------------------------------------------------------------
def step_counts(sched, stats_counts):
    """The documented hook counts of every step: the sweep's statistics pieces (sharded_ref.plain_counts / planned_counts), then
    GRAD_SLOTS on a learning step and nothing on a step without learning."""
    return [list(stats_counts) + ([GRAD_SLOTS] if learn else []) for _, _, learn, _ in sched]


def groups_of(sched, n_stats_pieces=1):
    """The frontier's advances: per step the sweep's pieces at once, then (learning steps) the gradient's one."""
    out = []
    for _, _, learn, _ in sched:
        out.append(int(n_stats_pieces))
        if learn:
            out.append(1)
    return out


def split_steps(calls, per_step):
    """A flat sequence of hook counts cut into the steps' shares (the lengths of `per_step`)."""
    out, k = [], 0
    for want in per_step:
        out.append(list(calls[k:k + len(want)]))
        k += len(want)
    assert k == len(calls), (k, len(calls))
    return out


def slices_of(sched, world):
    """Every step's slice lengths, one per rank (gaussianprocessnode_amd.distributed.shard_bounds)."""
    return [[hi - lo for lo, hi in (shard_bounds(n, world, r) for r in range(world))] for _, n, _, _ in sched]


def same_bits(a, b):
    """Two outputs of a run (arrays, numbers, tuples of them, None where a run has none) agree in every bit."""
    if a is None or b is None:
        return a is b
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    a, b = (np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64))) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def n_max_of(sched, world):
    """One n_max for every rank of the run: the largest slice of the largest window (at least 1)."""
    return max(1, max(max(s) for s in slices_of(sched, world)))


# ---------------------------------------------------------------------------------------------------------------------------
# the buffers a hook is handed: device memory on the stream the library names, or a NumPy array (the host file's rank)
# ---------------------------------------------------------------------------------------------------------------------------
class NumpyBuffers:
    def on(self, stream):
        return contextlib.nullcontext()

    def view(self, buf, n):
        assert isinstance(buf, np.ndarray) and buf.dtype == np.float64 and buf.shape == (n,), (type(buf), n)
        return buf

    def clone(self, t):
        return t.copy()

    def add(self, acc, part):
        acc += part

    def write(self, t, acc):
        t[:] = acc

    def same_bits(self, a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))

    def numpy(self, t):
        return t.copy()

    def synchronize(self):
        pass


class TorchBuffers:
    """The sums are taken on the hook's stream through torch.cuda.ExternalStream, as sharded_ref.Rank takes them."""

    def __init__(self):
        import torch
        from gaussianprocessnode_amd.distributed import device_tensor
        self.torch, self.device_tensor = torch, device_tensor

    def on(self, stream):
        return self.torch.cuda.stream(self.torch.cuda.ExternalStream(stream))

    def view(self, buf, n):
        return self.device_tensor(buf, n)

    def clone(self, t):
        return t.clone()

    def add(self, acc, part):
        acc.add_(part)

    def write(self, t, acc):
        t.copy_(acc)

    def same_bits(self, a, b):
        return a.shape == b.shape and self.torch.equal(a.view(self.torch.int64), b.view(self.torch.int64))

    def numpy(self, t):
        return t.cpu().numpy()

    def synchronize(self):
        self.torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------------------------------------
class Replay:
    """`world` hooks, made once (`hook(r)`: install it once on rank r's device), and the passes over them (`run`)."""

    def __init__(self, world, groups, buffers):
        assert world >= 1 and len(groups) >= 1 and all(g >= 1 for g in groups), (world, groups)
        self.world, self.groups, self.B = int(world), [int(g) for g in groups], buffers
        self.total = sum(self.groups)
        self.frontiers = [0] + [int(v) for v in np.cumsum(self.groups)]           # one pass each; the last one sums every call
        self.recorded = [[] for _ in range(world)]        # [rank][call]: the true local pieces, calls below the frontier
        self.counts = None                                # the sequence of counts every rank issued in the first pass
        self.frontier, self.final, self.passes = 0, False, 0
        self._begin()

    def _begin(self):
        self.calls = [[] for _ in range(self.world)]      # this pass: counts,
        self.own = [[] for _ in range(self.world)]        # the rank's own pieces of calls below the frontier (before the sum),
        self.fresh = [[] for _ in range(self.world)]      # its cloned pieces of the calls from the frontier on,
        self.summed = [[] for _ in range(self.world)]     # and (last pass) copies of the sums

    def hook(self, r):
        B = self.B

        def fn(buf, n, stream):
            k = len(self.calls[r])
            with B.on(stream):
                t = B.view(buf, n)
                if k < self.frontier:
                    for q in range(self.world):
                        assert k < len(self.recorded[q]) and self.recorded[q][k].shape == (n,), \
                            f"rank {r}, call {k}: {n} doubles where rank {q} recorded {[tuple(p.shape) for p in self.recorded[q][k:k + 1]]}"
                    mine = B.clone(t)
                    parts = [mine if q == r else self.recorded[q][k] for q in range(self.world)]
                    acc = B.clone(parts[0])
                    for part in parts[1:]:
                        B.add(acc, part)
                    B.write(t, acc)
                    self.own[r].append(mine)
                    if self.final:
                        self.summed[r].append(acc)
                else:
                    self.fresh[r].append(B.clone(t))
            self.calls[r].append(int(n))
        return fn

    def _check(self):
        """After a pass: the same counts on every rank and in every pass; the pieces below the frontier are bitwise the recorded ones."""
        for r in range(self.world):
            assert self.calls[r] == self.calls[0], f"pass {self.passes}: rank {r} issued {self.calls[r]}, rank 0 {self.calls[0]}"
        if self.counts is None:
            self.counts = list(self.calls[0])
        assert self.calls[0] == self.counts, f"pass {self.passes}: counts {self.calls[0]}, first pass {self.counts}"
        assert len(self.counts) == self.total, f"{len(self.counts)} collectives per rank, the schedule's groups say {self.total}"
        for r in range(self.world):
            assert len(self.own[r]) == self.frontier
            for k, (a, b) in enumerate(zip(self.own[r], self.recorded[r])):
                assert self.B.same_bits(a, b), f"pass {self.passes}: rank {r}'s piece of call {k} is not the one it recorded"

    def run(self, run_rank):
        """run_rank(r) -> rank r's results of one whole run from scratch (its device calls `hook(r)`).  Returns the last pass's
        results, one per rank."""
        results = None
        for p, f in enumerate(self.frontiers):
            self.frontier, self.final = f, f == self.total
            self._begin()
            results = [run_rank(r) for r in range(self.world)]
            self.B.synchronize()                          # (between this pass's clones and the next pass's sums)
            self._check()
            self.passes += 1
            if not self.final:
                for r in range(self.world):
                    self.recorded[r].extend(self.fresh[r][:self.groups[p]])
        assert self.final and self.passes == len(self.groups) + 1
        return results

    def summed_numpy(self):
        return [[self.B.numpy(t) for t in s] for s in self.summed]


# ---------------------------------------------------------------------------------------------------------------------------
# the device side: one handle per rank behind distributed.ShardedDevice, every pass a `train_begin` again
# ---------------------------------------------------------------------------------------------------------------------------
class ProbedShard(ShardedDevice):
    """ShardedDevice that notes, per step, its slice length and what the library plans for the step's sweep."""

    def __init__(self, dev, rank, world):
        super().__init__(dev, rank, world)
        self.slices, self.plans = [], []

    def train_step(self, offset, n, learn=True, reset_prior=False):
        lo, hi = self._slice(n)
        self.slices.append(hi - lo)
        self.plans.append(self.dev.overlap_plan())
        super().train_step(offset, n, learn, reset_prior)


def truncated(case, nsteps=None):
    return case if nsteps is None else {**case, "sched": case["sched"][:nsteps]}


def device_replay(G, device_run, name, world, nsteps=None, overlap=None):
    """Case `name` of train_step_ref (its first `nsteps` steps) on `world` simulated ranks.  `device_run`:
    tests/test_gpu_train_step.device_run, which collects a rank's observable outputs after train_end.  Returns a dict:
    results (one per rank), calls (per rank, the last pass's counts), summed (per rank, NumPy copies of the summed pieces), slices
    (per rank and step), plans_idle (per rank: overlap_plan() with the hook installed, before the run), plans (per rank and step:
    overlap_plan() inside the run), passes, n_max."""
    case = truncated(TS.get_case(name), nsteps)
    sched = case["sched"]
    M, D = case["Xu"].shape
    n_max = n_max_of(sched, world)
    rp = Replay(world, groups_of(sched), TorchBuffers())
    shards = []
    try:
        with SR.overlap_env(overlap):                       # (the library reads SGP_OVERLAP in sgp_create)
            for r in range(world):
                dev = G.SGPDevice(n_max, M, D)
                shards.append(ProbedShard(dev, r, world))
                dev.set_allreduce(rp.hook(r))               # once
        plans_idle = [s.dev.overlap_plan() for s in shards]

        def run_rank(r):
            shards[r].slices, shards[r].plans = [], []
            return device_run(G, case, shards[r])
        results = rp.run(run_rank)
        return dict(results=results, calls=[list(c) for c in rp.calls], summed=rp.summed_numpy(), slices=[list(s.slices) for s in shards],
                    plans=[list(s.plans) for s in shards], plans_idle=plans_idle, passes=rp.passes, n_max=n_max)
    finally:
        for s in shards:
            s.dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the last step's whole-window statistics by the reference, and what its theta tolerance lets them move by
# ---------------------------------------------------------------------------------------------------------------------------
def last_window_stats(name, nsteps=None):
    """(Psi2, B, n, allowance for Psi2, allowance for B) of the last step's WHOLE window at the reference's theta of that step.
    Allowances (relative Frobenius): train_step_ref.compare_outputs' model for the kernel left behind -- a kernel value moves by at
    most (1 + s) of its size per unit of relative change in sigma2 or a lengthscale, and the reference's theta is held to
    theta_tol, 4 x rel_theta in softplus(theta) -- so with d = 4 rel_theta (1 + s_max) every entry of K_uf moves by at most d of
    its size, every entry of Psi2 = K_uf K_uf' (all kernel values >= 0) by 2 d, and B = K_uf y by d |K_uf| |y|.  s_max is taken
    over the entries that are not exactly 0 (a value that underflowed at s > 1400 stays 0 under a relative change << 1)."""
    ref, case = TS.reference(name, nsteps), TS.get_case(name)
    rec = ref["log"][-1]
    off, n = rec["offset"], rec["n"]
    p = O.softplus(rec["theta"])
    ell = TS.full_ell(p[1:], case["Xu"].shape[1])
    Xw = case["X"][off:off + n]
    y = rec["mf"] if case["likelihood"] == "probit" else case["y"][off:off + n]
    Kuf = TS.kernelmatrix(case["family"], p[0], ell, case["Xu"], Xw)
    s = TS.sq_dist(ell, case["Xu"], Xw)
    smax = float(np.max(s[Kuf > 0.0]))
    rel_theta = float(np.max(ref["theta_tol"] / O.softplus(ref["theta"]))) if ref["steps"] else 0.0
    d = 4.0 * rel_theta * (1.0 + smax)
    B = Kuf @ y
    return Kuf @ Kuf.T, B, n, 2.0 * d, d * float(np.linalg.norm(np.abs(Kuf) @ np.abs(y)) / np.linalg.norm(B))


# ---------------------------------------------------------------------------------------------------------------------------
# the host file's rank: one step of train_step_ref.TrainRef over a slice, with the exchange where the header puts it
# ---------------------------------------------------------------------------------------------------------------------------
RANK_FAULTS = ("gamma_counts_local_slice", "grad_payload_unsummed", "grad_slot_dropped", "empty_rank_skips_grad", "syy_from_local_slice")


class NumpyRank(TS.TrainRef):
    """A rank of a data-sharded run in NumPy, from train_step_ref's pieces (kernels, Probit moments, the oracle's q(v) update and
    traces, AdaMax) and include/sgp_hip.h's text: the window's statistics AND data scalars of this rank's slice go through the hook
    in the exchange buffer's layout (sharded_ref.pack_exchange); q(v), sum I1 / I2 and the Gamma update -- whose shape counts
    SGP_S_N of the reduced buffer -- come from the sum; the data half of the gradient (one slot per dimension, 33 doubles) goes
    through the hook, the K_uu half and the n / 2 term come from the reduced statistics, and one lengthscale's derivative is summed
    over the dimensions after the reduce.  The interface is the device's: set_allreduce, train_begin, train_step over a slice,
    train_end.  `fault`: one of RANK_FAULTS (`slot`: the payload slot of grad_slot_dropped)."""

    def __init__(self, case, fault=None, slot=None):
        self.case, self.rank_fault, self.slot, self.hook = case, fault, slot, None
        self.train_begin()

    def set_allreduce(self, fn):
        self.hook = fn

    def train_begin(self):
        c = self.case
        super().__init__(c["X"], c["y"], c["Xu"], c["theta0"], prior=c["prior"], **c["kw"])

    def _reduce(self, buf):
        if self.hook is not None:
            self.hook(buf, buf.size, None)

    def train_step(self, offset, n, learn=True, reset_prior=False):
        if reset_prior:
            self.Lambda0, self.xi0 = np.eye(self.M) / self.prior_var, np.zeros(self.M)
        s2, ell = self.kernel()
        Xw, yw = self.X[offset:offset + n].reshape(n, self.D), self.y[offset:offset + n]
        w = self.w
        if self.probit:
            mz = TS.kernelmatrix(self.family, s2, ell, Xw, self.Xu) @ self.mu
            mf, vf, _, _ = TS.probit_moments(yw, mz, 1.0 / w)
        else:
            mf, vf = yw, None
        Kuu0 = TS.kernelmatrix(self.family, s2, ell, self.Xu, self.Xu)
        Kuu = Kuu0 + self.jitter * np.eye(self.M)
        Kuf = TS.kernelmatrix(self.family, s2, ell, self.Xu, Xw)
        syy_local = float(np.sum(mf * mf) + (0.0 if vf is None else np.sum(vf)))
        P = Kuf @ Kuf.T
        buf = SR.pack_exchange(np.tril(P) + np.tril(P, -1).T, Kuf @ mf, SR.scalars_vector(syy_local, float(n), float(n), [[syy_local]]))
        self._reduce(buf)
        Psi2, B, sc = SR.unpack_exchange(buf, self.M)
        syy = syy_local if self.rank_fault == "syy_from_local_slice" else float(sc[0])
        n_all = float(sc[2])
        stats = O.SuffStats(Psi2, B.reshape(self.M, 1), np.array([[syy]]), s2 * float(sc[1]), n_all)
        Lam = self.Lambda0 + w * Psi2
        ok = True
        try:
            L = cholesky(Kuu, lower=True)
            cholesky(Lam, lower=True)
        except np.linalg.LinAlgError:
            ok = False
        gscale = 1.0
        if ok:
            mu, Sigma, _ = O.v_update(stats, w, Lambda0=self.Lambda0, xi0=self.xi0)
            sum_I1, sum_I2 = O.w_stats_trace(stats, L, mu, Sigma)
            self.Lambda0, self.xi0 = Lam, self.xi0 + w * stats.b[:, 0]
            self.mu, self.Sigma = mu, Sigma
            self.log.append(dict(sum_I2=sum_I2))
            if self.probit:
                n_gamma = float(n) if self.rank_fault == "gamma_counts_local_slice" else n_all
                self.a, self.b = O.gamma_update(self.a, self.b, n_gamma, sum_I1, sum_I2)
                self.w = self.a / self.b
                gscale = self.w / w
        else:
            self.skipped += 1
        if not learn or (self.rank_fault == "empty_rank_skips_grad" and n == 0):
            return
        # the gradient (train_step_ref.theta_grad): data half per slot over this rank's points, reduced; K_uu half replicated
        pay = np.zeros(GRAD_SLOTS)
        if ok:
            Kinv = np.linalg.inv(Kuu)
            s_uu, s_uf = TS.sq_dist(ell, self.Xu, self.Xu), TS.sq_dist(ell, self.Xu, Xw)
            A = (Sigma + np.outer(mu, mu) - Kinv) @ Kuf - np.outer(mu, mf)
            dsf = -2.0 * s2 * TS.dkappa_ds(self.family, s_uf)
            d_uf = [Kuf / s2] + [dsf * (self.Xu[:, k:k + 1] - Xw[None, :, k]) ** 2 / ell[k] ** 3 for k in range(self.D)]
            pay[:1 + self.D] = [np.sum(A * f) for f in d_uf]
        local = pay.copy()
        self._reduce(pay)
        if self.rank_fault == "grad_payload_unsummed":
            pay = local
        elif self.rank_fault == "grad_slot_dropped":
            pay[self.slot] = local[self.slot]
        if not ok:
            return                                                       # a rejected minibatch: counted, theta left alone
        H = Kinv @ Psi2 @ Kinv
        dsu = -2.0 * s2 * TS.dkappa_ds(self.family, s_uu)
        # (the jitter is no part of dK_uu)
        d_uu = [Kuu0 / s2] + [dsu * (self.Xu[:, k:k + 1] - self.Xu[None, :, k]) ** 2 / ell[k] ** 3 for k in range(self.D)]
        full = pay[:1 + self.D] + np.array([0.5 * np.sum(H * u) for u in d_uu])
        full[0] += 0.5 * n_all
        if self.n_ell == 1:
            full = np.array([full[0], full[1:].sum()])
        self._adamax(gscale * w * full * TS.sigmoid(self.theta))
        self.steps += 1

    def train_end(self):
        """The run's outputs in the form train_step_ref.compare_outputs takes (train_step_ref.observed)."""
        out = self.observables()
        out["log"] = self.log
        return TS.observed(self.case, out)


def host_replay(name, world, nsteps=None, fault=None, slot=None, faulty_ranks=None):
    """Case `name` on `world` NumPy ranks through the same Replay as the device runs.  Returns (results per rank, the Replay)."""
    case = truncated(TS.get_case(name), nsteps)
    sched = case["sched"]
    rp = Replay(world, groups_of(sched), NumpyBuffers())
    ranks = []
    for r in range(world):
        rk = NumpyRank(case, fault if faulty_ranks is None or r in faulty_ranks else None, slot)
        rk.set_allreduce(rp.hook(r))                          # once
        ranks.append(ShardedDevice(rk, r, world))

    def run_rank(r):
        ranks[r].train_begin()
        for off, n, learn, reset in sched:
            ranks[r].train_step(off, n, learn, reset_prior=reset)
        return ranks[r].train_end()
    return rp.run(run_rank), rp
