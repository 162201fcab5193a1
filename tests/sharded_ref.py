"""Data-sharded sweeps simulated in one process (helper, no tests): the cases, their whole-data references and the two-pass
all-reduce that tests/test_gpu_shards.py, tests/test_gpu_sharded_shapes.py and tests/test_sharded_host.py share.

A run has `world` ranks, one handle each, all created with the same `n_max` (include/sgp_hip.h, sgp_config.n_max), every rank
holding its slice of the points.  A sum-all-reduce is simulated in two passes over the ranks: in the first every rank's hook
clones the pieces the library hands it (this rank's local contribution), in the second the hook adds the other ranks' pieces,
call by call, to the buffer -- what the collective would leave there, the same bits on every rank -- and keeps a copy of the
sum.  Every operation of a sequence (`run`) goes through both passes; the setters that make the library form its statistics
again are repeated in the second pass, so that both passes issue the same collectives.

The exchange buffer's layout is restated here in NumPy from the header's text (sgp_set_allreduce, sgp_stats_layout), not from
the kernels: `pack_exchange` / `unpack_exchange`.

Bounds.  `ratios` turns one rank's results into error / bound for every compared quantity; the bounds are the project's:
1e-13 (relative Frobenius, or relative) for summed statistics and scalars, `post_tol(cond(Lambda))` for q(v), the `tol_I1`
forms of test_gpu_parity / test_gpu_shards for sum I1, the energy and the Wishart inverse scale, train_step_ref's gradient
bound for the theta gradient.  The GPU file asserts every ratio < 1; the host file shows that damaged sums give ratios >= 10.
"""
from __future__ import annotations

import contextlib
import functools
import math
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from gaussianprocessnode_amd.distributed import S_COUNT, TILE, padded, shard_bounds
from oracle import sgp_oracle as O
from tests import train_step_ref as TS
from tests.test_gpu_parity import post_tol, relF
from tests.test_kernel_family_host import matern

EPS = float(np.finfo(np.float64).eps)
STAT_TOL = 1e-13            # summed statistics and data scalars (test_gpu_shards)
GRAD_SLOTS = 33             # the theta gradient's payload: 1 + 32 doubles (include/sgp_hip.h, sgp_set_allreduce)
FULL, TARGETS, REUSED = 0, 1, 2       # SGP_SWEEP_*


# ---------------------------------------------------------------------------------------------------------------------------
# the exchange buffer (include/sgp_hip.h): [lower 64 x 64 tiles of Psi2 | B | scalars], T (T + 1) / 2 tiles with T = ceil(M / 64) in
# row-major triangle order -- (0,0), (1,0), (1,1), (2,0), .. --, each tile column-major; B is Mp x d_out column-major; the scalars are
# SGP_S_COUNT slots followed by Ryy (d_out x d_out, column-major)
# ---------------------------------------------------------------------------------------------------------------------------
def tile_rows(M):
    return padded(M) // TILE


def tail_count(M, d_out=1):
    return padded(M) * d_out + S_COUNT + d_out * d_out


def pack_count(M, d_out=1):
    T = tile_rows(M)
    return T * (T + 1) // 2 * TILE * TILE + tail_count(M, d_out)


def tile_order(T):
    return [(I, J) for I in range(T) for J in range(I + 1)]


def scalars_vector(s_yy, s_w, n_nodes, Ryy):
    Ryy = np.atleast_2d(np.asarray(Ryy, dtype=np.float64))
    out = np.zeros(S_COUNT + Ryy.size)
    out[0], out[1], out[2] = s_yy, s_w, n_nodes
    out[S_COUNT:] = Ryy.T.reshape(-1)
    return out


def pack_exchange(Psi2, B, scalars):
    Psi2 = np.asarray(Psi2, dtype=np.float64)
    M = Psi2.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(M, -1)
    d_out, Mp, T = B.shape[1], padded(M), tile_rows(M)
    P = np.zeros((Mp, Mp))
    P[:M, :M] = Psi2
    out = np.zeros(pack_count(M, d_out))
    for t, (I, J) in enumerate(tile_order(T)):
        tile = P[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE]
        out[t * TILE * TILE:(t + 1) * TILE * TILE] = tile.T.reshape(-1)            # column-major
    off = len(tile_order(T)) * TILE * TILE
    Bp = np.zeros((Mp, d_out))
    Bp[:M] = B
    out[off:off + Mp * d_out] = Bp.T.reshape(-1)
    out[off + Mp * d_out:] = scalars
    return out


def unpack_exchange(buf, M, d_out=1, unmirrored=None):
    """(Psi2 (M, M) full symmetric, B (M, d_out), scalars (SGP_S_COUNT + d_out^2)).  `unmirrored`: an off-diagonal tile (I, J) whose
    mirror image is left out (the damage of the host file's discrimination test)."""
    buf = np.asarray(buf, dtype=np.float64)
    Mp, T = padded(M), tile_rows(M)
    assert buf.size == pack_count(M, d_out), (buf.size, pack_count(M, d_out))
    P = np.zeros((Mp, Mp))
    for t, (I, J) in enumerate(tile_order(T)):
        tile = buf[t * TILE * TILE:(t + 1) * TILE * TILE].reshape(TILE, TILE).T
        P[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] = tile
        if I != J and (I, J) != unmirrored:
            P[J * TILE:(J + 1) * TILE, I * TILE:(I + 1) * TILE] = tile.T
    off = len(tile_order(T)) * TILE * TILE
    B = buf[off:off + Mp * d_out].reshape(d_out, Mp).T[:M].copy()
    return P[:M, :M].copy(), B, buf[off + Mp * d_out:].copy()


def unpack_tail(buf, M, d_out=1):
    """(B, scalars) of a tail-only piece (a SGP_SWEEP_TARGETS sweep's collective)."""
    buf = np.asarray(buf, dtype=np.float64)
    Mp = padded(M)
    assert buf.size == tail_count(M, d_out)
    return buf[:Mp * d_out].reshape(d_out, Mp).T[:M].copy(), buf[Mp * d_out:].copy()


def ryy_of(scalars, d_out):
    return np.asarray(scalars[S_COUNT:S_COUNT + d_out * d_out]).reshape(d_out, d_out).T.copy()


def plain_counts(M, d_out=1):
    return [pack_count(M, d_out)]


def planned_counts(plan, M, d_out=1):
    """The documented sequence of a full sweep's collectives: the whole buffer in the plain order (no plan), else one piece per
    statistics group, the tail travelling with the first."""
    if not plan:
        return plain_counts(M, d_out)
    return [g["tiles"] * TILE * TILE + (tail_count(M, d_out) if i == 0 else 0) for i, g in enumerate(plan)]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int = 0                      # UniSGP: points.  MultiSGP: set by `nodes` (N = nodes x (2 D + 1) cubature points)
    D: int = 2
    d_out: int = 1
    nodes: int = 0                  # MultiSGP: factor nodes, each with the 2 D + 1 points of the spherical-radial rule
    world: int = 2
    shards: Optional[Tuple[int, ...]] = None      # explicit shard sizes; None: `shard_bounds`
    family: str = "se"
    prior: str = "iso"              # "iso" (form 2), "precision" (form 1), "meancov" (form 0)
    weighted: bool = False          # UniSGP: point weights, three points per factor node
    y_var: bool = False
    overlap: bool = False           # SGP_OVERLAP=1 (else 0)
    reuse: bool = False             # handles created with reuse_stats
    n_ell: int = 0                  # 0: ARD (D lengthscales); 1: isotropic
    sigma2: float = 0.9
    ell: float = 0.8
    w: float = 30.0
    jitter: float = 1e-8
    xu: str = "data"                # inducing inputs: rows of X ("data"), or a permuted grid per dimension ("grid")
    seed: int = 0

    @property
    def n_points(self):
        return self.nodes * (2 * self.D + 1) if self.d_out > 1 else self.N

    @property
    def sizes(self):
        if self.shards is not None:
            assert sum(self.shards) == self.n_points and len(self.shards) == self.world, self.name
            return tuple(self.shards)
        return tuple(hi - lo for lo, hi in (shard_bounds(self.n_points, self.world, r) for r in range(self.world)))

    @property
    def bounds(self):
        edges = np.concatenate([[0], np.cumsum(self.sizes)])
        return [(int(edges[r]), int(edges[r + 1])) for r in range(self.world)]

    @property
    def n_max(self):
        return max(max(self.sizes), 1)


def _uni(name, M, N, world, seed, **kw):
    return Case(name=name, M=M, N=N, world=world, seed=seed, **kw)


def _multi(name, d_out, M, nodes, shards, seed, **kw):
    return Case(**{**dict(name=name, M=M, d_out=d_out, nodes=nodes, world=len(shards), shards=tuple(shards), prior="precision",
                          sigma2=0.8, ell=1.1, seed=seed), **kw})


# UniSGP sweeps, plain order: tile rows 1, 1, 2, 3 and 4, all padded; shard_bounds gives uneven shards (N mod world != 0)
SWEEP_UNI = [
    _uni("u_m1", 1, 151, 2, 1),
    _uni("u_m63", 63, 301, 3, 2),
    _uni("u_m65", 65, 401, 2, 3),
    _uni("u_m130", 130, 352, 3, 4),
    _uni("u_m200", 200, 451, 2, 5),
    _uni("u_m130_overlap", 130, 352, 3, 4, overlap=True),
    _uni("u_m200_overlap", 200, 451, 2, 5, overlap=True),
    _uni("u_m65_weights_yvar", 65, 402, 3, 6, shards=(171, 98, 133), weighted=True, y_var=True),
    _uni("u_m65_d3_matern12", 65, 333, 2, 7, D=3, family="matern12", ell=1.4),
    _uni("u_m65_d3_matern32", 65, 334, 3, 8, D=3, family="matern32", ell=1.4),
    _uni("u_m65_d3_matern52", 65, 335, 2, 9, D=3, family="matern52", ell=1.4),
    _uni("u_m65_prior_meancov", 65, 311, 2, 10, prior="meancov"),
    _uni("u_m65_prior_precision", 65, 311, 3, 11, prior="precision"),
    _uni("u_m130_empty_rank", 130, 341, 3, 12, shards=(200, 141, 0)),
]
# MultiSGP: cubature weights, Gaussian q_out, non-diagonal W; the shards cut through nodes (5 or 11 points each), so every rank's
# n_nodes and output-covariance shares are fractional
SWEEP_MULTI = [_multi(f"m_o{do}_m{M}", do, M, 60, (131, 97, 72) if (do + M) % 2 else (163, 137), 100 + 10 * do + k)
               for do in (2, 3, 4) for k, M in enumerate((21, 65, 130)) if (do, M) != (3, 65)]
SWEEP_MULTI += [_multi("m_o3_m65_d5", 3, 65, 30, (149, 103, 78), 31, D=5, ell=1.6),
                _multi("m_o2_m130_overlap", 2, 130, 61, (153, 152), 32, overlap=True)]
# more than 384 points on one rank: more than 24 chunks of 16 points, where the assembly of the statistics takes its many-chunks
# form (one entry per thread) -- the other rank, and every case above, takes the few-chunks form
SWEEP_UNI += [_uni("u_m65_weights_yvar_n700", 65, 700, 2, 13, shards=(450, 250), weighted=True, y_var=True),
              _uni("u_m130_weights_n700", 130, 700, 2, 14, shards=(250, 450), weighted=True)]
SWEEP_MULTI += [_multi("m_o2_m65_n700", 2, 65, 140, (451, 249), 33)]
# targets and reuse
REUSE = [_uni("r_u_m65_yvar", 65, 377, 3, 40, y_var=True, reuse=True),
         _multi("r_m_o2_m96", 2, 96, 61, (162, 143), 41, reuse=True)]
# theta objective (UniSGP): inducing inputs on a permuted grid, as train_step_ref's cases, so that cond(K_uu) leaves the gradient
# bound far below the gradient; reuse_stats handles, so that sweep_kind() after a re-evaluation says something
THETA = [
    _uni("t_d1", 12, 257, 2, 50, reuse=True, D=1, ell=0.5, w=20.0, xu="grid", jitter=1e-8),
    _uni("t_d8_iso", 40, 301, 3, 51, reuse=True, D=8, n_ell=1, ell=2.5, w=20.0, xu="grid"),
    _uni("t_d32_ard_m65", 65, 263, 2, 52, reuse=True, D=32, ell=5.0, w=20.0, xu="grid"),
    _uni("t_weights_yvar", 30, 302, 3, 53, reuse=True, shards=(120, 71, 111), weighted=True, y_var=True, ell=0.5, w=20.0, xu="grid"),
    _uni("t_d3_matern52", 65, 299, 2, 54, reuse=True, D=3, family="matern52", ell=1.4, w=20.0, xu="grid"),
]
CASES = {c.name: c for c in SWEEP_UNI + SWEEP_MULTI + REUSE + THETA}
assert len(CASES) == len(SWEEP_UNI) + len(SWEEP_MULTI) + len(REUSE) + len(THETA)
assert len({c.seed for c in CASES.values() if not c.overlap}) == len([c for c in CASES.values() if not c.overlap])


def ell_of(case):
    """The lengthscales as the handle takes them (n_ell entries) and over all dimensions."""
    n_ell = case.n_ell or case.D
    ell = np.full(1, case.ell) if n_ell == 1 else case.ell * np.linspace(0.85, 1.2, case.D)
    return ell, np.broadcast_to(ell, (case.D,)).copy()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The whole-data inputs of a case (arrays shared between the tests: not to be written to).  Two versions of the targets
    (`Y`, `y_var`, `Sig_y`: index 0 for `set_data`, 1 for `set_targets`) and of the noise (`W`, `E_logw`)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c.seed)
    D, M, n, do = c.D, c.M, c.n_points, c.d_out
    d = dict(case=c)
    if do == 1:
        X = rng.uniform(-1.7, 1.7, (n, D))
        f = np.sin(X @ rng.normal(size=D) / math.sqrt(D) * 2.0)
        d["Y"] = [(f + 0.1 * rng.normal(size=n))[:, None], (np.cos(1.3 * f) - 0.4 + 0.1 * rng.normal(size=n))[:, None]]
        d["y_var"] = [rng.uniform(0.05, 0.5, n), rng.uniform(0.1, 0.9, n)] if c.y_var else [None, None]
        d["omega"] = rng.uniform(0.05, 1.0, n) if c.weighted else None
        d["node_share"] = np.full(n, 1.0 / 3.0 if c.weighted else 1.0)           # the part of a factor node one point carries
        d["Sig_y"] = [None, None]
        W = [np.array([[c.w]]), np.array([[1.8 * c.w]])]
        d["E_logw"] = [math.log(W[0][0, 0]) - 0.01, math.log(W[1][0, 0]) - 0.02]
    else:
        T, S = c.nodes, 2 * D + 1
        means = rng.normal(size=(T, D))
        cub = [O.srcubature(means[t], np.diag(rng.uniform(0.02, 0.2, D))) for t in range(T)]
        d["pts"], d["wts"] = np.stack([q[0] for q in cub]), np.stack([q[1] for q in cub])          # (T, S, D), (T, S)
        X = d["pts"].reshape(T * S, D)
        d["omega"] = d["wts"].reshape(-1)
        d["node_share"] = np.full(n, 1.0 / S)
        d["Yn"] = [rng.normal(size=(T, do)), 0.5 + 1.5 * rng.normal(size=(T, do))]                  # per node
        d["Y"] = [np.repeat(y, S, axis=0) for y in d["Yn"]]
        d["y_var"] = [None, None]

        def covs():
            A = 0.3 * rng.normal(size=(T, do, do))
            return A @ np.transpose(A, (0, 2, 1)) + 0.05 * np.eye(do)
        d["Sig_y"] = [covs(), covs()]
        W = []
        for _ in range(2):
            A = rng.normal(size=(do, do))
            W.append(A @ A.T + do * np.eye(do))                                   # non-diagonal
        d["E_logw"] = [float(np.linalg.slogdet(W[0])[1]) - 0.1, float(np.linalg.slogdet(W[1])[1]) - 0.2]
    d["X"], d["W"] = X, W
    if c.xu == "grid":
        d["Xu"] = np.stack([rng.permutation(np.linspace(-1.7, 1.7, M)) for _ in range(D)], axis=1)
    elif do == 1:
        pool = X if n >= M else rng.uniform(-1.7, 1.7, (M, D))
        d["Xu"] = pool[rng.permutation(len(pool))[:M]].copy()
    else:
        d["Xu"] = rng.uniform(-2.0, 2.0, (M, D))
    d["ell_dev"], d["ell"] = ell_of(c)
    Q = M * do
    if c.prior == "iso":
        d["Lambda0"], d["xi0"] = np.eye(Q) / 50.0, np.zeros(Q)
    elif c.prior == "precision":
        if do == 1:
            A = rng.normal(size=(Q, Q)) / math.sqrt(Q)
            d["Lambda0"] = 0.05 * np.eye(Q) + 0.1 * A @ A.T
        else:
            d["Lambda0"] = np.eye(Q) / 10.0
        d["xi0"] = 0.01 * rng.normal(size=Q)
    else:
        A = rng.normal(size=(Q, Q)) / math.sqrt(Q)
        d["Sigma0"] = 5.0 * np.eye(Q) + 10.0 * A @ A.T
        d["mu0"] = 0.3 * rng.normal(size=Q)
        d["Lambda0"] = O.cholinv(d["Sigma0"])
        d["xi0"] = d["Lambda0"] @ d["mu0"]
    return d


def n_nodes_whole(name):
    d = inputs(name)
    c = d["case"]
    return float(c.nodes) if c.d_out > 1 else (c.N / 3.0 if c.weighted else float(c.N))


def rank_inputs(name, r, targets=0):
    """Rank r's share of a case: its slice of the points, targets, variances and weights, its share of the factor-node count --
    the node fractions its points carry, fractional where a shard cuts through a node -- and of the output-covariance sum."""
    d = inputs(name)
    c = d["case"]
    lo, hi = c.bounds[r]
    cut = lambda a: None if a is None else a[lo:hi]
    share = d["node_share"][lo:hi]
    out = dict(X=d["X"][lo:hi], Y=d["Y"][targets][lo:hi], y_var=cut(d["y_var"][targets]), omega=cut(d["omega"]),
               n_nodes=float(np.sum(share)), cov_sum=None, lo=lo, hi=hi)
    if c.d_out > 1:
        S = 2 * c.D + 1
        node = np.arange(lo, hi) // S
        out["cov_sum"] = np.tensordot(share, d["Sig_y"][targets][node], axes=(0, 0)) if hi > lo else np.zeros((c.d_out, c.d_out))
    return out


@contextlib.contextmanager
def oracle_family(family):
    """The oracle with its kernel replaced by the family's restatement (tests/test_kernel_family_host.py), as
    tests/test_gpu_kernel_family.py patches it."""
    saved = O.kernelmatrix
    O.kernelmatrix = matern(family)
    try:
        yield
    finally:
        O.kernelmatrix = saved


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's statistics of a set of points, and everything a sweep derives from summed statistics
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_stats(name, lo=None, hi=None, targets=0, n_nodes=None, cov_sum=None):
    """(Psi2, B, scalars) of the points [lo, hi) -- the whole data by default -- from the oracle: `suff_stats` with omega, y_var and
    n_nodes for UniSGP; for MultiSGP the same sums over a slice of the cubature points (`multi_suff_stats` takes whole nodes:
    `whole_multi_stats` below is that call, and the host file shows that the two agree on the whole data)."""
    d = inputs(name)
    c = d["case"]
    lo, hi = (0, c.n_points) if lo is None else (lo, hi)
    cut = lambda a: None if a is None else a[lo:hi]
    if hi == lo:                                   # an empty shard contributes zeros
        return np.zeros((c.M, c.M)), np.zeros((c.M, c.d_out)), np.zeros(S_COUNT + c.d_out ** 2)
    with oracle_family(c.family):
        st = O.suff_stats(d["Xu"], d["X"][lo:hi].reshape(hi - lo, c.D), d["Y"][targets][lo:hi], cut(d["y_var"][targets]), c.sigma2,
                          d["ell"], omega=cut(d["omega"]),
                          n_nodes=float(np.sum(d["node_share"][lo:hi])) if n_nodes is None else n_nodes)
    Ryy = st.s_yy.copy()
    if c.d_out > 1:
        S = 2 * c.D + 1
        if cov_sum is None:
            cov_sum = np.tensordot(d["node_share"][lo:hi], d["Sig_y"][targets][np.arange(lo, hi) // S], axes=(0, 0))
        Ryy = Ryy + cov_sum
    return st.Psi2, st.b, scalars_vector(Ryy[0, 0], st.s_kk / c.sigma2, st.n, Ryy)


def whole_multi_stats(name, targets=0):
    d = inputs(name)
    c = d["case"]
    with oracle_family(c.family):
        return O.multi_suff_stats(d["Xu"], d["pts"], d["wts"], d["Yn"][targets], d["Sig_y"][targets], c.sigma2, d["ell"])


def multi_energy(ms, mu, Sig, W, E_logdetW, Kinv):
    """sum over the nodes of `O.multi_average_energy` from the summed statistics (every term is linear in a node's Psi0, Psi1 y',
    Psi2 and Ry)."""
    do, M = ms.B.shape[1], ms.Psi2.shape[0]
    Rv = Sig + np.outer(mu, mu)
    S = sum(Rv[i * M:(i + 1) * M, j * M:(j + 1) * M] * W[i, j] for i in range(do) for j in range(do))
    BW = ms.B @ W
    cross = sum(float(mu[e * M:(e + 1) * M] @ BW[:, e]) for e in range(do))
    return (ms.n * (0.5 * do * O.LOG2PI - 0.5 * E_logdetW) + 0.5 * np.trace(W @ ms.Ryy)
            + 0.5 * np.trace(W) * (ms.s_kk - np.sum(Kinv * ms.Psi2)) - cross + 0.5 * np.sum(ms.Psi2 * S))


def sweep_from_stats(name, Psi2, B, scalars, noise=0):
    """What a sweep leaves on every rank, from summed statistics, by the oracle: q(v), sum I1 / sum I2 / energy, and for MultiSGP
    the Wishart inverse scale -- with the quantities the bounds are made of."""
    d = inputs(name)
    c = d["case"]
    W, E_logw = d["W"][noise], d["E_logw"][noise]
    M, do = c.M, c.d_out
    out = dict(Psi2=Psi2, B=B, scalars=scalars)
    with oracle_family(c.family):
        Kuu = O.kernelmatrix(c.sigma2, d["ell"], d["Xu"]) + c.jitter * np.eye(M)
        cond_K = float(np.linalg.cond(Kuu))
        s_kk = c.sigma2 * scalars[1]
        if do == 1:
            st = O.SuffStats(Psi2, B.reshape(M, 1), np.array([[scalars[0]]]), s_kk, scalars[2])
            r = O.vmp_sweep(d["Xu"], None, None, None, c.sigma2, d["ell"], W[0, 0], E_logw=E_logw, jitter=c.jitter,
                            Lambda0=d["Lambda0"], xi0=d["xi0"], stats=st)
            cond_L = float(np.linalg.cond(d["Lambda0"] + W[0, 0] * Psi2))
            out.update(mu=r.mu_v, Sigma=r.Sigma_v, Uv=r.Uv, sum_I1=r.sum_I1, sum_I2=r.sum_I2, energy=r.energy,
                       tol_I1=50 * EPS * cond_K * s_kk + 1e-12)
        else:
            ms = O.MultiStats(Psi2, B, ryy_of(scalars, do), s_kk, scalars[2])
            mu, Sig = O.multi_v_update(ms, W, d["Lambda0"], d["xi0"])
            Kinv = O.cholinv(Kuu)
            cond_L = float(np.linalg.cond(d["Lambda0"] + np.kron(W, Psi2)))
            out.update(mu=mu, Sigma=Sig, Uv=np.linalg.cholesky(Sig + np.outer(mu, mu)).T, wishart=O.multi_w_update(ms, mu, Sig, Kinv),
                       energy=float(multi_energy(ms, mu, Sig, W, E_logw, Kinv)), tol_I1=50 * EPS * cond_K * c.sigma2 * scalars[2])
    out.update(cond_K=cond_K, cond_L=cond_L, post_tol=post_tol(cond_L), W=W)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, targets=0, noise=0):
    """The whole-data reference of a case (computed once, shared, not to be written to).  UniSGP: `suff_stats` and `vmp_sweep`;
    MultiSGP: `multi_suff_stats`, `multi_v_update`, `multi_w_update` and the per-node `multi_average_energy`."""
    d = inputs(name)
    c = d["case"]
    if c.d_out == 1:
        return sweep_from_stats(name, *oracle_stats(name, targets=targets), noise=noise)
    ms = whole_multi_stats(name, targets)
    ref = sweep_from_stats(name, ms.Psi2, ms.B, scalars_vector(ms.Ryy[0, 0], ms.s_kk / c.sigma2, ms.n, ms.Ryy), noise=noise)
    with oracle_family(c.family):
        Kinv = O.cholinv(O.kernelmatrix(c.sigma2, d["ell"], d["Xu"]) + c.jitter * np.eye(c.M))
        U = 0.0
        for t in range(c.nodes):
            P0, P1, P2 = O.psi_statistics(d["Xu"], d["pts"][t], d["wts"][t], c.sigma2, d["ell"])
            U += O.multi_average_energy(P0, P1, P2, d["Yn"][targets][t], d["Sig_y"][targets][t], ref["mu"], ref["Sigma"],
                                        d["W"][noise], d["E_logw"][noise], Kinv)
    ref["energy_from_stats"], ref["energy"] = ref["energy"], float(U)
    return ref


def ratios(ref, got):
    """error / bound of everything one rank reports after a sweep (`got`: stats = (Psi2, B, scalars[:SGP_S_COUNT]), post = (mu,
    Sigma, Uv), sum_I1, sum_I2, energy, wishart, ryy -- absent entries are not compared) against `ref` (`reference` or
    `sweep_from_stats`).  Exact properties give 0 or inf."""
    r = {}
    rel = lambda a, b: abs(a - b) / (STAT_TOL * abs(b)) if b != 0 else (0.0 if a == 0 else math.inf)
    do = ref["B"].shape[1]
    if "stats" in got:
        Psi2, B, sc = got["stats"]
        r["Psi2"] = relF(Psi2, ref["Psi2"]) / STAT_TOL                                   # relF < 1e-13
        r["Psi2_symmetric"] = 0.0 if np.array_equal(Psi2, Psi2.T) else math.inf
        r["B"] = relF(B, ref["B"].reshape(B.shape)) / STAT_TOL
        r["S_N"], r["S_W"] = rel(sc[2], ref["scalars"][2]), rel(sc[1], ref["scalars"][1])  # rel_tol 1e-13
        if do == 1:
            r["S_YY"] = rel(sc[0], ref["scalars"][0])
    if got.get("ryy") is not None:
        r["Ryy"] = relF(got["ryy"], ryy_of(ref["scalars"], do)) / STAT_TOL
    tol = ref["post_tol"]                                                                # post_tol(cond(Lambda))
    if "post" in got:
        mu, Sig, Uv = got["post"]
        r["mu"], r["Sigma"], r["Uv"] = relF(mu, ref["mu"]) / tol, relF(Sig, ref["Sigma"]) / tol, relF(Uv, ref["Uv"]) / tol
    tol_I1 = ref["tol_I1"]
    if do == 1 and "sum_I1" in got:
        w = ref["W"][0, 0]
        r["sum_I1"] = abs(got["sum_I1"] - ref["sum_I1"]) / tol_I1                        # test_gpu_shards
        r["sum_I2"] = abs(got["sum_I2"] - ref["sum_I2"]) / (max(1e-7, tol) * abs(ref["sum_I2"]))      # test_gpu_parity
        r["energy"] = abs(got["energy"] - ref["energy"]) / (max(1e-7, tol) * abs(ref["energy"]) + 0.5 * w * tol_I1)
    elif do > 1 and "wishart" in got:
        # test_multisgp_sweep_matches_oracle: the diagonal carries sum I1, the off-diagonal does not
        Sw, S_ref = got["wishart"], ref["wishart"]
        r["wishart"] = float(np.abs(Sw - S_ref).max() / (1e-7 * np.abs(S_ref).max() + tol_I1))
        off = ~np.eye(do, dtype=bool)
        r["wishart_offdiag"] = float(np.max(np.abs(Sw[off] - S_ref[off]) / (1e-9 + 1e-7 * np.abs(S_ref[off]))))
        r["energy"] = abs(got["energy"] - ref["energy"]) / (1e-7 * abs(ref["energy"]) + 0.5 * np.trace(ref["W"]) * tol_I1)
    return r


def worst(r):
    k = max(r, key=lambda q: r[q])
    return k, float(r[k])


# ---------------------------------------------------------------------------------------------------------------------------
# the theta objective (UniSGP): value, analytic gradient and its bound over the whole data at a given q(v)
# ---------------------------------------------------------------------------------------------------------------------------
def moved_theta(name):
    """The kernel parameters of the second evaluation: sigma2 and every lengthscale moved by 10 to 30 %, in both directions."""
    d = inputs(name)
    c = d["case"]
    f = 1.0 + np.where(np.arange(len(d["ell_dev"])) % 2 == 0, 1.0, -1.0) * np.linspace(0.1, 0.3, len(d["ell_dev"]))
    return 1.2 * c.sigma2, d["ell_dev"] * f


def theta_reference(name, mu, Sigma, sigma2=None, ell_dev=None, noise=0):
    """(value, gradient, gradient bound, tol_I1) of train_step_ref's objective over the whole data at q(v) = N(mu, Sigma)."""
    d = inputs(name)
    c = d["case"]
    s2 = c.sigma2 if sigma2 is None else sigma2
    ell_dev = d["ell_dev"] if ell_dev is None else ell_dev
    n_ell, w, y = len(ell_dev), d["W"][noise][0, 0], d["Y"][0][:, 0]
    val = TS.theta_objective(c.family, s2, ell_dev, d["Xu"], d["X"], y, mu, Sigma, w, c.jitter, omega=d["omega"])
    g, b = TS.theta_grad(c.family, s2, ell_dev, n_ell, d["Xu"], d["X"], y, mu, Sigma, w, c.jitter, bound=True, omega=d["omega"])
    Kuu = TS.kernelmatrix(c.family, s2, TS.full_ell(ell_dev, c.D), d["Xu"], d["Xu"]) + c.jitter * np.eye(c.M)
    s_w = float(np.sum(d["omega"])) if d["omega"] is not None else float(c.N)
    return val, g, b, 50 * EPS * float(np.linalg.cond(Kuu)) * s2 * s_w + 1e-12


def data_half(name, r, mu, Sigma, sigma2=None, ell_dev=None, noise=0):
    """Rank r's data half of the gradient -- what it hands the hook, one entry per slot (sigma2, then every DIMENSION's
    lengthscale): w sum_pn omega_n dK_uf o ((R - Kinv) K_uf - mu y') over the rank's points (train_step_ref.theta_grad's first
    term).  The K_uu half and the s_w term come from the reduced statistics."""
    d = inputs(name)
    c = d["case"]
    s2 = c.sigma2 if sigma2 is None else sigma2
    ell = TS.full_ell(d["ell_dev"] if ell_dev is None else ell_dev, c.D)
    lo, hi = c.bounds[r]
    X, y = d["X"][lo:hi], d["Y"][0][lo:hi, 0]
    om = np.ones(hi - lo) if d["omega"] is None else d["omega"][lo:hi]
    Xu, w = d["Xu"], d["W"][noise][0, 0]
    Kinv = np.linalg.inv(TS.kernelmatrix(c.family, s2, ell, Xu, Xu) + c.jitter * np.eye(c.M))
    s_uf = TS.sq_dist(ell, Xu, X)
    Kuf = s2 * TS.kappa(c.family, s_uf)
    A = ((Sigma + np.outer(mu, mu) - Kinv) @ Kuf - np.outer(mu, y)) * om
    dsf = -2.0 * s2 * TS.dkappa_ds(c.family, s_uf)
    d_uf = [Kuf / s2] + [dsf * (Xu[:, k:k + 1] - X[None, :, k]) ** 2 / ell[k] ** 3 for k in range(c.D)]
    return w * np.array([np.sum(A * f) for f in d_uf])


# ---------------------------------------------------------------------------------------------------------------------------
# the simulation
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def overlap_env(value):
    """SGP_OVERLAP for the handles created inside (the library reads it in sgp_create); None leaves the environment alone."""
    saved = os.environ.get("SGP_OVERLAP")
    if value is not None:
        os.environ["SGP_OVERLAP"] = str(value)
    try:
        yield
    finally:
        if value is not None:
            if saved is None:
                os.environ.pop("SGP_OVERLAP", None)
            else:
                os.environ["SGP_OVERLAP"] = saved


class Rank:
    """One rank: its handle and its hook, installed once -- sgp_set_allreduce makes the next sweep a full one, so the hook stays and
    only its mode changes.  "capture": clone the piece; "add": replace the piece by the sum of all ranks' pieces of the same call
    -- the others' captured ones and this rank's own, added in rank order on every rank, as a collective leaves the same bits
    everywhere -- and keep a copy of the sum.  `others`: every rank's captured pieces, None at this rank's own place."""

    def __init__(self, dev):
        import torch
        from gaussianprocessnode_amd.distributed import device_tensor
        self.dev, self.mode, self.store, self.others, self.calls, self.summed = dev, "capture", [], [], [], []

        def hook(ptr, n, stream):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                t = device_tensor(ptr, n)
                if self.mode == "capture":
                    self.store.append(t.clone())
                else:
                    k = len(self.calls)
                    for o in self.others:
                        assert o is None or (k < len(o) and o[k].numel() == n), (k, n, [p.numel() for p in o])
                    parts = [t if o is None else o[k] for o in self.others]
                    acc = parts[0].clone()
                    for part in parts[1:]:
                        acc.add_(part)
                    t.copy_(acc)
                    self.summed.append(acc)
            self.calls.append(n)
        dev.set_allreduce(hook)

    def begin(self, mode, others=()):
        self.mode, self.others, self.calls, self.summed = mode, list(others), [], []
        if mode == "capture":
            self.store = []


def simulate(world, make, ops, apply):
    """`ops` on `world` ranks: make(r) -> a loaded handle, apply(r, dev, op, second) -> the op's result on that rank (second: the
    adding pass).  Returns one record per op: calls (every rank's hook counts in the adding pass), captured (the same in the
    capturing pass), summed (every rank's copies of the summed pieces, NumPy), results (every rank's result of the adding pass)."""
    import torch
    ranks, log = [], []
    try:
        for r in range(world):
            ranks.append(Rank(make(r)))
        for op in ops:
            for r, rk in enumerate(ranks):
                rk.begin("capture")
                apply(r, rk.dev, op, False)
            torch.cuda.synchronize()
            captured = [list(rk.calls) for rk in ranks]
            results = []
            for r, rk in enumerate(ranks):
                rk.begin("add", [None if q is rk else q.store for q in ranks])
                results.append(apply(r, rk.dev, op, True))
            torch.cuda.synchronize()
            log.append(dict(op=op, captured=captured, calls=[list(rk.calls) for rk in ranks],
                            summed=[[t.cpu().numpy() for t in rk.summed] for rk in ranks], results=results))
    finally:
        for rk in ranks:
            rk.dev.close()
    return log


def run(G, name, ops):
    """A sequence of operations of case `name`, every one captured and summed as above:
        ("sweep",)                  a full sweep
        ("targets", k)              set_targets (and set_output_cov_sum) with version k of the targets, then a sweep
        ("noise", k)                set_noise with version k, then a sweep
        ("objective",)              theta_objective with its gradient at the current kernel
        ("kernel_objective", s2, ell)   set_kernel at a new theta, then theta_objective
        ("objective_refused",)      theta_objective, expecting the library's refusal (returns the exception text)
    Sweeps report stats, post, sum_I1 / sum_I2 / energy, wishart (d_out > 1) and kind = sweep_kind(); objectives value, grad and
    kind.  Also returns every rank's overlap_plan() as of the first sweep."""
    d = inputs(name)
    c = d["case"]
    plans = [None] * c.world

    def load(r, dev):
        ri = rank_inputs(name, r)
        dev.set_data(ri["X"], ri["Y"], ri["y_var"], ri["omega"], n_nodes=ri["n_nodes"] if (c.weighted or c.d_out > 1) else None)
        if c.d_out > 1:
            dev.set_output_cov_sum(ri["cov_sum"])

    def make(r):
        dev = G.SGPDevice(c.n_max, c.M, c.D, d_out=c.d_out, reuse_stats=c.reuse)
        dev.set_inducing(d["Xu"])
        load(r, dev)
        dev.set_kernel(c.sigma2, d["ell_dev"], c.jitter, family=c.family)
        if c.prior == "iso":
            dev.set_prior_isotropic(50.0)
        elif c.prior == "precision":
            dev.set_prior_precision(d["xi0"], d["Lambda0"])
        else:
            dev.set_prior_meancov(d["mu0"], d["Sigma0"])
        dev.set_noise(d["W"][0], d["E_logw"][0])
        return dev

    def swept(dev):
        s = dev.scalars()
        out = dict(stats=dev.stats(), post=dev.posterior(), sum_I1=s.sum_I1, sum_I2=s.sum_I2, energy=s.energy, kind=dev.sweep_kind())
        if c.d_out > 1:
            out["wishart"] = dev.wishart_invscale()
        return out

    def apply(r, dev, op, second):
        if op[0] == "sweep":
            if second and c.reuse:
                load(r, dev)                       # (the resident statistics would be reused: the data again, a full sweep again)
            if plans[r] is None:
                plans[r] = dev.overlap_plan()
            dev.sweep()
            return swept(dev)
        if op[0] == "targets":
            ri = rank_inputs(name, r, targets=op[1])
            dev.set_targets(ri["Y"], ri["y_var"])
            if c.d_out > 1:
                dev.set_output_cov_sum(ri["cov_sum"])
            dev.sweep()
            return swept(dev)
        if op[0] == "noise":
            dev.set_noise(d["W"][op[1]], d["E_logw"][op[1]])
            dev.sweep()
            return swept(dev)
        if op[0] == "objective_refused":
            try:
                dev.theta_objective(want_grad=True)
            except G.SGPError as e:
                return dict(refused=str(e))
            return dict(refused=None)
        if op[0] == "kernel_objective":
            dev.set_kernel(op[1], op[2], c.jitter)
        val, grad = dev.theta_objective(want_grad=True)
        return dict(value=val, grad=grad, kind=dev.sweep_kind(), mu=dev.posterior(want_cov=False, want_uv=False)[0])

    with overlap_env(1 if c.overlap else 0):
        log = simulate(c.world, make, ops, apply)
    return log, plans
