"""The bookkeeping of the simulated data-sharded runs (tests/sharded_ref.py) on the CPU, no GPU: every rank's shares add up to the
whole-data values, the exchange buffer's layout as the header states it round-trips, and the cases of
tests/test_gpu_sharded_shapes.py tell a damaged sum from the right one -- a rank left out, Ryy left out of the tail, an off-diagonal
tile without its mirror image, a gradient slot whose data half one rank never contributed -- by at least ten times the bounds
the GPU file asserts."""
import math

import numpy as np
import pytest

from gaussianprocessnode_amd.distributed import shard_bounds
from tests import sharded_ref as R
from tests import train_step_ref as TS

SWEPT = [c.name for c in R.SWEEP_UNI + R.SWEEP_MULTI + R.REUSE if not c.overlap]     # (the overlapped cases share their inputs)


def rank_stats(name, targets=0):
    c = R.CASES[name]
    out = []
    for r in range(c.world):
        ri = R.rank_inputs(name, r, targets)
        Psi2, B, sc = R.oracle_stats(name, ri["lo"], ri["hi"], targets, n_nodes=ri["n_nodes"], cov_sum=ri["cov_sum"])
        out.append((np.tril(Psi2) + np.tril(Psi2, -1).T, B, sc))         # (a BLAS product is symmetric to rounding only)
    return out


# ------------------------------------------------------------------------------------------------
# 1. the shares sum to the whole

@pytest.mark.parametrize("name", sorted(R.CASES))
def test_shards_cover_the_points_with_one_n_max(name):
    c = R.CASES[name]
    assert len(c.sizes) == c.world >= 2 and sum(c.sizes) == c.n_points and 150 <= c.n_points <= 700
    assert c.bounds[0][0] == 0 and c.bounds[-1][1] == c.n_points
    assert all(a[1] == b[0] for a, b in zip(c.bounds, c.bounds[1:]))
    assert len(set(c.sizes)) > 1 and c.n_max == max(c.sizes)                       # uneven
    if c.shards is None:
        assert c.bounds == [shard_bounds(c.n_points, c.world, r) for r in range(c.world)]


@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("targets", [0, 1])
def test_rank_shares_sum_to_the_whole_data_values(name, targets):
    c = R.CASES[name]
    shares = [R.rank_inputs(name, r, targets) for r in range(c.world)]
    assert math.isclose(sum(s["n_nodes"] for s in shares), R.n_nodes_whole(name), rel_tol=1e-13)
    if c.d_out > 1:
        assert any(abs(s["n_nodes"] - round(s["n_nodes"])) > 0.1 for s in shares)  # a shard cuts through a node
        whole = R.inputs(name)["Sig_y"][targets].sum(axis=0)
        assert R.relF(sum(s["cov_sum"] for s in shares), whole) < R.STAT_TOL
    Psi2, B, sc = R.oracle_stats(name, targets=targets)
    parts = rank_stats(name, targets)
    assert R.relF(sum(p[0] for p in parts), Psi2) < R.STAT_TOL                     # relF < 1e-13, as test_gpu_shards
    assert R.relF(sum(p[1] for p in parts), B) < R.STAT_TOL
    tot = sum(p[2] for p in parts)
    for k in (0, 1, 2):                                                            # S_YY, S_W, S_N
        assert math.isclose(tot[k], sc[k], rel_tol=1e-13), k
    assert R.relF(R.ryy_of(tot, c.d_out), R.ryy_of(sc, c.d_out)) < R.STAT_TOL
    if c.d_out > 1:                                                                # the point-wise sums are multi_suff_stats'
        ms = R.whole_multi_stats(name, targets)
        assert R.relF(Psi2, ms.Psi2) < R.STAT_TOL and R.relF(B, ms.B) < R.STAT_TOL
        assert R.relF(R.ryy_of(sc, c.d_out), ms.Ryy) < R.STAT_TOL
        assert math.isclose(sc[1] * c.sigma2, ms.s_kk, rel_tol=1e-13) and math.isclose(sc[2], ms.n, rel_tol=1e-13)


@pytest.mark.parametrize("name", [c.name for c in R.SWEEP_MULTI + R.REUSE if c.d_out > 1])
def test_multisgp_energy_from_summed_statistics_is_the_per_node_sum(name):
    ref = R.reference(name)
    bound = 1e-7 * abs(ref["energy"]) + 0.5 * np.trace(ref["W"]) * ref["tol_I1"]
    assert abs(ref["energy_from_stats"] - ref["energy"]) < bound


# ------------------------------------------------------------------------------------------------
# 2. the exchange buffer's layout

@pytest.mark.parametrize("M", [1, 63, 64, 65, 130, 200, 257])
@pytest.mark.parametrize("d_out", [1, 2, 3, 4])
def test_exchange_buffer_layout_round_trips(M, d_out):
    rng = np.random.default_rng(M + d_out)
    A = rng.normal(size=(M, M + 3))
    Psi2, B = A @ A.T, rng.normal(size=(M, d_out))
    sc = R.scalars_vector(1.5, 2.5, 3.5, rng.normal(size=(d_out, d_out)))
    buf = R.pack_exchange(Psi2, B, sc)
    T, Mp = -(-M // 64), -(-M // 64) * 64
    assert buf.size == R.pack_count(M, d_out) == T * (T + 1) // 2 * 4096 + Mp * d_out + 8 + d_out ** 2
    assert R.tail_count(M, d_out) == Mp * d_out + 8 + d_out ** 2
    P2, B2, sc2 = R.unpack_exchange(buf, M, d_out)
    assert np.array_equal(P2, Psi2) and np.array_equal(B2, B) and np.array_equal(sc2, sc)
    Bt, sct = R.unpack_tail(buf[buf.size - R.tail_count(M, d_out):], M, d_out)
    assert np.array_equal(Bt, B) and np.array_equal(sct, sc)
    # element (i, j) of lower tile (I, J): tile I (I + 1) / 2 + J of the row-major triangle, column-major inside the tile
    for I, J, i, j in [(0, 0, 0, 0), (T - 1, 0, 5, 7), (T - 1, T - 1, 0, 1), (T // 2, T // 3, 63, 62)]:
        row, col = 64 * I + i, 64 * J + j
        want = Psi2[row, col] if row < M and col < M else 0.0
        assert buf[(I * (I + 1) // 2 + J) * 4096 + j * 64 + i] == want
    off = T * (T + 1) // 2 * 4096
    assert buf[off + (d_out - 1) * Mp + M - 1] == B[M - 1, d_out - 1]              # B: Mp x d_out column-major
    assert np.all(buf[off + (d_out - 1) * Mp + M:off + d_out * Mp] == 0.0)         # ... its padded rows zero
    assert list(buf[off + Mp * d_out:off + Mp * d_out + 3]) == [1.5, 2.5, 3.5]     # SGP_S_YY, SGP_S_W, SGP_S_N
    assert buf[-1] == sc[-1] and R.plain_counts(M, d_out) == [buf.size]


def test_group_pieces_add_up_to_the_buffer():
    plan = [dict(tiles=3), dict(tiles=3)]                                          # M = 130 .. 192: six lower tiles in two groups
    assert R.planned_counts(plan, 130, 2) == [3 * 4096 + R.tail_count(130, 2), 3 * 4096]
    assert sum(R.planned_counts(plan, 130, 2)) == R.pack_count(130, 2)


# ------------------------------------------------------------------------------------------------
# 3. the cases see a damaged sum

def oracle_got(name, Psi2, B, sc):
    """What a device that swept over these summed statistics would report, by the oracle."""
    c = R.CASES[name]
    o = R.sweep_from_stats(name, Psi2, B, sc)
    got = dict(stats=(Psi2, B, sc[:R.S_COUNT]), post=(o["mu"], o["Sigma"], o["Uv"]), energy=o["energy"])
    if c.d_out == 1:
        got.update(sum_I1=o["sum_I1"], sum_I2=o["sum_I2"])
    else:
        got.update(wishart=o["wishart"], ryy=R.ryy_of(sc, c.d_out))
    return got


@pytest.mark.parametrize("name", SWEPT)
def test_cases_discriminate_damaged_sums(name):
    c = R.CASES[name]
    ref = dict(R.reference(name))
    if c.d_out > 1:
        ref["energy"] = ref["energy_from_stats"]                  # (both sides from summed statistics)
    bufs = [R.pack_exchange(*p) for p in rank_stats(name)]
    clean = R.ratios(ref, oracle_got(name, *R.unpack_exchange(sum(bufs), c.M, c.d_out)))
    assert max(clean.values()) < 1.0, clean
    # a rank left out of the sum (the last one that holds points)
    out = max(r for r in range(c.world) if c.sizes[r] > 0)
    less = R.ratios(ref, oracle_got(name, *R.unpack_exchange(sum(b for r, b in enumerate(bufs) if r != out), c.M, c.d_out)))
    for k in ("Psi2", "B", "S_N", "S_W", "mu", "Sigma", "energy"):
        assert less[k] >= 10.0, (k, less[k])
    # Ryy left out of the sum: this rank's alone
    if c.d_out > 1:
        buf = sum(bufs)
        buf[buf.size - c.d_out ** 2:] = bufs[0][buf.size - c.d_out ** 2:]
        no_ryy = R.ratios(ref, oracle_got(name, *R.unpack_exchange(buf, c.M, c.d_out)))
        for k in ("Ryy", "wishart", "energy"):
            assert no_ryy[k] >= 10.0, (k, no_ryy[k])
        assert max(v for k, v in no_ryy.items() if k not in ("Ryy", "wishart", "wishart_offdiag", "energy")) < 1.0
    # an off-diagonal tile without its mirror image (cases of one tile row have none)
    if R.tile_rows(c.M) > 1:
        Psi2, B, sc = R.unpack_exchange(sum(bufs), c.M, c.d_out, unmirrored=(1, 0))
        torn = R.ratios(ref, dict(stats=(Psi2, B, sc[:R.S_COUNT])))
        assert torn["Psi2"] >= 10.0 and torn["Psi2_symmetric"] == math.inf
    else:
        assert c.M <= 64


# ------------------------------------------------------------------------------------------------
# 4. the theta gradient: weights in the reference, and a slot one rank never contributed

def test_integer_point_weights_are_repeated_points_in_the_reference_gradient():
    rng = np.random.default_rng(5)
    N, M, D = 40, 9, 2
    X, Xu, y = rng.uniform(-1.5, 1.5, (N, D)), rng.uniform(-1.5, 1.5, (M, D)), rng.normal(size=N)
    om = rng.integers(1, 4, N)
    Xr, yr = np.repeat(X, om, axis=0), np.repeat(y, om)
    mu = rng.normal(size=M)
    A = rng.normal(size=(M, M))
    Sig = A @ A.T / M + 0.1 * np.eye(M)
    for family, n_ell in [("se", 2), ("matern52", 1)]:
        ell = np.array([0.9, 1.3])[:n_ell]
        v = TS.theta_objective(family, 1.2, ell, Xu, X, y, mu, Sig, 3.0, 1e-8, omega=om.astype(float))
        g, b = TS.theta_grad(family, 1.2, ell, n_ell, Xu, X, y, mu, Sig, 3.0, 1e-8, bound=True, omega=om.astype(float))
        vr = TS.theta_objective(family, 1.2, ell, Xu, Xr, yr, mu, Sig, 3.0, 1e-8)
        gr, br = TS.theta_grad(family, 1.2, ell, n_ell, Xu, Xr, yr, mu, Sig, 3.0, 1e-8, bound=True)
        assert math.isclose(v, vr, rel_tol=1e-12)
        np.testing.assert_allclose(g, gr, rtol=1e-11)
        np.testing.assert_allclose(b, br, rtol=1e-11)
        assert np.all(np.abs(g - gr) < 0.01 * b)


@pytest.mark.parametrize("name", [c.name for c in R.THETA])
def test_theta_cases_discriminate_a_slot_that_is_not_summed(name):
    """With the last rank's share of the FIRST or of the LAST payload slot left out of the sum -- slot 32 at D = 32 -- the gradient
    misses train_step_ref's bound by more than ten times, at the sweep's theta and at the moved one."""
    c = R.CASES[name]
    ref = R.reference(name)
    mu, Sigma = ref["mu"], ref["Sigma"]
    for s2, ell_dev in [(None, None), R.moved_theta(name)]:
        _, g, bound, _ = R.theta_reference(name, mu, Sigma, s2, ell_dev)
        halves = [R.data_half(name, r, mu, Sigma, s2, ell_dev) for r in range(c.world)]
        assert all(h.shape == (1 + c.D,) for h in halves)
        if (c.n_ell or c.D) == 1:                                 # one lengthscale: the dimensions' slots are folded afterwards
            halves = [np.array([h[0], h[1:].sum()]) for h in halves]
            slots = [(0, 0), (c.D, 1)]
        else:
            slots = [(0, 0), (c.D, c.D)]
        full = R.data_half(name, c.world - 1, mu, Sigma, s2, ell_dev)
        for slot, comp in slots:
            assert abs(full[slot]) / bound[comp] >= 10.0, (slot, full[slot], bound[comp])
        # ... and so would the whole gradient without any rank's whole data half
        for h in halves:
            assert np.all(np.abs(h) >= 10.0 * bound), (h, bound)
        assert g.shape == halves[0].shape
