"""Data-sharded sweeps, target updates and theta objectives with two or three simulated ranks, beyond the one UniSGP shape of
tests/test_gpu_shards.py: every rank of every case against the whole-data oracle (tests/sharded_ref.py: the cases, the two-pass
all-reduce, the references and `ratios`, error / bound for each compared quantity).  With more than one rank a tail that is too
short, a tile mirrored to the wrong place or a payload slot that is never summed changes the numbers -- with one rank the sum is
the identity and none of them shows.  tests/test_sharded_host.py shows on the CPU that the cases see such damage.

Every bound is one the project already uses, named in `sharded_ref.ratios`: relF < 1e-13 for the summed Psi2 and B and rel_tol
1e-13 for the summed scalars (test_gpu_shards), `post_tol(cond(Lambda))` for q(v), the tol_I1 forms of test_gpu_shards (UniSGP)
and test_multisgp_sweep_matches_oracle (MultiSGP) for sum I1, the energy and the Wishart inverse scale, and train_step_ref's
gradient bound.  Each test prints its worst ratio."""
import math

import numpy as np
import pytest

from tests import sharded_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    pytest.importorskip("torch")
    import gaussianprocessnode_amd as g
    return g


def check_sweep(name, rec, ref, counts):
    """One swept operation: every rank issued `counts`, in both passes, and holds the whole-data result."""
    c = R.CASES[name]
    assert all(q == counts for q in rec["calls"]), (rec["calls"], counts)
    assert rec["captured"] == rec["calls"]
    worst = ("", 0.0)
    for r, got in enumerate(rec["results"]):
        got = dict(got)
        if c.d_out > 1 and rec["summed"][r]:
            # Ryy is no output of sgp_get_stats: the "Ryy" ratio is taken from the sum the simulated collective left in the tail of
            # the piece that carries it, so it checks every rank's PACKED tail (and the simulation), not the copy k_unpack_stats
            # makes of it.  The unpacked Ryy is covered through what is computed from it: the Wishart inverse scale and the energy.
            first = rec["summed"][r][0]
            got["ryy"] = R.ryy_of(first[first.size - (R.S_COUNT + c.d_out ** 2):], c.d_out)
        ratios = R.ratios(ref, got)
        bad = {k: v for k, v in ratios.items() if not v < 1.0}
        assert not bad, (name, r, bad)
        worst = max(worst, R.worst(ratios), key=lambda q: q[1])
    print(f"RATIO {name} {rec['op']}: worst error / bound {worst[1]:.3g} ({worst[0]})")
    return rec


# ------------------------------------------------------------------------------------------------
# 1. full sweeps

@pytest.mark.parametrize("name", [c.name for c in R.SWEEP_UNI + R.SWEEP_MULTI])
def test_every_rank_sweeps_to_the_whole_data_posterior(G, name):
    """Uneven shards (and an empty one), 1 to 4 padded tile rows, the plain and the overlapped order, weights and y_var, the Matern
    families, dense priors, MultiSGP with Ryy in the tail and fractional n_nodes per rank.  The hook counts are the documented ones:
    the whole exchange buffer in the plain order, one piece per statistics group with the tail on the first in the overlapped order
    -- which the library plans for UniSGP only (include/sgp_hip.h, sgp_overlap_plan): the MultiSGP case under SGP_OVERLAP=1 runs, and
    is asserted to run, in the plain order, so the grouped exchange with a d_out > 1 tail cannot be reached and is not tested.  The
    cases with 450 or 451 points on one rank take the many-chunks form of the statistics' assembly on that rank."""
    c = R.CASES[name]
    log, plans = R.run(G, name, [("sweep",)])
    assert all(p == plans[0] for p in plans), plans
    if c.overlap and c.d_out == 1:
        assert len(plans[0]) == 2, plans[0]
        assert sum(g["tiles"] for g in plans[0]) == R.tile_rows(c.M) * (R.tile_rows(c.M) + 1) // 2
    else:
        assert plans[0] == []
    counts = R.planned_counts(plans[0], c.M, c.d_out)
    assert sum(counts) == R.pack_count(c.M, c.d_out)
    check_sweep(name, log[0], R.reference(name), counts)


def weighted_inputs(N, M, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, D))
    Xu = X[rng.permutation(N)[:M]].copy()
    y = np.sin(X.sum(axis=1)) + 0.1 * rng.normal(size=N)
    return X, Xu, y, rng.uniform(0.05, 1.0, N)


# N 700: 44 chunks of 16 points, the many-chunks form of the assembly; N 250: its few-chunks form; N 4000 x 6 lower tiles: the
# SYRK that fills the chip (one workgroup per CU), again more than 24 chunks
@pytest.mark.parametrize("N,M", [(700, 65), (700, 130), (250, 65), (4000, 130)])
def test_weighted_psi2_is_exactly_symmetric_without_a_hook_too(G, N, M):
    """sum_n omega_n k_n k_n' without an all-reduce hook, one handle holding all points: exactly symmetric (include/sgp_hip.h,
    sgp_get_stats) and the oracle's within relF < 1e-13, the bound of the weighted sweeps of test_gpu_kernel_family."""
    from oracle import sgp_oracle as O
    D, s2, ell = 2, 0.9, np.array([0.7, 0.95])
    X, Xu, y, om = weighted_inputs(N, M, D, N + M)
    with G.SGPDevice(N, M, D) as dev:
        dev.set_inducing(Xu)
        dev.set_data(X, y, weights=om)
        dev.set_kernel(s2, ell, 1e-8)
        dev.set_prior_isotropic(50.0)
        dev.set_noise([[30.0]])
        dev.sweep()
        Psi2, B, _ = dev.stats()
    ref = O.suff_stats(Xu, X, y, None, s2, ell, omega=om)
    assert np.array_equal(Psi2, Psi2.T)
    assert R.relF(Psi2, ref.Psi2) < R.STAT_TOL and R.relF(B, ref.b) < R.STAT_TOL


# ------------------------------------------------------------------------------------------------
# 2. new targets and a new noise on handles that reuse their statistics

@pytest.mark.parametrize("name", [c.name for c in R.REUSE])
def test_new_targets_are_summed_through_the_tail_alone_and_a_new_noise_needs_no_collective(G, name):
    c = R.CASES[name]
    log, _ = R.run(G, name, [("sweep",), ("targets", 1), ("noise", 1)])
    check_sweep(name, log[0], R.reference(name), R.plain_counts(c.M, c.d_out))
    tail = c.M + (-c.M % 64)
    tail = tail * c.d_out + 8 + c.d_out ** 2
    assert tail == R.tail_count(c.M, c.d_out)
    rec = check_sweep(name, log[1], R.reference(name, targets=1), [tail])
    assert all(got["kind"] == (R.REUSED, R.TARGETS) for got in rec["results"]), [got["kind"] for got in rec["results"]]
    ref = R.reference(name, targets=1)
    for summed in rec["summed"]:                                 # the sum the hook left: B and the scalars of the whole data
        B, sc = R.unpack_tail(summed[0], c.M, c.d_out)
        assert R.relF(B, ref["B"].reshape(B.shape)) < R.STAT_TOL
        k = 0 if c.d_out == 1 else 1                             # (SGP_S_YY is UniSGP's: MultiSGP keeps Ryy, behind the slots)
        assert R.relF(sc[k:], ref["scalars"][k:]) < R.STAT_TOL
    rec = check_sweep(name, log[2], R.reference(name, targets=1, noise=1), [])
    assert all(got["kind"][1] == R.REUSED for got in rec["results"])


# ------------------------------------------------------------------------------------------------
# 3. the theta objective

def check_objective(name, rec, counts, noise=0, sigma2=None, ell_dev=None, post=None):
    assert all(q == counts for q in rec["calls"]) and rec["captured"] == rec["calls"], (rec["calls"], rec["captured"], counts)
    c = R.CASES[name]
    w = R.inputs(name)["W"][noise][0, 0]
    worst = 0.0
    for r, got in enumerate(rec["results"]):
        mu, Sigma, _ = post[r]                                   # this rank's q(v), held
        assert np.array_equal(got["mu"], mu)
        v_ref, g_ref, bound, tol_I1 = R.theta_reference(name, mu, Sigma, sigma2, ell_dev, noise)
        assert got["grad"].shape == g_ref.shape
        ratio = float(np.max(np.abs(got["grad"] - g_ref) / bound))                       # train_step_ref's gradient bound
        worst = max(worst, ratio)
        assert ratio < 1.0, (name, r, ratio, got["grad"], g_ref)
        assert math.isclose(got["value"], v_ref, rel_tol=1e-8, abs_tol=0.5 * w * tol_I1), (got["value"], v_ref)    # test_gpu_shards
    first = rec["results"][0]
    for got in rec["results"][1:]:                               # identical summed inputs: identical bits on every rank
        assert got["value"] == first["value"] and np.array_equal(got["grad"], first["grad"])
    print(f"RATIO {name} {rec['op'][0]}: worst gradient error / bound {worst:.3g}")


@pytest.mark.parametrize("name", [c.name for c in R.THETA])
def test_sharded_theta_objective_at_the_sweeps_theta_and_at_a_new_one(G, name):
    """D = 1, an isotropic lengthscale at D = 8, all 33 payload slots at D = 32, weights with y_var, Matern-5/2: value and
    gradient of every rank against the analytic whole-data reference at that rank's q(v) -- one exchange (33 doubles) at the
    sweep's theta, two (the statistics, then the gradient) after set_kernel at a theta 10 to 30 % away."""
    c = R.CASES[name]
    s2n, elln = R.moved_theta(name)
    log, _ = R.run(G, name, [("sweep",), ("objective",), ("kernel_objective", s2n, elln)])
    check_sweep(name, log[0], R.reference(name), R.plain_counts(c.M))
    post = [got["post"] for got in log[0]["results"]]
    check_objective(name, log[1], [R.GRAD_SLOTS], post=post)
    check_objective(name, log[2], [R.pack_count(c.M), R.GRAD_SLOTS], sigma2=s2n, ell_dev=elln, post=post)
    assert all(got["kind"][0] == R.FULL for got in log[2]["results"])
    assert all(got["kind"][0] == R.REUSED for got in log[1]["results"])          # (... and before the re-evaluation it was not)
    # the statistics every rank was left with are the whole data's at the new theta
    stats_new = [R.unpack_exchange(s[0], c.M) for s in log[2]["summed"]]
    for Psi2, B, sc in stats_new[1:]:
        assert np.array_equal(Psi2, stats_new[0][0]) and np.array_equal(B, stats_new[0][1]) and np.array_equal(sc, stats_new[0][2])


def test_sharded_multisgp_theta_objective_is_still_refused(G):
    log, _ = R.run(G, "m_o2_m21", [("sweep",), ("objective_refused",)])
    for got in log[1]["results"]:
        assert got["refused"] is not None and "MultiSGP" in got["refused"], got
    assert all(q == [] for q in log[1]["calls"])
